"""CPU tests of the Parquet source (deviation D12): the two HIP-free headers (csrc/dfx_parquet_meta.hpp, csrc/dfx_parquet_rle.hpp)
through tests/native/parquet_check.cpp, a stand-alone program built once plain and once under the host sanitizers, held against
pyarrow's reader over the case matrix of tests/parquet_cases.py; the run decoder alone against a three-line decoder here; damage
that must be reported and never read out of bounds; and what the library answers without a device."""
import json
import os
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import parquet_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "parquet_check.cpp")

DTYPES = {pa.bool_(): 1, pa.int8(): 2, pa.int16(): 3, pa.int32(): 4, pa.int64(): 5, pa.uint8(): 6, pa.uint16(): 7, pa.uint32(): 8, pa.uint64(): 9,
          pa.float32(): 10, pa.float64(): 11, pa.string(): 12}
UNSIGNED = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("parquet_check")
    out = {}
    for name, flags in (("plain", []), ("sanitized", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(d / f"parquet_check_{name}")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, SRC])
        out[name] = exe
    return out


def run(exe, *args, ok=(0,)):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert r.returncode in ok, f"{os.path.basename(exe)} {args[:1]}: exit {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}"
    return json.loads(r.stdout)


def column_bits(col: pa.ChunkedArray):
    """(valid, bit patterns as Python ints / bytes) of a pyarrow column"""
    arr = col.combine_chunks() if isinstance(col, pa.ChunkedArray) else col
    valid = np.asarray(arr.is_valid())
    if arr.type == pa.string():
        return valid, [None if v is None else v.encode() for v in arr.to_pylist()]
    if arr.type == pa.bool_():
        return valid, np.asarray(arr.fill_null(False)).astype(np.uint64)
    zero = pa.scalar(0, type=arr.type)
    v = arr.fill_null(zero).to_numpy(zero_copy_only=False)
    return valid, v.view(UNSIGNED[v.dtype.itemsize]).astype(np.uint64)


def compare_with_pyarrow(d, path, flipped=False):
    f = pq.ParquetFile(path)
    md, truth = f.metadata, f.read()
    schema = truth.schema
    assert d["num_rows"] == md.num_rows and len(d["row_groups"]) == md.num_row_groups
    assert [c["name"] for c in d["columns"]] == schema.names
    assert [c["dtype"] for c in d["columns"]] == [DTYPES[t] for t in schema.types]
    assert [c["optional"] for c in d["columns"]] == [schema.field(i).nullable for i in range(len(schema))]
    assert [c["physical"] for c in d["columns"]] == [f.schema.column(i).physical_type for i in range(len(schema))]
    row0 = 0
    for g, rg in enumerate(d["row_groups"]):
        mg = md.row_group(g)
        assert rg["num_rows"] == mg.num_rows
        for c, ch in enumerate(rg["chunks"]):
            mc = mg.column(c)
            assert ch["total_compressed_size"] == mc.total_compressed_size and ch["num_values"] == mc.num_values and ch["codec"] == mc.compression
            assert ch["data_page_offset"] == mc.data_page_offset
            assert mg.num_rows == 0 or ch["start"]== (mc.dictionary_page_offset if mc.has_dictionary_page else mc.data_page_offset)
            assert sum(p["num_values"] for p in ch["pages"] if p["kind"] != 2) == mg.num_rows
            # (a byte flip inside the footer's list of encodings leaves a valid file whose list no longer names its pages' encodings)
            assert flipped or {p["encoding"] for p in ch["pages"]} <= set(mc.encodings)
            assert (ch["dict_pages"] > 0) == mc.has_dictionary_page
            valid, bits = column_bits(truth.column(c).slice(row0, mg.num_rows))
            assert ch["valid"] == "".join("1" if v else "0" for v in valid), (g, c)
            if "strs" in ch:
                assert [bytes.fromhex(s) if v else None for s, v in zip(ch["strs"], valid)] == bits, (g, c)
            else:
                mine = np.array(ch["bits"], dtype=np.uint64)
                assert np.array_equal(mine[valid], bits[valid]) and not mine[~valid].any(), (g, c)
        row0 += mg.num_rows


# ---- 1. metadata and decode against pyarrow -------------------------------------------------------------------------------------
def test_matrix_against_pyarrow(programs, tmp_path):
    seen, seen_widths = set(), set()
    for i, (name, table, options) in enumerate(PC.cases()):
        path = str(tmp_path / f"{name}.parquet")
        PC.write(table, path, options)
        d = run(programs["sanitized" if i % 4 == 0 else "plain"], "dump", path)
        assert d["code"] == 0, (name, d)
        compare_with_pyarrow(d, path)
        for rg in d["row_groups"]:
            for ch in rg["chunks"]:
                seen |= {(p["kind"], p["encoding"]) for p in ch["pages"]}
                if name == "fallback":
                    assert ch["dict_pages"] > 0 and ch["plain_pages"] > 0, "the chunk must continue in PLAIN pages"
        if name.startswith("dict-"):  # the index width the case is there for was written and decoded (the required Int64 key column)
            distinct = int(name.split("-")[1])
            widths = {p["bit_width"] for rg in d["row_groups"] for p in rg["chunks"][0]["data_pages"] if p["enc"] == 1}
            assert PC.DICT_WIDTH[distinct] in widths, (name, widths)
            seen_widths |= widths
    assert set(PC.DICT_WIDTH.values()) <= seen_widths, seen_widths
    # the matrix reaches every page kind and value encoding of the subset
    assert {(0, "PLAIN"), (3, "PLAIN"), (2, "PLAIN"), (0, "RLE_DICTIONARY"), (3, "RLE_DICTIONARY"), (3, "RLE")} <= seen, seen


# ---- 2. the run decoder alone ---------------------------------------------------------------------------------------------------
def varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def rle_run(count, value, width):
    return varint(count << 1) + int(value).to_bytes((width + 7) // 8, "little")


def packed_run(values, width):
    groups = (len(values) + 7) // 8
    acc = 0
    for i, v in enumerate(values):
        acc |= int(v) << (i * width)
    return varint((groups << 1) | 1) + acc.to_bytes(groups * width, "little")


def reference_decode(stream, width, want):
    """the three-line decoder: header, then count copies of a value or groups * 8 fields of `width` bits"""
    out, pos = [], 0
    while len(out) < want and pos < len(stream):
        h, shift = 0, 0
        while True:
            b = stream[pos]; pos += 1; h |= (b & 0x7F) << shift; shift += 7
            if not b & 0x80:
                break
        if h & 1:
            nbytes = (h >> 1) * width
            acc = int.from_bytes(stream[pos:pos + nbytes], "little"); pos += nbytes
            out += [(acc >> (i * width)) & ((1 << width) - 1) for i in range((h >> 1) * 8)]
        else:
            nb = (width + 7) // 8
            out += [int.from_bytes(stream[pos:pos + nb], "little")] * (h >> 1); pos += nb
    return out[:want]


@pytest.mark.parametrize("width", [0, 1, 2, 7, 8, 9, 24, 32])
def test_hybrid_widths(programs, width):
    rng = np.random.default_rng(width)
    top = (1 << width) - 1
    vals = [int(v) for v in rng.integers(0, top, size=61, endpoint=True)]
    vals[:2] = [top, 0]
    stream = packed_run(vals, width) + rle_run(5, top, width) + packed_run(vals[:8], width) + rle_run(1, vals[3], width) + rle_run(300, 0, width)
    want = 64 + 5 + 8 + 1 + 300
    for exe in programs.values():
        d = run(exe, "hybrid", width, want, stream.hex() or "")
        assert d["err"] == 0 and d["values"] == reference_decode(stream, width, want)
        # a bit-packed run whose last group is padding: 61 values asked of 64
        d = run(exe, "hybrid", width, 61, packed_run(vals, width).hex())
        assert d["err"] == 0 and d["values"] == vals and d["packed_runs"] == 1


def test_hybrid_run_lengths(programs):
    for exe in programs.values():
        for count in (1, 2, 1 << 20):
            s = rle_run(count, 1, 1)
            d = run(exe, "hybrid", 1, count, s.hex())
            assert d["err"] == 0 and d["got"] == count and d["rle_runs"] == 1 and set(d["values"]) == {1}
        s = b"".join(rle_run(3, i & 1, 1) + packed_run([1, 0, 1, 1, 0, 0, 1, 0], 1) for i in range(40))
        d = run(exe, "hybrid", 1, 40 * 11, s.hex())
        assert d["err"] == 0 and d["values"] == reference_decode(s, 1, 40 * 11) and d["rle_runs"] == 40 and d["packed_runs"] == 40
        # malformed: a payload past the end, a header of six bytes, a truncated RLE value
        for bad, width in ((varint((4 << 1) | 1) + b"\x00" * 3, 1), (b"\x80\x80\x80\x80\x80\x01", 1), (varint(8 << 1), 9)):
            d = run(exe, "hybrid", width, 64, bad.hex())
            assert d["err"] != 0


# ---- 3. damage ------------------------------------------------------------------------------------------------------------------
def test_damage_is_reported(programs, tmp_path):
    path = str(tmp_path / "small.parquet")
    PC.small_file(path)
    data = open(path, "rb").read()
    assert len(data) < 4096
    d = run(programs["plain"], "dump", path)
    compare_with_pyarrow(d, path)
    first = d["row_groups"][0]["chunks"][0]
    lo = first["start"]  # the first page header: from the chunk's start to the first byte of the page's levels
    hi = first["data_pages"][0]["lev_off"]
    assert 0 < hi - lo < 64
    res = run(programs["sanitized"], "damage", path, lo, hi)
    assert res["truncations"] == len(data)
    truth = pq.read_table(path)
    survivors = 0
    for pos, val in res["parsed"]:
        flipped = bytearray(data)
        flipped[pos] = val
        fpath = str(tmp_path / "flipped.parquet")
        open(fpath, "wb").write(bytes(flipped))
        try:
            theirs = pq.read_table(fpath)
        except Exception as e:  # noqa: BLE001
            raise AssertionError(f"byte {pos} = {val:#x}: parsed here, pyarrow says {e}")
        # the flipped file is a valid one: pyarrow reads it to the same table as the undamaged file, and so does the decoder here
        assert theirs.equals(truth), f"byte {pos} = {val:#x} changes what pyarrow reads"
        compare_with_pyarrow(run(programs["plain"], "dump", fpath), fpath, flipped=True)
        survivors += 1
    # observed: 204 of 1 256 byte changes (16 %) leave a valid file that reads to the same table -- bytes of created_by and fields no
    # reader interprets (the list of encodings, encoding statistics, column orders, total_byte_size, file_offset).  A changed column
    # name is no such case: the chunk's path_in_schema no longer matches it and the file is refused.
    assert survivors == len(res["parsed"]) and survivors < res["flips"] / 4, (survivors, res["flips"])


def test_handmade_page_damage(programs, tmp_path):
    path = str(tmp_path / "small.parquet")
    PC.small_file(path)
    data = open(path, "rb").read()
    d = run(programs["plain"], "dump", path)
    kcol, scol = d["row_groups"][0]["chunks"][:2]
    spage, kpage = scol["data_pages"][0], kcol["data_pages"][0]
    assert spage["enc"] == 1 and kpage["enc"] == 0

    def damaged(pos, new):
        b = bytearray(data)
        b[pos:pos + len(new)] = new
        p = str(tmp_path / "damaged.parquet")
        open(p, "wb").write(bytes(b))
        for exe in programs.values():
            r = run(exe, "dump", p, ok=(3,))
            assert r["code"] == 2, r
        return r["error"]

    # the first run of the dictionary indices claims 127 groups: it overruns the page
    assert "overruns" in damaged(spage["val_off"], varint((127 << 1) | 1))
    # ... an RLE run of index 7 (what 3 bits can hold) in a dictionary of 7
    assert spage["bit_width"] == 3
    assert "beyond the dictionary" in damaged(spage["val_off"], rle_run(spage["num_values"], 7, 3))
    # the first run of the definition levels overruns the page
    assert "overruns" in damaged(kpage["lev_off"], bytes([0xFF, 0xFF, 0x03]))
    # the dictionary's first string claims 2^32 - 1 bytes
    first = next(s for s in pq.read_table(path).column("s").to_pylist() if s is not None).encode()
    at = data.index(len(first).to_bytes(4, "little") + first, scol["start"])  # (the dictionary holds the strings in order of first use)
    assert "string length" in damaged(at, b"\xff\xff\xff\xff")


def test_utf8_column_beyond_32_bit_offsets_is_refused(programs, tmp_path):
    """The bytes of a dictionary-encoded Utf8 column are not bounded by the file: 2 049 rows of one 1 MiB dictionary entry are a file
    of about 1 MB and a column of 2^31 + 2^20 bytes.  Both decoders sum the lengths in 64 bits and refuse before anything is sized by
    the total (pq::utf8_total_error, the rule dfx_parquet.cpp applies to the kernel's sum); 2^31 - 1 bytes is the most that passes."""
    path = str(tmp_path / "long_entry.parquet")
    t = pa.table({"s": pa.array(["x" * (1 << 20)] * 2049, type=pa.string())})
    pq.write_table(t, path, compression="NONE", use_dictionary=True, dictionary_pagesize_limit=4 << 20)
    assert os.path.getsize(path) < 2 << 20
    for exe in programs.values():
        r = run(exe, "dump", path, ok=(3,))
        assert r["code"] == 8 and "exceeds 2 GB" in r["error"] and str(2049 << 20) in r["error"], r
    # the same shape below the bound decodes: 3 rows of the entry
    pq.write_table(t.slice(0, 3), path, compression="NONE", use_dictionary=True, dictionary_pagesize_limit=4 << 20)
    compare_with_pyarrow(run(programs["plain"], "dump", path), path)


# ---- 4. without a device: the subset's refusals, and the loud failure of a valid file ------------------------------------------
def _source(path, projection=None):
    from datafusion_archive_amd import execution as ex
    return ex.ParquetDataSource(path, projection=projection)


def rejection_files(tmp_path):
    """[(path, projection, status, words the message must hold)]"""
    n = 100
    k = pa.array(np.arange(n), type=pa.int64())
    out = []
    p = str(tmp_path / "snappy.parquet")
    pq.write_table(pa.table({"k": k}), p, compression="SNAPPY")
    out.append((p, None, 5, ["'k'", "SNAPPY"]))
    p = str(tmp_path / "list.parquet")
    pq.write_table(pa.table({"k": k, "l": pa.array([[1, 2]] * n, type=pa.list_(pa.int64()))}), p, compression="NONE")
    out.append((p, None, 5, ["'l'", "group"]))
    p = str(tmp_path / "timestamp.parquet")
    pq.write_table(pa.table({"k": k, "t": pa.array(np.arange(n), type=pa.timestamp("us"))}), p, compression="NONE")
    out.append((p, None, 5, ["'t'", "TIMESTAMP"]))
    p = str(tmp_path / "ok.parquet")
    pq.write_table(pa.table({"k": k, "v": pa.array(np.arange(n) * 0.5)}), p, compression="NONE")
    out.append((p, [0, 2], 4, ["2"]))
    out.append((str(tmp_path / "missing.parquet"), None, 1, ["missing.parquet"]))
    return out


def test_rejections_need_no_device(tmp_path):
    from datafusion_archive_amd import execution as ex
    for path, projection, status, words in rejection_files(tmp_path):
        with pytest.raises(ex.ExecutionError) as e:
            _source(path, projection)
        assert e.value.code == status, (path, str(e.value))
        for w in words:
            assert w in str(e.value), (path, str(e.value))


def test_valid_file_without_a_device_fails_loudly(tmp_path):
    from datafusion_archive_amd import execution as ex
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("a GPU is present: tests/test_gpu_parquet.py reads the file")
    except ImportError:
        pass
    p = str(tmp_path / "ok.parquet")
    pq.write_table(pa.table({"k": pa.array(np.arange(10), type=pa.int64())}), p, compression="NONE")
    with pytest.raises(ex.ExecutionError) as e:
        _source(p)
    assert e.value.code == 8 and "no HIP device available" in str(e.value) and "no CPU fallback" in str(e.value)
