"""CPU tests of the Parquet source's inflate stage (deviation D12, codec 7 = LZ4_RAW): csrc/dfx_parquet_lz4.hpp and the header pass /
body pass of csrc/dfx_parquet_meta.hpp through tests/native/parquet_lz4_check.cpp, a stand-alone program built once plain and once
under the host sanitizers and run directly.  It takes a compressed chunk the way the device does (header pass, every page inflated
into the image, the pages' prologues, body pass, decode) and is held against pyarrow's reader over the LZ4 case matrix and the shape
cases of tests/parquet_lz4_cases.py; damaged blocks and headers must be reported and never read or written out of bounds; and what
the library answers without a device."""
import os
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import parquet_cases as PC
import parquet_lz4_cases as LC
from test_parquet_host import compare_with_pyarrow, run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "parquet_lz4_check.cpp")


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("parquet_lz4_check")
    out = {}
    for name, flags in (("plain", []), ("sanitized", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(d / f"parquet_lz4_check_{name}")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, SRC])
        out[name] = exe
    return out


def check_lz4_chunks(d, path):
    """every chunk of a file with rows is LZ4_RAW, and the image holds what the page headers say"""
    md = pq.ParquetFile(path).metadata
    for g, rg in enumerate(d["row_groups"]):
        for c, ch in enumerate(rg["chunks"]):
            if md.row_group(g).num_rows == 0 and not ch["inflate"]:
                continue
            assert ch["codec_id"] == 7 and md.row_group(g).column(c).compression == "LZ4", (path, g, c)
            assert ch["image_len"] >= sum(p["dst_len"] for p in ch["inflate"])
            assert all(p["dst_off"] % 8 == 0 for p in ch["inflate"])


# ---- 1. the matrix against pyarrow ------------------------------------------------------------------------------------------------
def test_matrix_against_pyarrow(programs, tmp_path):
    seen = set()
    total = {"sequences": 0, "inflated_pages": 0, "stored_pages": 0, "prologue_only_chunks": 0}
    for i, (name, table, options) in enumerate(LC.matrix()):
        assert options["compression"] == "LZ4"
        path = str(tmp_path / f"{name}.parquet")
        PC.write(table, path, options)
        d = run(programs["sanitized" if i % 4 == 0 else "plain"], "dump", path)
        assert d["code"] == 0, (name, d)
        compare_with_pyarrow(d, path)
        check_lz4_chunks(d, path)
        for k in total:
            total[k] += d["lz4"][k]
        for rg in d["row_groups"]:
            for ch in rg["chunks"]:
                seen |= {(p["kind"], p["encoding"]) for p in ch["pages"]}
    assert {(0, "PLAIN"), (3, "PLAIN"), (2, "PLAIN"), (0, "RLE_DICTIONARY"), (3, "RLE_DICTIONARY"), (3, "RLE")} <= seen, seen
    # pages were inflated, V2 pages were stored, and chunks were walked from their prologues alone
    assert all(v > 0 for v in total.values()), total


# ---- 2. the shapes ----------------------------------------------------------------------------------------------------------------
def test_shapes_against_pyarrow_and_coverage(programs, tmp_path):
    total = {k: 0 for k, _ in LC.COVERAGE}
    per_shape = {}
    for name, table, options in LC.shapes():
        path = str(tmp_path / f"{name}.parquet")
        PC.write(table, path, options)
        for exe in programs.values():
            d = run(exe, "dump", path)
            assert d["code"] == 0, (name, d)
            compare_with_pyarrow(d, path)
            check_lz4_chunks(d, path)
        per_shape[name] = d["lz4"]
        for k in total:
            total[k] += d["lz4"][k]
        pages = [p for rg in d["row_groups"] for ch in rg["chunks"] for p in ch["inflate"]]
        if name in ("period-40000", "arange", "far-repeat"):
            assert len(pages) == 1 and pages[0]["dst_len"] > 65536, (name, pages)
        if name == "far-repeat":
            assert pages[0]["dst_len"] > 131072
        if name == "single":
            assert pages[0]["src_len"] == 9 and pages[0]["dst_len"] == 8, pages
        if name == "random-v2":
            assert d["lz4"]["stored_pages"] == 1 and d["lz4"]["inflated_pages"] == 0, d["lz4"]
        if name == "nullable-v2":
            assert all(p["prefix_len"] > 0 for p in pages), pages
        if name.startswith("utf8-dict"):
            assert pages[0]["kind"] == 2 and pages[0]["flags"] & 1, pages  # the dictionary page, compressed
    for key, shape in LC.COVERAGE:
        assert total[key] > 0, f"no shape reaches `{key}` with this pyarrow build (meant to: {shape}); per shape: " + \
            str({n: s[key] for n, s in per_shape.items()})


# ---- 3. damage --------------------------------------------------------------------------------------------------------------------
DAMAGE = ["offset_zero", "offset_beyond_output", "length_chain_to_the_end", "uncompressed_size_plus_1", "uncompressed_size_minus_1",
          "uncompressed_size_above_cap"]


def test_damaged_blocks_and_sizes_are_reported(programs, tmp_path):
    (name, table, options), = [c for c in LC.shapes() if c[0] == "zeros"]
    path = str(tmp_path / "zeros.parquet")
    PC.write(table, path, options)
    for exe in programs.values():
        r = run(exe, "damage", path)
        # every truncation of the compressed page, inflated from a heap block of its own size
        assert r["truncations"] == r["block_len"] > 16 and r["truncations_accepted"] == 0, r
        assert [c["name"] for c in r["cases"]] == DAMAGE, r
        for c in r["cases"]:
            assert "skipped" not in c and c["result"]["code"] == 2, c
        by_name = {c["name"]: c["result"]["error"] for c in r["cases"]}
        # beyond the 255 x cap: refused by the header pass, before an image of that size is allocated
        assert r["cap_value"] > r["cap"] and "more than a block of" in by_name["uncompressed_size_above_cap"], r
        for k in DAMAGE[:5]:
            assert "malformed" in by_name[k], (k, by_name[k])


def test_v2_level_prefix_above_the_page_is_reported(programs, tmp_path):
    path = str(tmp_path / "tiny_v2.parquet")
    t = pa.Table.from_arrays([pa.array([1, None, 3, None, 5], type=pa.int64())], schema=pa.schema([pa.field("k", pa.int64())]))
    pq.write_table(t, path, compression="LZ4", use_dictionary=False, data_page_version="2.0", write_statistics=False)
    for exe in programs.values():
        compare_with_pyarrow(run(exe, "dump", path), path)
        r = run(exe, "damage_v2", path)
        (c,) = r["cases"]
        assert "skipped" not in c and c["result"]["code"] == 2 and "levels" in c["result"]["error"], c


# ---- 4. the library without a device ----------------------------------------------------------------------------------------------
def _gpu_present():
    try:
        import torch
        return torch.cuda.is_available()
    except ImportError:
        return False


def test_lz4_file_passes_the_judgement(tmp_path):
    """an LZ4 file is judged like a valid uncompressed one: without a device it fails loudly for want of one, not for its codec"""
    from datafusion_archive_amd import execution as ex
    p = str(tmp_path / "lz4.parquet")
    pq.write_table(pa.table({"k": pa.array(np.arange(10), type=pa.int64())}), p, compression="LZ4")
    assert pq.ParquetFile(p).metadata.row_group(0).column(0).compression == "LZ4"
    if _gpu_present():
        assert ex.ParquetDataSource(p).schema().names == ["k"]
        return
    with pytest.raises(ex.ExecutionError) as e:
        ex.ParquetDataSource(p)
    assert e.value.code == 8 and "no HIP device available" in str(e.value) and "no CPU fallback" in str(e.value)


def test_other_codecs_stay_refused(tmp_path):
    from datafusion_archive_amd import execution as ex
    k = pa.array(np.arange(100), type=pa.int64())
    for codec in ("ZSTD", "SNAPPY", "GZIP", "BROTLI"):
        if not pa.Codec.is_available(codec.lower()):
            assert codec != "ZSTD", "this pyarrow build cannot write ZSTD"
            continue
        p = str(tmp_path / f"{codec}.parquet")
        pq.write_table(pa.table({"k": k}), p, compression=codec)
        with pytest.raises(ex.ExecutionError) as e:
            ex.ParquetDataSource(p)
        assert e.value.code == 5 and "'k'" in str(e.value) and codec in str(e.value), (codec, str(e.value))
