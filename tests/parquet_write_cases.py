"""What the CPU tests (tests/test_parquet_write_host.py) and the GPU tests (tests/test_gpu_parquet_write.py) of the Parquet writer
(deviation D13) share: the stand-alone program tests/native/parquet_write_check.cpp built at test time, the binary description of
Arrow batches it reads, seeded inputs, and the comparison of a written file with the table that went in -- through pyarrow's reader,
bit for bit, and through the file's metadata.  No binary fixture is committed."""
from __future__ import annotations

import json
import os
import struct
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "parquet_write_check.cpp")
SEED = 20240913

DTYPES = {pa.bool_(): 1, pa.int8(): 2, pa.int16(): 3, pa.int32(): 4, pa.int64(): 5, pa.uint8(): 6, pa.uint16(): 7, pa.uint32(): 8, pa.uint64(): 9,
          pa.float32(): 10, pa.float64(): 11, pa.string(): 12}
WIDTH = {2: 1, 3: 2, 4: 4, 5: 8, 6: 1, 7: 2, 8: 4, 9: 8, 10: 4, 11: 8}
PHYSICAL = {1: "BOOLEAN", 2: "INT32", 3: "INT32", 4: "INT32", 5: "INT64", 6: "INT32", 7: "INT32", 8: "INT32", 9: "INT64", 10: "FLOAT", 11: "DOUBLE",
            12: "BYTE_ARRAY"}
UNSIGNED = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
DEFAULT_ROW_GROUP_ROWS, DEFAULT_PAGE_ROWS = 1 << 20, 1 << 15

ALL_TYPES = [("b", pa.bool_()), ("i8", pa.int8()), ("i16", pa.int16()), ("i32", pa.int32()), ("i64", pa.int64()), ("u8", pa.uint8()), ("u16", pa.uint16()),
             ("u32", pa.uint32()), ("u64", pa.uint64()), ("f32", pa.float32()), ("f64", pa.float64()), ("s", pa.string())]
WORDS = ["", "a", "ab", "abc", "prefix-1", "größe", "日本語のテキスト", "naïve café", "x" * 40, "tab\there", "quote\"inside", "comma,inside", " lead", "trail ",
         "𝄞 clef"]


def build_program(directory, sanitized: bool) -> str:
    exe = os.path.join(str(directory), "parquet_write_check_" + ("sanitized" if sanitized else "plain"))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitized else []
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, SRC])
    return exe


# ---- the description the program reads ---------------------------------------------------------------------------------------------
def _buffer(buf, nbytes: int) -> bytes:
    raw = b"" if buf is None or nbytes == 0 else buf.to_pybytes()[:nbytes]
    assert len(raw) == nbytes, (len(raw), nbytes)
    return struct.pack("<Q", nbytes) + raw


def describe(schema: pa.Schema, batches, row_group_rows: int = DEFAULT_ROW_GROUP_ROWS, page_rows: int = DEFAULT_PAGE_ROWS) -> bytes:
    """the Arrow buffers of `batches` as they are -- offsets of slices included -- each cut to exactly the bytes its rows reach"""
    out = [b"PQWD", struct.pack("<QQI", row_group_rows, page_rows, len(schema))]
    for f in schema:
        name = f.name.encode()
        out.append(struct.pack("<I", len(name)) + name + struct.pack("<II", DTYPES[f.type], 1 if f.nullable else 0))
    out.append(struct.pack("<I", len(batches)))
    for b in batches:
        out.append(struct.pack("<Q", b.num_rows))
        for i, f in enumerate(schema):
            arr = b.column(i)
            assert arr.type == f.type, (arr.type, f.type)
            off, n, bufs = arr.offset, len(arr), arr.buffers()
            end = off + n
            out.append(struct.pack("<Q", off))
            out.append(_buffer(bufs[0] if arr.null_count else None, (end + 7) // 8 if arr.null_count else 0))
            if f.type == pa.string():
                last = struct.unpack_from("<i", bufs[1].to_pybytes(), 4 * end)[0] if bufs[1] is not None and bufs[1].size >= 4 * (end + 1) else 0
                out.append(_buffer(None, 0))
                if bufs[1] is None or bufs[1].size < 4 * (end + 1):  # an empty array may come without offsets
                    assert n == 0
                    out.append(struct.pack("<Q", 4 * (end + 1)) + bytes(4 * (end + 1)))
                else:
                    out.append(_buffer(bufs[1], 4 * (end + 1)))
                out.append(_buffer(bufs[2], last))
            else:
                nbytes = (end + 7) // 8 if f.type == pa.bool_() else end * WIDTH[DTYPES[f.type]]
                if bufs[1] is None or bufs[1].size < nbytes:
                    assert n == 0
                    out.append(struct.pack("<Q", nbytes) + bytes(nbytes))
                else:
                    out.append(_buffer(bufs[1], nbytes))
                out.append(_buffer(None, 0))
                out.append(_buffer(None, 0))
    return b"".join(out)


def host_write(exe: str, desc: bytes, out_path: str, tmp_dir) -> dict:
    """runs `write` of the program: the file at out_path and the program's JSON report"""
    desc_path = os.path.join(str(tmp_dir), os.path.basename(out_path) + ".desc")
    with open(desc_path, "wb") as fh:
        fh.write(desc)
    r = subprocess.run([exe, "write", desc_path, out_path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"{os.path.basename(exe)} write: exit {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}"
    os.remove(desc_path)
    return json.loads(r.stdout)


# ---- the geometry, restated ---------------------------------------------------------------------------------------------------------
def expected_pages(batch_rows, row_group_rows: int, page_rows: int):
    """[[rows of every page] per row group] for batches of the given row counts"""
    groups, pages, filled = [], [], 0
    for rows in batch_rows:
        r0 = 0
        while r0 < rows:
            piece = min(rows - r0, row_group_rows - filled)
            pages += [min(page_rows, piece - p0) for p0 in range(0, piece, page_rows)]
            r0 += piece
            filled += piece
            if filled == row_group_rows:
                groups.append(pages)
                pages, filled = [], 0
    if filled:
        groups.append(pages)
    return groups


def expected_runs(valid: np.ndarray, pages):
    """the level-run kind of every page of a nullable column whose rows' validity is `valid`: by the page's own non-null count"""
    out, r0 = [], 0
    for group in pages:
        kinds = []
        for n in group:
            k = int(valid[r0:r0 + n].sum())
            kinds.append("rle1" if k == n else "rle0" if k == 0 else "packed")
            r0 += n
        out.append(kinds)
    return out


# ---- comparisons --------------------------------------------------------------------------------------------------------------------
def column_bits(col):
    """(valid, bit patterns / bytes) of a pyarrow column: floats through their integer views, so NaN payloads and -0.0 count"""
    arr = col.combine_chunks() if isinstance(col, pa.ChunkedArray) else col
    valid = np.asarray(arr.is_valid()).astype(bool)
    if arr.type == pa.string():
        return valid, [None if v is None else v.encode() for v in arr.to_pylist()]
    if arr.type == pa.bool_():
        return valid, np.asarray(arr.fill_null(False)).astype(np.uint64)
    w = WIDTH[DTYPES[arr.type]]
    buf = arr.buffers()[1]
    raw = np.frombuffer(buf, dtype=UNSIGNED[w], count=arr.offset + len(arr))[arr.offset:] if len(arr) else np.zeros(0, dtype=UNSIGNED[w])
    return valid, raw.astype(np.uint64)


def assert_same_table(got: pa.Table, want: pa.Table, what=""):
    assert got.schema.names == want.schema.names and got.schema.types == want.schema.types, (what, got.schema, want.schema)
    assert [f.nullable for f in got.schema] == [f.nullable for f in want.schema], (what, got.schema, want.schema)
    assert got.num_rows == want.num_rows, (what, got.num_rows, want.num_rows)
    for c in range(want.num_columns):
        gv, gb = column_bits(got.column(c))
        wv, wb = column_bits(want.column(c))
        assert np.array_equal(gv, wv), f"{what}: validity of column {want.schema.names[c]}"
        if isinstance(wb, list):
            assert gb == wb, f"{what}: column {want.schema.names[c]}"
        else:
            assert np.array_equal(gb[wv], wb[wv]), f"{what}: column {want.schema.names[c]}"


def check_file(path: str, schema: pa.Schema, batches, row_group_rows: int = DEFAULT_ROW_GROUP_ROWS, page_rows: int = DEFAULT_PAGE_ROWS, what=""):
    """pyarrow's view of a written file: the table that went in, and the metadata the format fixes"""
    want = pa.Table.from_batches(batches, schema=schema)
    f = pq.ParquetFile(path)
    assert_same_table(f.read(), want, what)
    md = f.metadata
    pages = expected_pages([b.num_rows for b in batches], row_group_rows, page_rows)
    assert md.num_rows == want.num_rows and md.num_row_groups == len(pages), (what, md.num_rows, md.num_row_groups, len(pages))
    assert "dfx_parquet_write" in md.created_by, md.created_by
    row0 = 0
    for g, group in enumerate(pages):
        mg = md.row_group(g)
        assert mg.num_rows == sum(group), (what, g)
        for c, field in enumerate(schema):
            mc = mg.column(c)
            assert mc.num_values == mg.num_rows and mc.compression == "UNCOMPRESSED" and mc.path_in_schema == field.name, (what, g, c)
            assert mc.physical_type == PHYSICAL[DTYPES[field.type]], (what, g, c, mc.physical_type)
            assert set(mc.encodings) == ({"PLAIN", "RLE"} if field.nullable else {"PLAIN"}), (what, g, c, mc.encodings)
            assert not mc.has_dictionary_page and mc.total_compressed_size == mc.total_uncompressed_size, (what, g, c)
            st = mc.statistics
            assert st is not None and st.has_null_count and not st.has_min_max, (what, g, c)
            assert st.null_count == want.column(c).slice(row0, mg.num_rows).null_count, (what, g, c)
            assert f.schema.column(c).max_definition_level == (1 if field.nullable else 0), (what, c)
        row0 += mg.num_rows
    return md


# ---- seeded inputs ------------------------------------------------------------------------------------------------------------------
def _values(t: pa.DataType, n: int, rng):
    if t == pa.bool_():
        return rng.random(n) < 0.5
    if t == pa.string():
        return [WORDS[i] for i in rng.integers(0, len(WORDS), size=n)]
    if pa.types.is_floating(t):
        dt = np.float32 if t == pa.float32() else np.float64
        bits = np.uint32 if dt == np.float32 else np.uint64
        fi = np.finfo(dt)
        nan_payload = np.array([0x7FC00001, 0xFFC00000, 0x7F800001] if dt == np.float32 else
                               [0x7FF8000000000001, 0xFFF8000000000000, 0x7FF0000000000001], dtype=bits).view(dt)
        special = np.concatenate([np.array([0.0, -0.0, fi.max, fi.min, fi.tiny, fi.smallest_subnormal, np.inf, -np.inf, np.nan], dtype=dt), nan_payload])
        v = (rng.standard_normal(n) * 1e3).astype(dt)
        k = min(n, len(special))
        at = rng.permutation(n)[:k]
        v[at] = special[:k]
        return v
    dt = t.to_pandas_dtype()
    ii = np.iinfo(dt)
    v = rng.integers(ii.min, ii.max, size=n, dtype=dt, endpoint=True)
    special = np.array([ii.min, ii.max, 0, 1], dtype=dt)
    k = min(n, len(special))
    at = rng.permutation(n)[:k]
    v[at] = special[:k]
    return v


def column(t: pa.DataType, n: int, rng, null_p: float = 0.0) -> pa.Array:
    values = _values(t, n, rng)
    mask = (rng.random(n) < null_p) if null_p > 0 else None
    if isinstance(values, np.ndarray) and pa.types.is_floating(t):
        return pa.array(values, type=t, mask=mask, from_pandas=False)
    return pa.array(values, type=t, mask=mask) if mask is not None else pa.array(values, type=t)


def all_types_schema(nullable: bool) -> pa.Schema:
    return pa.schema([pa.field(name, t, nullable=nullable) for name, t in ALL_TYPES])


def all_types_batch(n: int, nullable: bool, seed: int) -> pa.RecordBatch:
    """n rows of all twelve types; nulls (about one row in five) in every column of the nullable form"""
    rng = np.random.default_rng(SEED + seed)
    schema = all_types_schema(nullable)
    return pa.RecordBatch.from_arrays([column(t, n, rng, 0.2 if nullable else 0.0) for _, t in ALL_TYPES], schema=schema)


def run_kinds_batch():
    """192 rows for page_rows = 64: a page without a valid row, a page without a null, a mixed page -- in one chunk"""
    rng = np.random.default_rng(SEED + 7)
    mask = np.concatenate([np.ones(64, dtype=bool), np.zeros(64, dtype=bool), rng.random(64) < 0.5])
    mask[128], mask[129] = True, False  # (mixed whatever the seed gives)
    schema = pa.schema([pa.field("k", pa.int64()), pa.field("b", pa.bool_()), pa.field("s", pa.string())])
    arrays = [pa.array(rng.integers(-2**40, 2**40, size=192), type=pa.int64(), mask=mask), pa.array(rng.random(192) < 0.5, type=pa.bool_(), mask=mask),
              pa.array([WORDS[i] for i in rng.integers(0, len(WORDS), size=192)], type=pa.string(), mask=mask)]
    return schema, pa.RecordBatch.from_arrays(arrays, schema=schema), ~mask


def boolean_batch(n: int = 1000):
    """Boolean with nulls: the dense bits of a page cross byte and word boundaries at every tile"""
    rng = np.random.default_rng(SEED + 11)
    schema = pa.schema([pa.field("b", pa.bool_()), pa.field("r", pa.bool_(), nullable=False)])
    arrays = [pa.array(rng.random(n) < 0.5, type=pa.bool_(), mask=rng.random(n) < 0.3), pa.array(rng.random(n) < 0.5, type=pa.bool_())]
    return schema, pa.RecordBatch.from_arrays(arrays, schema=schema)


def utf8_batch():
    """six tiles: short values, empty strings, nulls, multi-byte characters; one 20 kB value in the middle of tile 2; tile 4 only empty strings"""
    rng = np.random.default_rng(SEED + 13)
    n = 64 * 6
    s = [WORDS[i] for i in rng.integers(0, len(WORDS), size=n)]
    s[64 * 2 + 31] = ("0123456789 größe 日本 " * 1000)[:20000]
    for i in range(64 * 4, 64 * 5):
        s[i] = ""
    mask = rng.random(n) < 0.15
    mask[64 * 2 + 31] = False
    mask[64 * 4:64 * 5] = False
    schema = pa.schema([pa.field("id", pa.int32(), nullable=False), pa.field("s", pa.string()), pa.field("t", pa.string(), nullable=False)])
    arrays = [pa.array(np.arange(n, dtype=np.int32)), pa.array(s, type=pa.string(), mask=mask), pa.array(list(reversed(s)), type=pa.string())]
    return schema, pa.RecordBatch.from_arrays(arrays, schema=schema)
