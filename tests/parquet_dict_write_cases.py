"""What the CPU tests (tests/test_parquet_dict_write_host.py) and the GPU tests (tests/test_gpu_parquet_dict_write.py) of the Parquet
writer's "dictionary" option share: the stand-alone program tests/native/parquet_dict_write_check.cpp built at test time, the rules of
the option restated in Python (index width, run kind, the per-launch decision), seeded inputs of chosen cardinalities, and the
comparison of a written file with the table that went in -- values by bit pattern, the chunk metadata, and every chunk's dictionary
against pyarrow.compute.unique of its non-null values (first-occurrence order).  The description of the batches and the value
comparison are parquet_write_cases.py's.  No binary fixture is committed."""
from __future__ import annotations

import json
import os
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pyarrow.parquet as pq

import parquet_write_cases as W

SRC = os.path.join(W.ROOT, "tests", "native", "parquet_dict_write_check.cpp")
MAX_DICTIONARY = 1 << 20
LAUNCH_ROWS = 1 << 20
NON_BOOLEAN = W.ALL_TYPES[1:]


def build_program(directory, sanitized: bool) -> str:
    exe = os.path.join(str(directory), "parquet_dict_write_check_" + ("sanitized" if sanitized else "plain"))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitized else []
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, SRC])
    return exe


def host_write(exe: str, desc: bytes, out_path: str, tmp_dir, dictionary: int) -> dict:
    """runs `write` of the program: the file at out_path and the program's JSON report"""
    desc_path = os.path.join(str(tmp_dir), os.path.basename(out_path) + ".desc")
    with open(desc_path, "wb") as fh:
        fh.write(desc)
    r = subprocess.run([exe, "write", desc_path, out_path, str(dictionary)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"{os.path.basename(exe)} write: exit {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}"
    os.remove(desc_path)
    return json.loads(r.stdout)


def rules(exe: str, command: str, numbers) -> list:
    r = subprocess.run([exe, command] + [str(v) for v in numbers], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


# ---- the rules, restated --------------------------------------------------------------------------------------------------------------
def index_width(entries: int) -> int:
    return max(1, (max(entries, 1) - 1).bit_length())


def varint_len(v: int) -> int:
    return max(1, -(-v.bit_length() // 7))


def run_bytes(w: int, nn: int, all_equal: bool) -> int:
    if nn == 0:
        return 0
    if all_equal:
        return varint_len(nn << 1) + (w + 7) // 8
    groups = (nn + 7) // 8
    return varint_len(groups << 1 | 1) + groups * w


def launches_of(batch_rows, row_group_rows: int, page_rows: int):
    """[[(first row, rows) of every launch] per row group], rows counted over the whole input"""
    per_launch = page_rows if page_rows >= LAUNCH_ROWS else LAUNCH_ROWS // page_rows * page_rows
    groups, launches, filled, at = [], [], 0, 0
    for rows in batch_rows:
        r0 = 0
        while r0 < rows:
            piece = min(rows - r0, row_group_rows - filled)
            launches += [(at + r0 + l0, min(per_launch, piece - l0)) for l0 in range(0, piece, per_launch)]
            r0 += piece
            filled += piece
            if filled == row_group_rows:
                groups.append(launches)
                launches, filled = [], 0
        at += rows
    if filled:
        groups.append(launches)
    return groups


def expected_chunk(valid: np.ndarray, keys, entry_bytes, launches, page_rows: int, limit: int):
    """the sequential rule over one chunk: `keys` the stored key of every row of the whole input (anything hashable), `entry_bytes`
    the bytes of its dictionary entry.  Returns (dictionary keys in id order or None: no dictionary page, [(run, width, rows) per page])"""
    ids, body, plain, held, pages = {}, 0, limit <= 0, 0, []
    for first, rows in launches:
        if not plain:
            fresh, b_new = {}, 0
            for r in range(first, first + rows):
                if valid[r] and keys[r] not in ids and keys[r] not in fresh:
                    fresh[keys[r]] = len(fresh)
                    b_new += entry_bytes[r]
            if len(ids) + len(fresh) > limit or body + b_new > 2 ** 31 - 2:
                plain = True
            else:
                for k in fresh:
                    ids[k] = len(ids)
                body += b_new
                held += 1
        for p0 in range(first, first + rows, page_rows):
            n = min(page_rows, first + rows - p0)
            if plain:
                pages.append(("plain", 0, n))
                continue
            idx = [ids[keys[r]] for r in range(p0, p0 + n) if valid[r]]
            pages.append(("none" if not idx else "rle" if len(set(idx)) == 1 else "packed", index_width(len(ids)), n))
    return (list(ids) if held else None), pages


def column_keys(col, dtype_id: int):
    """(valid, keys, entry bytes) of a pyarrow column for expected_chunk"""
    valid, bits = W.column_bits(col)
    if dtype_id == 12:
        return valid, bits, [0 if b is None else 4 + len(b) for b in bits]
    if dtype_id == 1:  # (Boolean: never dictionary-encoded)
        return valid, [int(b) for b in bits], [0] * len(bits)
    w = W.WIDTH[dtype_id]
    sw = 8 if w == 8 else 4
    if dtype_id in (2, 3):  # Int8 / Int16 are stored sign-extended to 32 bits
        signed = bits.astype({1: np.uint8, 2: np.uint16}[w]).view({1: np.int8, 2: np.int16}[w]).astype(np.int32).view(np.uint32).astype(np.uint64)
        bits = signed
    return valid, [int(b) for b in bits], [sw] * len(bits)


# ---- a written file against the table that went in -------------------------------------------------------------------------------------
def check_file(path: str, schema: pa.Schema, batches, limit: int, row_group_rows: int = W.DEFAULT_ROW_GROUP_ROWS, page_rows: int = W.DEFAULT_PAGE_ROWS, what="",
               report=None):
    """pyarrow's view of a file written under dictionary = limit: the values, the metadata the format fixes, every chunk's dictionary.
    `report`: the host program's view of the same file (encodings, widths and run kinds of every page), checked against the rules.
    Returns {(row group, column): (dictionary entries or None, pages)}."""
    want = pa.Table.from_batches(batches, schema=schema)
    f = pq.ParquetFile(path)
    W.assert_same_table(f.read(), want, what)
    md = f.metadata
    pages = W.expected_pages([b.num_rows for b in batches], row_group_rows, page_rows)
    launches = launches_of([b.num_rows for b in batches], row_group_rows, page_rows)
    assert md.num_rows == want.num_rows and md.num_row_groups == len(pages), (what, md.num_rows, md.num_row_groups, len(pages))
    out = {}
    for c, field in enumerate(schema):
        dt = W.DTYPES[field.type]
        valid, keys, entry_bytes = column_keys(want.column(c), dt)
        row0 = 0
        for g, group in enumerate(pages):
            mg, mc = md.row_group(g), md.row_group(g).column(c)
            where = (what, field.name, g)
            entries, chunk_pages = expected_chunk(valid, keys, entry_bytes, launches[g], page_rows, 0 if dt == 1 else limit)
            out[(g, c)] = (entries, chunk_pages)
            assert [p[2] for p in chunk_pages] == group, where
            assert mc.num_values == mg.num_rows == sum(group) and mc.compression == "UNCOMPRESSED" and mc.path_in_schema == field.name, where
            assert mc.physical_type == W.PHYSICAL[dt] and mc.total_compressed_size == mc.total_uncompressed_size, where
            st = mc.statistics
            assert st is not None and st.has_null_count and not st.has_min_max, where
            assert st.null_count == want.column(c).slice(row0, mg.num_rows).null_count, where
            if entries is None:
                assert not mc.has_dictionary_page and set(mc.encodings) == ({"PLAIN", "RLE"} if field.nullable else {"PLAIN"}), (where, mc.encodings)
            else:
                assert mc.has_dictionary_page and 4 <= mc.dictionary_page_offset < mc.data_page_offset, where
                assert set(mc.encodings) == {"PLAIN", "RLE", "RLE_DICTIONARY"}, (where, mc.encodings)
                # the dictionary itself, in id order: pyarrow.compute.unique of the chunk's non-null values is first-occurrence order
                # (fixed-width values through their stored bit patterns, so that NaN payloads and -0.0 count)
                if all(p[0] != "plain" for p in chunk_pages):  # (a chunk that fell back holds only the entries of its dictionary launches)
                    rows = range(row0, row0 + mg.num_rows)
                    if dt == 12:
                        unique = [v.encode() for v in pc.unique(want.column(c).slice(row0, mg.num_rows).combine_chunks().drop_null()).to_pylist()]
                        got = pq.ParquetFile(path, read_dictionary=[field.name]).read_row_group(g, columns=[field.name]).column(0)
                        for piece in got.chunks:
                            assert [v.encode() for v in piece.dictionary.to_pylist()] == unique, where
                    else:
                        unique = pc.unique(pa.array([keys[r] for r in rows if valid[r]], pa.uint64())).to_pylist()
                    assert entries == unique, where
                if report is not None:  # the dictionary page's body, from the file's bytes: the entries PLAIN, in id order
                    n = report["row_groups"][g]["chunks"][c]["dict_len"]
                    raw = open(path, "rb").read()[mc.data_page_offset - n:mc.data_page_offset]
                    sw = 8 if W.WIDTH.get(dt) == 8 else 4
                    body = b"".join(len(e).to_bytes(4, "little") + e if dt == 12 else int(e).to_bytes(sw, "little") for e in entries)
                    assert raw == body, where
            if report is not None:
                rc = report["row_groups"][g]["chunks"][c]
                assert rc["has_dict"] == (entries is not None) and rc["dict_n"] == (len(entries) if entries is not None else 0), (where, rc)
                assert rc["dict_first"] == (entries is not None), (where, rc)
                assert [(p["run"], p["width"], p["num_values"]) for p in rc["pages"]] == chunk_pages, (where, rc["pages"], chunk_pages)
            row0 += mg.num_rows
    return out


# ---- seeded inputs -----------------------------------------------------------------------------------------------------------------------
def cardinality_column(t: pa.DataType, n: int, distinct: int, rng, null_p: float = 0.0) -> pa.Array:
    """n rows drawn from `distinct` values of the type (all of them occur when n >= distinct), nulls with probability null_p"""
    distinct = max(1, distinct)
    pick = np.concatenate([rng.permutation(distinct)[:n], rng.integers(0, distinct, size=max(0, n - distinct))])
    mask = (rng.random(n) < null_p) if null_p > 0 else None
    if t == pa.string():
        pool = [W.WORDS[i % len(W.WORDS)] + ("" if i < len(W.WORDS) else f"#{i}") for i in range(distinct)]
        return pa.array([pool[i] for i in pick], type=t, mask=mask)
    if pa.types.is_floating(t):
        dt = np.float32 if t == pa.float32() else np.float64
        pool = (np.arange(distinct) * 0.5 - 3.0).astype(dt)
        return pa.array(pool[pick], type=t, mask=mask, from_pandas=False)
    dt = t.to_pandas_dtype()
    ii = np.iinfo(dt)
    span = int(ii.max) - int(ii.min) + 1
    pool = np.array([int(ii.min) + (i * 2654435761) % span if distinct <= span else 0 for i in range(distinct)], dtype=object)
    if distinct <= span and len(set(pool.tolist())) < distinct:  # (narrow types: consecutive values from the minimum)
        pool = np.array([int(ii.min) + i for i in range(distinct)], dtype=object)
    return pa.array(np.array([pool[i % len(pool)] for i in pick], dtype=dt), type=t, mask=mask)


def eleven_schema(nullable: bool, with_boolean: bool = True) -> pa.Schema:
    return pa.schema([pa.field(name, t, nullable=nullable) for name, t in (W.ALL_TYPES if with_boolean else NON_BOOLEAN)])


def cardinality_batch(n: int, distinct: int, nullable: bool, seed: int, null_p: float = 0.125) -> pa.RecordBatch:
    """n rows of the twelve types: the Boolean column as it comes, every other column of `distinct` values (fewer where the type has
    fewer: Int8 / UInt8 hold 256); one null in eight in the nullable form"""
    rng = np.random.default_rng(W.SEED + 7000 + seed)
    cols = []
    for _, t in W.ALL_TYPES:
        if t == pa.bool_():
            cols.append(W.column(t, n, rng, null_p if nullable else 0.0))
        else:
            d = min(distinct, 256) if t in (pa.int8(), pa.uint8()) else min(distinct, 65536) if t in (pa.int16(), pa.uint16()) else distinct
            cols.append(cardinality_column(t, n, d, rng, null_p if nullable else 0.0))
    return pa.RecordBatch.from_arrays(cols, schema=eleven_schema(nullable))


def nulls_batch():
    """192 rows for page_rows = 64: one null in eight, an all-null page between mixed ones, an all-null column, and null Utf8 slots that
    lie over distinct non-empty bytes ("hidden-<row>"): the dictionary must not hold them"""
    n = 64 * 3
    mask = np.zeros(n, dtype=bool)
    mask[64:128] = True
    mask[::8] = True
    rng = np.random.default_rng(W.SEED + 3)
    schema = pa.schema([pa.field("v", pa.int32()), pa.field("none", pa.int64()), pa.field("s", pa.string())])
    words = [f"w{i % 5}" if not mask[i] else f"hidden-{i}" for i in range(n)]
    offsets = np.concatenate([[0], np.cumsum([len(w) for w in words])]).astype(np.int32)
    s = pa.Array.from_buffers(pa.string(), n, [pa.py_buffer(np.packbits(~mask, bitorder="little").tobytes()), pa.py_buffer(offsets.tobytes()),
                                               pa.py_buffer("".join(words).encode())])
    assert s.null_count == int(mask.sum()) and s[9].as_py() == "w4"
    return schema, pa.RecordBatch.from_arrays([pa.array(rng.integers(0, 3, n), pa.int32(), mask=mask), pa.array([None] * n, pa.int64()), s], schema=schema)


SAME16 = ["0123456789abcdef" + t for t in ("", "x", "y", "x" * 300)]  # equal in their first 16 bytes; one of more than 256 bytes


def same16_batch():
    schema = pa.schema([pa.field("s", pa.string(), nullable=False)])
    return schema, pa.RecordBatch.from_arrays([pa.array([SAME16[i % 4] for i in range(200)])], schema=schema)


def edge_batch():
    """the key that equals the device table's empty word (all ones), as UInt64 and as Int64 -1, beside values above 2^63"""
    schema = pa.schema([pa.field("u", pa.uint64()), pa.field("i", pa.int64())])
    return schema, pa.RecordBatch.from_arrays([pa.array([2 ** 64 - 1, 0, 2 ** 64 - 1, 2 ** 63] * 20, pa.uint64()), pa.array([-1, 0, -1, -2 ** 63] * 20, pa.int64())],
                                              schema=schema)


DECISION_SCHEMA = pa.schema([pa.field("v", pa.int32()), pa.field("s", pa.string())])


def decision_batch(vals):
    return pa.RecordBatch.from_arrays([pa.array(vals, pa.int32()), pa.array([f"s{v}" for v in vals])], schema=DECISION_SCHEMA)
