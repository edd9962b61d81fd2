"""Seeded generator of the Parquet source's case matrix (deviation D12), shared by the CPU tests (tests/test_parquet_host.py: the
sequential host decoder against pyarrow) and the GPU tests (tests/test_gpu_parquet.py: the kernels against pyarrow).  Every file is
written at test time into a temporary directory by pyarrow.parquet with compression='NONE'; no binary fixture is committed.

A case is (name, table, write options).  Groups: `types`, `rows`, `nulls`, `dict`, `fallback`, `projection`."""
from __future__ import annotations

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq

SEED = 20240612

NUMERIC = [("i8", pa.int8()), ("i16", pa.int16()), ("i32", pa.int32()), ("i64", pa.int64()), ("u8", pa.uint8()), ("u16", pa.uint16()),
           ("u32", pa.uint32()), ("u64", pa.uint64()), ("f32", pa.float32()), ("f64", pa.float64())]

WORDS = ["", "a", "ab", "abc", "abcd", "prefix", "prefix-1", "prefix-2", "prefix-22", "größe", "日本語のテキスト", "naïve café", "x" * 40,
         "y" * 39 + "z", "Ünïcödé strïng wïth äccénts", "tab\there", "quote\"inside", "comma,inside", " lead", "trail "]


def _numeric_values(t: pa.DataType, n: int, rng) -> np.ndarray:
    if pa.types.is_floating(t):
        dt = np.float32 if t == pa.float32() else np.float64
        fi = np.finfo(dt)
        bits = np.uint32 if dt == np.float32 else np.uint64
        nan_payload = np.array([0x7FC00001, 0xFFC00000, 0x7F800001] if dt == np.float32 else
                               [0x7FF8000000000001, 0xFFF8000000000000, 0x7FF0000000000001], dtype=bits).view(dt)
        special = np.concatenate([np.array([0.0, -0.0, fi.max, fi.min, fi.tiny, fi.smallest_subnormal, -fi.smallest_subnormal, np.inf, -np.inf,
                                            np.nan], dtype=dt), nan_payload])
        v = rng.standard_normal(n).astype(dt) * dt(1e3)
        v[:len(special)] = special[:n]
        return v
    dt = t.to_pandas_dtype()
    ii = np.iinfo(dt)
    v = rng.integers(ii.min, ii.max, size=n, dtype=dt, endpoint=True)
    special = np.array([ii.min, ii.max, 0, 1, ii.max - 1, ii.min + 1 if ii.min < 0 else 2], dtype=dt)
    v[:len(special)] = special[:n]
    return v


def _strings(n: int, rng, distinct: int = 0) -> list:
    if distinct:
        pool = [f"key-{i:05d}" if i % 3 else f"k{i}" for i in range(distinct)]
        return [pool[i] for i in rng.integers(0, distinct, size=n)]
    return [WORDS[i] for i in rng.integers(0, len(WORDS), size=n)]


def _mask(n: int, p: float, rng):
    return None if p <= 0 else (rng.random(n) < p)


def _array(values, t: pa.DataType, mask):
    return pa.array(values, type=t, mask=mask) if mask is not None else pa.array(values, type=t)


def _table(cols, nullable: bool) -> pa.Table:
    """cols: [(name, pa.Array)]"""
    fields = [pa.field(n, a.type, nullable=nullable) for n, a in cols]
    return pa.Table.from_arrays([a for _, a in cols], schema=pa.schema(fields))


def types_table(n: int, nullable: bool, rng) -> pa.Table:
    cols = []
    for name, t in NUMERIC:
        cols.append((name, _array(_numeric_values(t, n, rng), t, _mask(n, 0.2, rng) if nullable else None)))
    cols.append(("b", _array(rng.random(n) < 0.5, pa.bool_(), _mask(n, 0.2, rng) if nullable else None)))
    cols.append(("s", _array(_strings(n, rng), pa.string(), _mask(n, 0.2, rng) if nullable else None)))
    return _table(cols, nullable)


def rows_table(n: int, rng) -> pa.Table:
    fields = [pa.field("k", pa.int64(), nullable=True), pa.field("s", pa.string(), nullable=True), pa.field("v", pa.float64(), nullable=False),
              pa.field("b", pa.bool_(), nullable=True), pa.field("w", pa.int16(), nullable=True)]
    arrays = [_array(rng.integers(-2**62, 2**62, size=n), pa.int64(), _mask(n, 0.2, rng) if n else None),
              _array(_strings(n, rng), pa.string(), _mask(n, 0.2, rng) if n else None),
              pa.array(rng.standard_normal(n), type=pa.float64()),
              _array(rng.random(n) < 0.3, pa.bool_(), _mask(n, 0.2, rng) if n else None),
              _array(rng.integers(-2**15, 2**15, size=n).astype(np.int16), pa.int16(), _mask(n, 0.5, rng) if n else None)]
    return pa.Table.from_arrays(arrays, schema=pa.schema(fields))


NULL_LAYOUTS = ["p0", "p1", "second_page", "alternating", "halves"]


def null_layout_table(layout: str, rng) -> pa.Table:
    n = 10000
    if layout == "p0":
        mask = np.zeros(n, dtype=bool)
    elif layout == "p1":
        mask = np.ones(n, dtype=bool)
    elif layout == "second_page":
        mask = np.zeros(n, dtype=bool)
        mask[1100:1500:3] = True  # the writer closes a page every 1 024 values here: page 0 has no null, page 1 has them all
    elif layout == "alternating":
        mask = (np.arange(n) % 2).astype(bool)
    else:
        mask = np.arange(n) >= 5000
    fields = [pa.field("k", pa.int64(), nullable=True), pa.field("s", pa.string(), nullable=True)]
    arrays = [pa.array(rng.integers(-2**40, 2**40, size=n), type=pa.int64(), mask=mask), pa.array(_strings(n, rng), type=pa.string(), mask=mask)]
    return pa.Table.from_arrays(arrays, schema=pa.schema(fields))


DICT_DISTINCT = [2, 3, 37, 256, 257, 5000, 40000]
DICT_WIDTH = {2: 1, 3: 2, 37: 6, 256: 8, 257: 9, 5000: 13, 40000: 16}  # bits of an index once the dictionary is complete


def dict_table(distinct: int, order: str, rng) -> pa.Table:
    n = max(4000, distinct + distinct // 2)
    keys = np.concatenate([np.arange(distinct), rng.integers(0, distinct, size=n - distinct)])
    keys = np.sort(keys) if order == "sorted" else rng.permutation(keys)
    ints = (keys.astype(np.int64) * 1000003 - 17)
    strs = [f"key-{k:05d}" if k % 3 else f"k{k}" for k in keys]
    fields = [pa.field("k", pa.int64(), nullable=False), pa.field("s", pa.string(), nullable=True), pa.field("f", pa.float32(), nullable=True)]
    arrays = [pa.array(ints, type=pa.int64()), pa.array(strs, type=pa.string(), mask=_mask(n, 0.1, rng)),
              pa.array((keys % 997).astype(np.float32), type=pa.float32(), mask=_mask(n, 0.1, rng))]
    return pa.Table.from_arrays(arrays, schema=pa.schema(fields))


def fallback_table(rng) -> pa.Table:
    """2 801 distinct Int64 values: a dictionary page within dictionary_pagesize_limit=2048 holds at most 256 eight-byte values, so the
    writer necessarily gives the dictionary up inside the chunk and continues in PLAIN pages"""
    n = 6000
    keys = np.concatenate([np.arange(2801), rng.integers(0, 2801, size=n - 2801)])
    fields = [pa.field("k", pa.int64(), nullable=False), pa.field("s", pa.string(), nullable=True)]
    arrays = [pa.array(keys.astype(np.int64) * 7919, type=pa.int64()),
              pa.array([f"string-number-{k:06d}" for k in keys], type=pa.string(), mask=_mask(n, 0.1, rng))]
    return pa.Table.from_arrays(arrays, schema=pa.schema(fields))


def projection_table(rng) -> pa.Table:
    n = 5000
    cols = [("c0", pa.array(rng.integers(0, 50, size=n), type=pa.int64())), ("c1", pa.array(rng.standard_normal(n), type=pa.float64())),
            ("c2", pa.array(_strings(n, rng), type=pa.string())), ("c3", pa.array(rng.integers(-100, 100, size=n).astype(np.int32), type=pa.int32())),
            ("c4", pa.array(rng.random(n) < 0.5, type=pa.bool_())), ("c5", pa.array(rng.standard_normal(n).astype(np.float32), type=pa.float32())),
            ("c6", pa.array(_strings(n, rng, 100), type=pa.string())), ("c7", pa.array(rng.integers(0, 2**63, size=n).astype(np.uint64), type=pa.uint64()))]
    return _table(cols, True)


BASE = dict(compression="NONE", write_statistics=True)


def cases(groups=None):
    """[(name, table, write options)] of the named groups (all by default), in a fixed order"""
    rng = np.random.default_rng(SEED)
    out = []
    for nullable in (True, False):
        for use_dict in (True, False):
            for version in ("1.0", "2.0"):
                name = f"types-{'nullable' if nullable else 'required'}-{'dict' if use_dict else 'plain'}-v{version[0]}"
                out.append((name, types_table(300, nullable, rng), dict(BASE, use_dictionary=use_dict, data_page_version=version, data_page_size=512)))
    for n in (0, 1, 63, 64, 65, 2047, 2048, 2049, 65537):
        for rgs in (1000, 4096):
            if n <= 65 and rgs == 4096:
                continue  # one row group either way
            version = "2.0" if (n + rgs) % 2 else "1.0"
            out.append((f"rows-{n}-rg{rgs}", rows_table(n, rng), dict(BASE, use_dictionary=(n % 2 == 0), data_page_version=version, data_page_size=256,
                                                                      row_group_size=rgs)))
    for layout in NULL_LAYOUTS:
        out.append((f"nulls-{layout}", null_layout_table(layout, rng), dict(BASE, use_dictionary=False, data_page_version="1.0", data_page_size=4096)))
    for d in DICT_DISTINCT:
        for order in ("uniform", "sorted"):
            out.append((f"dict-{d}-{order}", dict_table(d, order, rng), dict(BASE, use_dictionary=True, data_page_version="1.0" if d % 2 else "2.0",
                                                                            data_page_size=2048)))
    out.append(("fallback", fallback_table(rng), dict(BASE, use_dictionary=True, dictionary_pagesize_limit=2048, data_page_size=512)))
    out.append(("projection", projection_table(rng), dict(BASE, use_dictionary=True, row_group_size=2000)))
    if groups is not None:
        out = [c for c in out if c[0].split("-")[0] in groups]
    return out


def write(table: pa.Table, path: str, options: dict) -> None:
    pq.write_table(table, path, **options)


def small_file(path: str) -> None:
    """the file of the damage tests: under 4 KB, six columns (the second a dictionary-encoded Utf8), no ARROW:schema blob"""
    rng = np.random.default_rng(SEED + 1)
    n = 60
    t = pa.Table.from_arrays([pa.array(rng.integers(-1000, 1000, size=n), type=pa.int64(), mask=rng.random(n) < 0.2),
                              pa.array(_strings(n, rng, 7), type=pa.string(), mask=rng.random(n) < 0.2),
                              pa.array(rng.standard_normal(n), type=pa.float64()),
                              pa.array(rng.integers(0, 200, size=n).astype(np.uint8), type=pa.uint8(), mask=rng.random(n) < 0.2),
                              pa.array(rng.random(n) < 0.5, type=pa.bool_()),
                              pa.array(rng.standard_normal(n).astype(np.float32), type=pa.float32(), mask=rng.random(n) < 0.5)],
                             schema=pa.schema([pa.field("k", pa.int64()), pa.field("s", pa.string()), pa.field("v", pa.float64(), nullable=False),
                                               pa.field("u", pa.uint8()), pa.field("b", pa.bool_(), nullable=False), pa.field("f", pa.float32())]))
    pq.write_table(t, path, compression="NONE", use_dictionary=["s"], store_schema=False, write_statistics=False)
