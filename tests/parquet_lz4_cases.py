"""Files of the LZ4_RAW tests of the Parquet source (deviation D12), shared by the CPU tests (tests/test_parquet_lz4_host.py: the
sequential host decoder against pyarrow) and the GPU tests (tests/test_gpu_parquet_lz4.py: the inflate kernel against pyarrow).
Every file is written at test time by pyarrow.parquet with compression='LZ4' (Parquet codec 7, one raw LZ4 block per page body);
no binary fixture is committed.

matrix():  every case of tests/parquet_cases.py with its options overridden by compression='LZ4'.
shapes():  one column each (required Int64 or Utf8 unless the name says otherwise, use_dictionary=False unless it says `dict`),
           chosen for the sequences the writer's compressor makes of them -- see each line."""
from __future__ import annotations

import numpy as np
import pyarrow as pa

import parquet_cases as PC

PERIODS = [1, 2, 3, 4, 7, 8, 63, 64, 65, 255, 256, 40000]


def matrix(groups=None):
    return [(name, table, dict(options, compression="LZ4")) for name, table, options in PC.cases(groups)]


def _i64(values, nullable=False, mask=None):
    arr = pa.array(np.asarray(values, dtype=np.int64), type=pa.int64(), mask=mask)
    return pa.Table.from_arrays([arr], schema=pa.schema([pa.field("k", pa.int64(), nullable=nullable)]))


def _utf8(values, nullable=False):
    return pa.Table.from_arrays([pa.array(values, type=pa.string())], schema=pa.schema([pa.field("s", pa.string(), nullable=nullable)]))


def _period(p: int, rng) -> np.ndarray:
    """Int64 rows whose bytes repeat with period p: 513 rows (4 104 bytes), or three periods and a bit where p is large (one page of
    more than 64 KB, matches more than 32 768 bytes back)"""
    nbytes = 513 * 8 if p <= 256 else (3 * p + 4000) // 8 * 8
    pattern = rng.integers(1, 256, size=p, dtype=np.uint8)
    return np.resize(pattern, nbytes).view(np.int64)


def shapes():
    """[(name, table, write options)] in a fixed order"""
    rng = np.random.default_rng(PC.SEED + 77)
    base = dict(compression="LZ4", use_dictionary=False, write_statistics=False, data_page_version="1.0", data_page_size=1 << 20)
    out = [("zeros", _i64(np.zeros(5000)), base)]  # two sequences, the match at offset 1 with a long extension
    for p in PERIODS:  # 1, 63, 64, 65: the wave-width edges of the match copy; 40000: an offset of 32 768 or more
        out.append((f"period-{p}", _i64(_period(p, rng)), base))
    out.append(("arange", _i64(np.arange(20000)), base))  # thousands of short sequences, a page of 160 000 bytes
    random = rng.integers(-2**62, 2**62, size=5000)
    out.append(("random-v1", _i64(random), base))  # one literal-only sequence with an extension; compressed_size > uncompressed_size
    out.append(("random-v2", _i64(random), dict(base, data_page_version="2.0")))  # is_compressed false: a stored page
    out.append(("tile-40", _i64(np.tile(rng.integers(-2**62, 2**62, size=40), 100)), base))  # one overlapping match at offset 320, both extensions
    out.append(("single", _i64([-7]), base))  # a block of 9 bytes
    half = rng.integers(-2**62, 2**62, size=9000)  # 72 000 bytes: the repeat is beyond the 64 KB window and cannot be a match
    out.append(("far-repeat", _i64(np.concatenate([half, half])), base))
    mask = rng.random(3000) < 0.3
    out.append(("nullable-v2", _i64(np.arange(3000) % 11, nullable=True, mask=mask), dict(base, data_page_version="2.0")))  # the level prefix
    out.append(("nullable-v1", _i64(np.arange(3000) % 11, nullable=True, mask=mask), base))  # the probe offset follows the levels
    words = [f"word-{i % 97:03d}-{'x' * (i % 13)}" for i in range(4000)]
    out.append(("utf8-plain", _utf8(words), base))  # length chains walked over the inflated image
    out.append(("utf8-dict", _utf8(words), dict(base, use_dictionary=True)))  # a compressed dictionary page
    out.append(("utf8-dict-v2", _utf8(words), dict(base, use_dictionary=True, data_page_version="2.0")))
    out.append(("bool-v2", pa.Table.from_arrays([pa.array(np.arange(5000) % 3 == 0)], schema=pa.schema([pa.field("b", pa.bool_(), nullable=False)])),
                dict(base, data_page_version="2.0")))  # RLE Booleans: the 4-byte length read from the prologue
    return out


# what the shapes must reach between them (keys of the native program's `lz4` object), and the shape that is there for it
COVERAGE = [("lit_extensions", "random-v1, tile-40"), ("match_extensions", "zeros, tile-40"), ("offset_1", "zeros, period-1"), ("offset_lt8", "period-3, period-7"),
            ("offset_ge64", "period-64, tile-40"), ("offset_ge32768", "period-40000"), ("overlapping", "zeros, period-3"), ("stored_pages", "random-v2"),
            ("oversized_v1_pages", "random-v1")]
