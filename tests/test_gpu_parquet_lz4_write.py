"""GPU tests of the Parquet writer's "compression" option (dfx_parquet_write with {"compression": 7}, deviation D13; kernels:
csrc/dfx_k_parquet_write_lz4.hip).  Every file is held three ways: pyarrow reads back the table that went in, bit for bit, with the
chunk metadata; the library's own source (dfx_parquet_datasource_new) reads back the same table, inflating the pages on the device;
and the file's BYTES equal what the sequential host encoder (tests/native/parquet_lz4_write_check.cpp over
csrc/dfx_parquet_lz4_enc.hpp) writes for the same batches and options.  The counters are held against the host program's dump of the
file.  No test feeds a kernel damaged input or tries to trip a guard."""
import os
import sys

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle  # noqa: E402
import parquet_dict_write_cases as D  # noqa: E402
import parquet_lz4_write_cases as Z  # noqa: E402
import parquet_write_cases as W  # noqa: E402
from gpu_util import assert_groups_identical  # noqa: E402

from datafusion_archive_amd import execution as ex  # noqa: E402
from datafusion_archive_amd.logicalplan import AggregateFunction, Column, DataType  # noqa: E402

pytestmark = pytest.mark.gpu
LZ4 = ["parquet_write_lz4_pages", "parquet_write_lz4_bytes_in", "parquet_write_lz4_bytes_out", "parquet_write_lz4_sequences"]
COUNTERS = ["parquet_write_pages", "parquet_write_bytes", "parquet_write_row_groups", "parquet_write_dict_pages"] + LZ4


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return Z.build_program(tmp_path_factory.mktemp("parquet_lz4_write_check"), False)


def read_back(path):
    """(the table through the library's own source, the pages it inflated on the device)"""
    ex.counter_reset()
    src = ex.ParquetDataSource(path)
    schema = src.schema()
    table = pa.Table.from_batches(list(src), schema=schema)
    return table, ex.counter_get("parquet_inflated_pages")


def write(path, schema, batches, relation, options):
    rel = relation if relation is not None else ex.DataSourceRelation(schema, batches)
    ex.counter_reset()
    rows, nbytes = ex.write_parquet(rel, path, options)
    counters = {k: ex.counter_get(k) for k in COUNTERS}
    assert rows == sum(b.num_rows for b in batches)
    assert nbytes == os.path.getsize(path) == counters["parquet_write_bytes"]
    assert not os.path.exists(path + ".dfx-partial")
    return counters


def assert_same_bytes(path, other, name):
    got, want = open(path, "rb").read(), open(other, "rb").read()
    if got != want:
        at = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError(f"{name}: the file differs from {os.path.basename(other)} at byte {at} of {len(got)} / {len(want)}: "
                             f"{got[max(0, at - 16):at + 16].hex()} != {want[max(0, at - 16):at + 16].hex()}")


def write_and_check(program, tmp_path, schema, batches, dictionary=0, relation=None, options=None, name="out.parquet"):
    """writes `relation` (default: the batches as a host stream) under compression = 7 and holds the file the three ways; `batches`:
    the batches as the sink receives them.  Returns (path, counters of the call, the host program's pages of the file, its report)."""
    path = str(tmp_path / name)
    options = dict(options or {})
    rg, pr = options.get("row_group_rows", W.DEFAULT_ROW_GROUP_ROWS), options.get("page_rows", W.DEFAULT_PAGE_ROWS)
    options["compression"] = ex.PARQUET_COMPRESSION_LZ4_RAW
    if dictionary:
        options["dictionary"] = dictionary
    counters = write(path, schema, batches, relation, options)
    report = Z.host_write(program, W.describe(schema, batches, rg, pr), path + ".host", tmp_path, dictionary)
    assert report["code"] == 0 and report["reader_code"] == 0 and report["mismatch"] == "", {k: report[k] for k in report if k != "row_groups"}
    assert_same_bytes(path, path + ".host", name)
    pages = Z.check_file(path, schema, batches, report, rg, pr, what=name)
    want = pa.Table.from_batches(batches, schema=schema)
    got, inflated = read_back(path)
    W.assert_same_table(got, want, name + " through dfx_parquet_datasource_new")
    assert (inflated > 0) == (want.num_rows > 0), (name, inflated, len(pages))
    # the counters against the dump: every page of the file is a block, dictionary pages included; both header sizes; the sequences
    assert counters["parquet_write_lz4_pages"] == len(pages), (name, counters)
    assert counters["parquet_write_pages"] == sum(1 for p in pages if p["type"] == 0) and counters["parquet_write_dict_pages"] == sum(1 for p in pages if p["type"] == 2)
    assert counters["parquet_write_lz4_bytes_in"] == sum(p["uncompressed"] for p in pages), (name, counters)
    assert counters["parquet_write_lz4_bytes_out"] == sum(p["compressed"] for p in pages), (name, counters)
    assert counters["parquet_write_lz4_sequences"] == report["encoder"]["sequences"] == sum(p["sequences"] for p in pages), (name, counters)
    return path, counters, pages, report


# ---- the file matrix of the CPU tests --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dictionary", [0, 16])
@pytest.mark.parametrize("nullable", [True, False])
@pytest.mark.parametrize("n", [0, 1, 7, 64, 65, 1000])
def test_all_types_through_host_streams(program, tmp_path, n, nullable, dictionary):
    b = D.cardinality_batch(n, 5, nullable, n) if dictionary else W.all_types_batch(n, nullable, n)
    schema = D.eleven_schema(nullable) if dictionary else W.all_types_schema(nullable)
    for page_rows in (64, 128):
        write_and_check(program, tmp_path, schema, [b], dictionary, options={"row_group_rows": 250, "page_rows": page_rows}, name=f"p{page_rows}.parquet")


@pytest.mark.parametrize("dictionary", [0, 16])
@pytest.mark.parametrize("nullable", [True, False])
def test_all_types_through_a_resident_scan_at_a_row_offset(program, tmp_path, nullable, dictionary):
    schema = D.eleven_schema(nullable)
    whole = [D.cardinality_batch(1500, 9, nullable, 410 + i) for i in range(2)]
    table = ex.DeviceTable.from_batches(schema, whole)
    begin = 64 * 3
    seen = pa.Table.from_batches(whole, schema=schema).combine_chunks().slice(begin, 1000).to_batches()
    for page_rows in (64, 128):
        write_and_check(program, tmp_path, schema, seen, dictionary, relation=table.scan(0, begin, 1000), options={"row_group_rows": 250, "page_rows": page_rows},
                        name=f"resident{page_rows}.parquet")


# ---- one-column shapes: the sequence count of each comes from the host program's dump ---------------------------------------------------
@pytest.mark.parametrize("shape", Z.shapes(), ids=[s[0] for s in Z.shapes()])
def test_shapes(program, tmp_path, shape):
    name, schema, batch, page_rows, dictionary = shape
    _, c, pages, report = write_and_check(program, tmp_path, schema, [batch], dictionary, options={"page_rows": page_rows}, name=name + ".parquet")
    data = [p for p in pages if p["type"] == 0]
    if "pages-of" not in name:
        assert len(data) == 1, (name, len(data))
    assert c["parquet_write_lz4_sequences"] == sum(p["sequences"] for p in pages), name  # (what write_and_check asked as well: by name here)
    if name == "zeros":  # 40 000 zero bytes: 64 literals, one match at offset 1 to the end less 5, the last 5 literals
        assert data[0]["sequences"] == 2 and data[0]["compressed"] == 66 + 2 + 1 + (40000 - 69 - 4 - 15) // 255 + 6, data
    if name.startswith("period-") and name != "period-40000":
        assert data[0]["sequences"] == 2, (name, data)
    if name == "period-40000":
        assert data[0]["uncompressed"] > 65536 and data[0]["sequences"] == 2, data
    if name == "arange":
        assert data[0]["uncompressed"] == 160000 and data[0]["sequences"] == 19972 and data[0]["compressed"] == 80142, data
    if name == "random":
        assert data[0]["sequences"] == 1 and data[0]["compressed"] > data[0]["uncompressed"], data
        assert report["row_groups"][0]["chunks"][0]["oversized_v1_pages"] == 1
    if name == "single":  # a body under 13 bytes
        assert data[0]["uncompressed"] == 8 and data[0]["compressed"] == 9 and data[0]["sequences"] == 1, data
    if name == "far-repeat":
        assert data[0]["sequences"] == 1, data
    if name == "nullable":
        assert data[0]["sequences"] == 984, data
    if name == "bool-mod-3":
        assert data[0]["sequences"] == 2, data
    if name == "utf8-plain":
        assert data[0]["sequences"] == 3002, data
    if name == "utf8-dict-pages-of-1024":  # the dictionary page and the index pages appear as blocks in the dump
        assert [p["type"] for p in pages] == [2, 0, 0, 0, 0] and pages[0]["compressed"] < pages[0]["uncompressed"], pages
        assert [p["sequences"] for p in pages] == [2969, 1, 1, 1, 1], pages  # 1 261 distinct words; the 11-bit index pages do not shrink


def test_a_chunk_that_falls_back_mid_chunk(program, tmp_path):
    schema, batches = Z.fallback_batches()
    path, c, pages, report = write_and_check(program, tmp_path, schema, batches, 4, options={"page_rows": 64}, name="fallback.parquet")
    for k in range(2):
        assert [p["type"] for p in report["row_groups"][0]["chunks"][k]["pages"]] == [2, 0, 0, 0, 0, 0, 0]
        assert set(pq.ParquetFile(path).metadata.row_group(0).column(k).encodings) == {"PLAIN", "RLE", "RLE_DICTIONARY"}
    assert c["parquet_write_dict_pages"] == 2 and c["parquet_write_lz4_pages"] == 14, c


def test_a_dictionary_without_an_entry(program, tmp_path):
    schema, b = D.nulls_batch()
    _, _, _, report = write_and_check(program, tmp_path, schema, [b], 64, options={"page_rows": 64}, name="nulls.parquet")
    first = report["row_groups"][0]["chunks"][1]["pages"][0]
    assert first["type"] == 2 and first["uncompressed"] == 0 and first["compressed"] == 1, first


def test_the_option_at_zero_is_the_file_written_without_it(tmp_path):
    schema = D.eleven_schema(True)
    batches = [D.cardinality_batch(300, 3, True, 90 + i) for i in range(2)]
    small = {"row_group_rows": 250, "page_rows": 128}
    for extra in ({}, {"dictionary": 16}):
        a, z = str(tmp_path / "zero.parquet"), str(tmp_path / "without.parquet")
        c = write(a, schema, batches, None, dict(small, compression=ex.PARQUET_COMPRESSION_UNCOMPRESSED, **extra))
        assert all(c[k] == 0 for k in LZ4), c
        write(z, schema, batches, None, dict(small, **extra))
        assert_same_bytes(a, z, "compression = 0")
        assert pq.ParquetFile(a).metadata.row_group(0).column(1).compression == "UNCOMPRESSED"


def test_write_compressed_read_back_group_by(program, tmp_path):
    """a two-column table written compressed, read back through ParquetDataSource, SUM(v) GROUP BY k over it against the oracle"""
    rng = np.random.default_rng(Z.SEED + 9)
    n = 5000
    schema = pa.schema([pa.field("k", pa.int32(), nullable=False), pa.field("v", pa.int64(), nullable=False)])
    k, v = rng.integers(0, 37, size=n).astype(np.int32), rng.integers(-1000, 1000, size=n)
    b = pa.RecordBatch.from_arrays([pa.array(k), pa.array(v, pa.int64())], schema=schema)
    path, _, _, _ = write_and_check(program, tmp_path, schema, [b], 0, options={"page_rows": 1024}, name="query.parquet")
    ex.counter_reset()
    src = ex.ParquetDataSource(path)
    s = src.schema()
    aggs = [AggregateFunction("SUM", [Column(1)], DataType.Int64)]
    got = ex.AggregateRelation(None, src, [ex.compile_scalar_expr(None, Column(0), s)], [ex.compile_expr(None, a, s) for a in aggs]).next()
    assert ex.counter_get("parquet_inflated_pages") > 0
    assert got.num_rows == len(np.unique(k))
    assert_groups_identical(got, oracle.aggregate([Column(0)], aggs, [b]), 1, "SUM(v) GROUP BY k over the compressed file")
