"""GPU tests of the Parquet source's inflate stage (deviation D12, codec 7 = LZ4_RAW): pages inflated on the device by k_pq_inflate,
then decoded by the kernels of the uncompressed path, against pyarrow's reader -- over the case matrix of tests/parquet_cases.py
written with compression='LZ4' and the shape cases of tests/parquet_lz4_cases.py (files written into tmp_path at test time).  Truth
is pq.read_table; results are compared bit for bit on the concatenation of all batches.  No test feeds the kernel a damaged page:
corrupt blocks are covered on the CPU by the shared sequence parser (tests/test_parquet_lz4_host.py)."""
import os
import subprocess
import sys

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle  # noqa: E402
import parquet_cases as PC  # noqa: E402
import parquet_lz4_cases as LC  # noqa: E402
from gpu_util import assert_groups_identical  # noqa: E402
from test_gpu_parquet import assert_same_table, expected_batch_rows, read_all  # noqa: E402
from test_parquet_host import run  # noqa: E402

from datafusion_archive_amd import execution as ex  # noqa: E402
from datafusion_archive_amd.logicalplan import AggregateFunction, Column, DataType  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["parquet_inflated_pages", "parquet_stored_pages", "parquet_inflated_bytes", "parquet_lz4_sequences", "parquet_inflated_bytes_to_host"]


def new_counters():
    return {k: ex.counter_get(k) for k in NEW}


def check_file(path, what, batch_sizes=(0, 64)):
    """the file through ParquetDataSource against pq.read_table; the new counters of the last read"""
    md = pq.ParquetFile(path).metadata
    if md.num_rows:
        assert md.row_group(0).column(0).compression == "LZ4", what
    truth = pq.read_table(path)
    c = None
    for bs in batch_sizes:
        got, rows, _ = read_all(path, batch_size=bs)
        c = new_counters()
        assert rows == expected_batch_rows(path, bs), (what, bs)
        assert_same_table(got, truth, f"{what} batch_size={bs}")
    return c


# ---- 1. the matrix ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", ["types", "rows", "nulls", "dict", "fallback", "projection"])
def test_matrix(tmp_path, group):
    total = {k: 0 for k in NEW}
    for name, table, options in LC.matrix({group}):
        path = str(tmp_path / f"{name}.parquet")
        PC.write(table, path, options)
        c = check_file(path, name)
        for k in NEW:
            total[k] += c[k]
    assert total["parquet_inflated_pages"] > 0 and total["parquet_lz4_sequences"] > 0 and total["parquet_inflated_bytes"] > 0, total


# ---- 2. the shapes ------------------------------------------------------------------------------------------------------------------
SHAPES = [c[0] for c in LC.shapes()]


@pytest.fixture(scope="module")
def host_decoder(tmp_path_factory):
    """tests/native/parquet_lz4_check.cpp: the sequential decoder the kernel's sequence count is held against"""
    exe = str(tmp_path_factory.mktemp("parquet_lz4_check") / "parquet_lz4_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "native", "parquet_lz4_check.cpp")])
    return exe


@pytest.mark.parametrize("name", SHAPES)
def test_shapes_and_counters(tmp_path, host_decoder, name):
    (_, table, options), = [c for c in LC.shapes() if c[0] == name]
    path = str(tmp_path / f"{name}.parquet")
    PC.write(table, path, options)
    c = check_file(path, name)
    d = run(host_decoder, "dump", path)
    pages = [p for rg in d["row_groups"] for ch in rg["chunks"] for p in ch["inflate"]]
    # the kernel parsed the sequences the host decoder parsed; the image holds the pages' uncompressed sizes less V2's level prefixes
    assert c["parquet_lz4_sequences"] == d["lz4"]["sequences"], (c, d["lz4"])
    assert c["parquet_inflated_bytes"] == sum(p["dst_len"] - p["prefix_len"] for p in pages), (c, pages)
    assert c["parquet_inflated_pages"] == d["lz4"]["inflated_pages"] and c["parquet_stored_pages"] == d["lz4"]["stored_pages"], (c, d["lz4"])
    if table.schema.types[0] == pa.int64() and not table.schema.field(0).nullable and options["data_page_version"] == "1.0":
        assert c["parquet_inflated_bytes"] == 8 * table.num_rows, c  # required PLAIN Int64, V1: the values and nothing else
    if name == "random-v2":
        assert c["parquet_stored_pages"] > 0 and c["parquet_lz4_sequences"] == 0, c
    if table.schema.types[0] == pa.string():  # the length chains are walked on the host: the image comes back
        assert c["parquet_inflated_bytes_to_host"] == sum(ch["image_len"] for rg in d["row_groups"] for ch in rg["chunks"]) > 0, c
    else:  # fixed width and Boolean: the body pass runs from the prologues, the inflated bytes never leave the device
        assert c["parquet_inflated_bytes_to_host"] == 0, c


def test_numeric_file_keeps_its_bytes_on_the_device_and_uncompressed_files_count_nothing(tmp_path):
    rng = np.random.default_rng(PC.SEED + 5)
    table = PC.types_table(1000, True, rng).drop_columns(["s"])
    for version in ("1.0", "2.0"):
        for use_dict in (False, True):
            path = str(tmp_path / f"numeric-{version}-{use_dict}.parquet")
            pq.write_table(table, path, compression="LZ4", use_dictionary=use_dict, data_page_version=version, data_page_size=1024)
            c = check_file(path, path)
            assert c["parquet_inflated_bytes_to_host"] == 0 and c["parquet_inflated_pages"] + c["parquet_stored_pages"] > 0, c
    path = str(tmp_path / "none.parquet")
    pq.write_table(PC.types_table(1000, True, rng), path, compression="NONE", data_page_size=1024)
    got, _, _ = read_all(path)
    assert_same_table(got, pq.read_table(path), "uncompressed")
    assert new_counters() == {k: 0 for k in NEW}


# ---- 3. projection and a real query -------------------------------------------------------------------------------------------------
def test_projection_keeps_unread_chunks_off_the_device(tmp_path):
    (name, table, options), = LC.matrix({"projection"})
    path = str(tmp_path / "projection.parquet")
    PC.write(table, path, options)
    got, _, c = read_all(path, projection=[3, 0])
    assert_same_table(got, pq.read_table(path, columns=["c3", "c0"]))
    md = pq.ParquetFile(path).metadata
    assert c["parquet_chunk_bytes"] == sum(md.row_group(g).column(i).total_compressed_size for g in range(md.num_row_groups) for i in (3, 0))
    assert ex.counter_get("parquet_inflated_bytes_to_host") == 0  # neither Utf8 column was read
    ex.counter_reset()
    src = ex.ParquetDataSource(path)
    schema = src.schema()
    agg = ex.AggregateRelation(None, src, [ex.compile_scalar_expr(None, Column(0), schema)],
                               [ex.compile_expr(None, AggregateFunction("MAX", [Column(1)], DataType.Float64), schema)])
    assert "LZ4_RAW" in ex.explain(agg)
    out = agg.next()
    assert ex.counter_get("parquet_chunk_bytes") == sum(md.row_group(g).column(i).total_compressed_size for g in range(md.num_row_groups) for i in (0, 1))
    want = oracle.aggregate([Column(0)], [AggregateFunction("MAX", [Column(1)], DataType.Float64)], pq.read_table(path).to_batches())
    assert_groups_identical(out, want, 1, "MAX GROUP BY over LZ4 Parquet")


def test_sum_group_by_matches_the_uncompressed_file(tmp_path):
    rng = np.random.default_rng(PC.SEED + 9)
    n = 20000
    t = pa.Table.from_arrays([pa.array(rng.integers(0, 300, size=n), type=pa.int64()), pa.array(rng.integers(-1000, 1000, size=n), type=pa.int64())],
                             schema=pa.schema([pa.field("k", pa.int64(), nullable=False), pa.field("v", pa.int64(), nullable=False)]))
    results = {}
    for codec in ("NONE", "LZ4"):
        path = str(tmp_path / f"grouped-{codec}.parquet")
        pq.write_table(t, path, compression=codec, use_dictionary=["k"], row_group_size=6000, data_page_size=4096)
        ex.counter_reset()
        src = ex.ParquetDataSource(path)
        schema = src.schema()
        aggs = [AggregateFunction("SUM", [Column(1)], DataType.Int64)]
        rel = ex.AggregateRelation(None, src, [ex.compile_scalar_expr(None, Column(0), schema)], [ex.compile_expr(None, a, schema) for a in aggs])
        out = rel.next()
        assert (ex.counter_get("parquet_inflated_pages") > 0) == (codec == "LZ4")
        assert_groups_identical(out, oracle.aggregate([Column(0)], aggs, t.to_batches()), 1, f"SUM(v) GROUP BY k, {codec}")
        results[codec] = sorted(zip(out.column(0).to_pylist(), out.column(1).to_pylist()))
    assert results["LZ4"] == results["NONE"]
