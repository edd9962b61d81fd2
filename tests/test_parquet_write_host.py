"""CPU tests of the Parquet writer (deviation D13): the two HIP-free headers (csrc/dfx_parquet_thrift_write.hpp, csrc/dfx_parquet_enc.hpp)
through tests/native/parquet_write_check.cpp, a stand-alone program built once plain and once under the host sanitizers, which writes
whole files with the sequential host encoder.  Every file is held three ways: pyarrow reads back the table that went in (names, types,
field nullability, nulls, values by bit pattern) and the metadata the format fixes; the library's own reader headers, called from the
same program, parse the footer, walk every page and decode the values that went in; the page geometry and the level-run kinds, read
from the level bytes, are the ones the rules give.  dfx_parquet_write itself needs a GPU: what it refuses without one is at the end."""
import json
import os
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import parquet_write_cases as W

from datafusion_archive_amd import _ffi
from datafusion_archive_amd import execution as ex


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("parquet_write_check")
    return {"plain": W.build_program(d, False), "sanitized": W.build_program(d, True)}


def write_and_check(programs, tmp_path, name, schema, batches, row_group_rows=W.DEFAULT_ROW_GROUP_ROWS, page_rows=W.DEFAULT_PAGE_ROWS, which="sanitized"):
    path = str(tmp_path / f"{name}.parquet")
    report = W.host_write(programs[which], W.describe(schema, batches, row_group_rows, page_rows), path, tmp_path)
    assert report["code"] == 0 and report["reader_code"] == 0 and report["mismatch"] == "", (name, {k: report[k] for k in report if k != "row_groups"})
    assert report["bytes"] == os.path.getsize(path)
    W.check_file(path, schema, batches, row_group_rows, page_rows, what=name)
    # the reader's headers saw the schema and the geometry the rules give
    assert [(c["name"], c["dtype"], c["optional"]) for c in report["columns"]] == [(f.name, W.DTYPES[f.type], f.nullable) for f in schema], name
    assert [c["physical"] for c in report["columns"]] == [W.PHYSICAL[W.DTYPES[f.type]] for f in schema], name
    pages = W.expected_pages([b.num_rows for b in batches], row_group_rows, page_rows)
    assert [g["num_rows"] for g in report["row_groups"]] == [sum(g) for g in pages], name
    for g, group in zip(report["row_groups"], pages):
        for ch in g["chunks"]:
            assert [p["num_values"] for p in ch["pages"]] == group, name
    want = pa.Table.from_batches(batches, schema=schema)
    for c, f in enumerate(schema):
        runs = [[p["run"] for p in g["chunks"][c]["pages"]] for g in report["row_groups"]]
        if f.nullable:
            assert runs == W.expected_runs(np.asarray(want.column(c).combine_chunks().is_valid()).astype(bool), pages), (name, f.name)
        else:
            assert all(r == "none" for g in runs for r in g), (name, f.name)
    return path, report


@pytest.mark.parametrize("nullable", [True, False])
@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 63, 64, 65, 1000])
def test_all_types_at_the_row_count_edges(programs, tmp_path, n, nullable):
    b = W.all_types_batch(n, nullable, n)
    schema = W.all_types_schema(nullable)
    write_and_check(programs, tmp_path, "default", schema, [b])
    write_and_check(programs, tmp_path, "small", schema, [b], row_group_rows=250, page_rows=128, which="plain")
    if n == 0:
        assert pq.ParquetFile(str(tmp_path / "default.parquet")).metadata.num_row_groups == 0  # the schema and no row group


@pytest.mark.parametrize("page_rows", [64, 128])
@pytest.mark.parametrize("row_group_rows", [100, 250])
def test_pieces_that_straddle_and_short_pages_inside_a_chunk(programs, tmp_path, row_group_rows, page_rows):
    batches = [W.all_types_batch(300, True, 100 + i) for i in range(3)]
    _, report = write_and_check(programs, tmp_path, "geometry", W.all_types_schema(True), batches, row_group_rows, page_rows)
    pages = W.expected_pages([300] * 3, row_group_rows, page_rows)
    assert len(pages) == -(-900 // row_group_rows)
    if row_group_rows == 250:  # 300-row batches straddle the groups: a piece ends, and with it a page, in the middle of a chunk
        assert any(p < page_rows for g in pages for p in g[:-1])


@pytest.mark.parametrize("offset", [0, 3, 67])
def test_source_bit_offsets(programs, tmp_path, offset):
    """slices: every buffer and bitmap of the source starts `offset` rows / bits in"""
    whole = W.all_types_batch(500, True, 200)
    b = whole.slice(offset, 300)
    assert b.column(0).offset == offset
    write_and_check(programs, tmp_path, "offset", W.all_types_schema(True), [b], row_group_rows=250, page_rows=64)
    req = W.all_types_batch(500, False, 201).slice(offset)
    write_and_check(programs, tmp_path, "offset-required", W.all_types_schema(False), [req], page_rows=128, which="plain")


def test_the_three_run_kinds_in_one_chunk(programs, tmp_path):
    schema, b, valid = W.run_kinds_batch()
    path, report = write_and_check(programs, tmp_path, "runs", schema, [b], page_rows=64)
    for ch in report["row_groups"][0]["chunks"]:
        assert [p["run"] for p in ch["pages"]] == ["rle0", "rle1", "packed"]
        # an RLE run of 64: header 64 << 1 = 0x80 0x01 and the value byte; the bit-packed run: header 8 << 1 | 1 and 8 bytes
        assert [p["lev_len"] for p in ch["pages"]] == [3, 3, 9]
    ch = report["row_groups"][0]["chunks"][0]
    assert [p["val_len"] for p in ch["pages"]] == [0, 64 * 8, 8 * int(valid[128:].sum())]


@pytest.mark.parametrize("page_rows", [64, 128])
def test_boolean_with_nulls(programs, tmp_path, page_rows):
    schema, b = W.boolean_batch(1000)
    _, report = write_and_check(programs, tmp_path, "boolean", schema, [b], page_rows=page_rows)
    valid = np.asarray(b.column(0).is_valid())
    got = [p["val_len"] for p in report["row_groups"][0]["chunks"][0]["pages"]]
    assert got == [(int(valid[r:r + page_rows].sum()) + 7) // 8 for r in range(0, 1000, page_rows)]
    assert any(int(valid[r:r + 64].sum()) % 32 for r in range(0, 1000, 64)), "tiles must end inside words"


def test_utf8_values(programs, tmp_path):
    schema, b = W.utf8_batch()
    write_and_check(programs, tmp_path, "utf8", schema, [b], page_rows=64)
    write_and_check(programs, tmp_path, "utf8-one-page", schema, [b], which="plain")


def test_required_column_with_nulls_is_refused(programs, tmp_path):
    schema = pa.schema([pa.field("v", pa.int32(), nullable=False)])
    b = pa.RecordBatch.from_arrays([pa.array([1, None, 3], pa.int32())], schema=schema)
    path = str(tmp_path / "required.parquet")
    report = W.host_write(programs["sanitized"], W.describe(schema, [b]), path, tmp_path)
    assert report["code"] == 8 and "'v'" in report["error"] and not os.path.exists(path), report  # DFX_EXECUTION_ERROR


def test_the_i32_size_rule_on_made_up_sizes(programs):
    top = 2 ** 31 - 1
    cases = [(0, 0), (0, top - 1), (0, top), (10, top - 11), (10, top - 10), (4, 2 ** 32), (top - 1, 0), (top, 0), (2 ** 63, 2 ** 63), (2 ** 64 - 1, 1)]
    r = subprocess.run([programs["sanitized"], "fits"] + [str(v) for pair in cases for v in pair], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout) == [1, 1, 0, 1, 0, 0, 1, 0, 0, 0]  # a body of 2^31 - 1 bytes or more is refused; sums that wrap are too


def test_damaged_files_are_reported_not_read_out_of_bounds(programs, tmp_path):
    """what the writer wrote, cut at every length and with every footer byte changed, under the sanitizers: an error or a parse"""
    schema, b = W.boolean_batch(100)
    path, _ = write_and_check(programs, tmp_path, "damage", schema, [b], page_rows=64)
    r = subprocess.run([programs["sanitized"], "damage", path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads(r.stdout)
    assert d["truncations"] == os.path.getsize(path) and d["flips"] > 100 and d["errors"] > 0


# ---- the library without a device -------------------------------------------------------------------------------------------------
def _one_batch():
    schema = pa.schema([pa.field("v", pa.int32()), pa.field("s", pa.string())])
    return schema, pa.RecordBatch.from_arrays([pa.array([1, None, 3], pa.int32()), pa.array(["a", "", None])], schema=schema)


def _nothing_left(target):
    assert not os.path.exists(str(target)) and not os.path.exists(str(target) + ".dfx-partial")


def test_the_symbol_is_declared_and_exported():
    assert "dfx_parquet_write" in _ffi.EXPORTED_SYMBOLS and hasattr(_ffi.lib(), "dfx_parquet_write")
    assert callable(ex.write_parquet)


@pytest.mark.parametrize("options", [{"compression": 1}, {"page_rows": 100}, {"page_rows": 0}, {"page_rows": 32}, {"row_group_rows": 0},
                                     {"row_group_rows": -5}])
def test_option_errors_need_no_device(tmp_path, options):
    schema, b = _one_batch()
    target = tmp_path / "o.parquet"
    with pytest.raises(ex.ExecutionError) as ei:
        ex.write_parquet(ex.DataSourceRelation(schema, [b]), str(target), options)
    assert ei.value.kind == "General" and list(options)[0] in str(ei.value), ei.value
    _nothing_left(target)


def test_an_unsupported_column_type_needs_no_device(tmp_path):
    schema = pa.schema([pa.field("v", pa.int32()), pa.field("when", pa.date32())])
    b = pa.RecordBatch.from_arrays([pa.array([1], pa.int32()), pa.array([3], pa.date32())], schema=schema)
    target = tmp_path / "o.parquet"
    with pytest.raises(ex.ExecutionError) as ei:
        ex.write_parquet(ex.DataSourceRelation(schema, [b]), str(target))
    assert ei.value.kind == "NotImplemented" and "when" in str(ei.value) and "tdD" in str(ei.value), ei.value
    _nothing_left(target)


def test_a_valid_call_without_a_device_fails_loudly(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_parquet_write.py writes files")
    schema, b = _one_batch()
    target = tmp_path / "o.parquet"
    with pytest.raises(ex.ExecutionError) as ei:
        ex.write_parquet(ex.DataSourceRelation(schema, [b]), str(target), {"page_rows": 64, "row_group_rows": 2})
    assert ei.value.kind == "ExecutionError" and "no HIP device available" in str(ei.value), ei.value
    _nothing_left(target)
