"""CPU tests of the Parquet writer's "dictionary" option: csrc/dfx_parquet_dict_enc.hpp (the rules and the sequential encoder of a
dictionary chunk) with the additions to csrc/dfx_parquet_thrift_write.hpp and csrc/dfx_parquet_enc.hpp, through
tests/native/parquet_dict_write_check.cpp, a stand-alone program built once plain and once under the host sanitizers, which writes
whole files.  Every file is held against pyarrow (the table that went in by bit patterns, the chunk metadata, every chunk's dictionary
against pyarrow.compute.unique: first-occurrence order) and against the library's own reader headers, called from the same program,
which parse every header and decode every index page.  The rules are also asked on made-up numbers.  dfx_parquet_write itself needs a
GPU: what it refuses without one is at the end."""
import json
import os
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import parquet_dict_write_cases as D
import parquet_write_cases as W

from datafusion_archive_amd import execution as ex


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("parquet_dict_write_check")
    return {"plain": D.build_program(d, False), "sanitized": D.build_program(d, True)}


def write_and_check(programs, tmp_path, name, schema, batches, limit, row_group_rows=W.DEFAULT_ROW_GROUP_ROWS, page_rows=W.DEFAULT_PAGE_ROWS, which="sanitized"):
    path = str(tmp_path / f"{name}.parquet")
    report = D.host_write(programs[which], W.describe(schema, batches, row_group_rows, page_rows), path, tmp_path, limit)
    assert report["code"] == 0 and report["reader_code"] == 0 and report["mismatch"] == "", (name, {k: report[k] for k in report if k != "row_groups"})
    assert report["bytes"] == os.path.getsize(path)
    return path, report, D.check_file(path, schema, batches, limit, row_group_rows, page_rows, what=name, report=report)


# ---- the rules on made-up numbers ----------------------------------------------------------------------------------------------------
def test_index_widths(programs):
    entries = [0, 1, 2, 3, 4, 5, 256, 257, 2 ** 20]
    assert D.rules(programs["sanitized"], "width", entries) == [1, 1, 1, 2, 2, 3, 8, 9, 20] == [D.index_width(e) for e in entries]


def test_run_kinds_and_bytes(programs):
    cases = [(w, nn, eq) for w in (1, 2, 8, 9, 20) for nn in (0, 1, 7, 8, 9) for eq in (0, 1)]
    got = D.rules(programs["sanitized"], "run", [v for c in cases for v in c])
    for (w, nn, eq), (run, header, nbytes, block) in zip(cases, got):
        # one value is one RLE run whatever `eq` says of it: a page of one index has all its indices equal
        kind = 0 if nn == 0 else 1 if eq else 2
        assert run == kind and nbytes == D.run_bytes(w, nn, bool(eq)) and block == 1 + nbytes, (w, nn, eq)
        assert header == (0 if nn == 0 else nn << 1 if eq else ((nn + 7) // 8) << 1 | 1), (w, nn, eq)
    # spelled out: nothing; varint(7 << 1) + one byte; varint(1 << 1 | 1) + one group of 9 bits each; two groups
    assert D.run_bytes(9, 0, False) == 0 and D.run_bytes(9, 7, True) == 1 + 2 and D.run_bytes(9, 8, False) == 1 + 9 and D.run_bytes(9, 9, False) == 1 + 18


def test_the_decision_and_the_i32_rule_on_the_body(programs):
    top = 2 ** 31 - 2  # the largest body a page header can describe and the writer accepts
    cases = [(3, 1, 0, 4, 4), (3, 2, 0, 4, 4), (0, 4, 0, 0, 4), (0, 5, 0, 0, 4), (4, 0, 16, 0, 4), (0, 1, top - 8, 8, 4), (0, 1, top - 8, 9, 4),
             (0, 1, 2 ** 64 - 1, 8, 4), (2 ** 20 - 1, 1, 0, 8, 2 ** 20), (2 ** 20, 1, 0, 8, 2 ** 20)]
    assert D.rules(programs["sanitized"], "stays", [v for c in cases for v in c]) == [1, 0, 1, 0, 1, 1, 0, 0, 1, 0]


# ---- whole files ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nullable", [True, False])
@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 63, 64, 65, 1000])
def test_all_types_at_the_row_count_edges(programs, tmp_path, n, nullable):
    b = D.cardinality_batch(n, 5, nullable, n)
    schema = D.eleven_schema(nullable)
    write_and_check(programs, tmp_path, "default", schema, [b], D.MAX_DICTIONARY)
    _, _, chunks = write_and_check(programs, tmp_path, "small", schema, [b], 16, row_group_rows=250, page_rows=128, which="plain")
    if n > 0:
        assert chunks[(0, 0)][0] is None and all(chunks[(0, c)][0] is not None for c in range(1, 12))  # the Boolean column stays PLAIN


@pytest.mark.parametrize("distinct", [1, 2, 3, 4, 256, 257, 900])
def test_cardinalities_over_pieces_and_groups(programs, tmp_path, distinct):
    """batches of 300 rows into groups of 250 (700 where a group has to hold 256 entries and more): dictionaries grow over launches
    and start empty at every group.  The wide cases are REQUIRED columns: every value occurs in the first batch, so 256 entries give
    width 8 and 257 give width 9 whatever the seed."""
    nullable = distinct < 256
    batches = [D.cardinality_batch(300, distinct, nullable, 40 + i) for i in range(3)]
    _, report, chunks = write_and_check(programs, tmp_path, "card", D.eleven_schema(nullable), batches, D.MAX_DICTIONARY, row_group_rows=250 if distinct < 256 else 700,
                                        page_rows=64)
    widths = {p["width"] for g in report["row_groups"] for p in g["chunks"][3]["pages"]}  # Int32
    if distinct == 1:
        assert all(p["run"] in ("rle", "none") for g in report["row_groups"] for p in g["chunks"][3]["pages"])
    if distinct in (256, 257):
        assert max(widths) == (8 if distinct == 256 else 9), widths  # at 9 bits indices straddle bytes and words
    if distinct in (3, 4):
        assert 2 in widths, widths


def test_every_row_distinct_and_special_values(programs, tmp_path):
    b = W.all_types_batch(1000, True, 77)  # NaN payloads, -0.0 and +0.0, the integer extremes; UInt64 above 2^63
    _, _, chunks = write_and_check(programs, tmp_path, "distinct", W.all_types_schema(True), [b], D.MAX_DICTIONARY, page_rows=128)
    f64 = chunks[(0, 10)][0]
    assert {0x7FF8000000000001, 0xFFF8000000000000, 0x0, 0x8000000000000000} <= set(f64)
    assert any(k >= 2 ** 63 for k in chunks[(0, 8)][0])
    schema, edge = D.edge_batch()
    _, _, chunks = write_and_check(programs, tmp_path, "all-ones", schema, [edge], 4)
    assert chunks[(0, 0)][0] == [2 ** 64 - 1, 0, 2 ** 63] and chunks[(0, 1)][0] == [2 ** 64 - 1, 0, 2 ** 63]


def test_nulls(programs, tmp_path):
    schema, b = D.nulls_batch()
    path, report, chunks = write_and_check(programs, tmp_path, "nulls", schema, [b], 64, page_rows=64)
    assert [p[0] for p in chunks[(0, 0)][1]] == ["packed", "none", "packed"]
    assert chunks[(0, 1)][0] == [] and [p[0] for p in chunks[(0, 1)][1]] == ["none"] * 3  # a zero-entry dictionary page, width bytes and no run
    assert report["row_groups"][0]["chunks"][1]["dict_len"] == 0 and [p["val_len"] for p in report["row_groups"][0]["chunks"][1]["pages"]] == [0, 0, 0]
    assert chunks[(0, 2)][0] == [f"w{i}".encode() for i in (1, 2, 3, 4, 0)] and b"hidden" not in open(path, "rb").read()


def test_utf8_values(programs, tmp_path):
    schema, b = W.utf8_batch()  # the empty string, multi-byte characters, a 20 kB value
    write_and_check(programs, tmp_path, "utf8", schema, [b], D.MAX_DICTIONARY, page_rows=64)
    schema, b = D.same16_batch()
    _, _, chunks = write_and_check(programs, tmp_path, "same16", schema, [b], 4, page_rows=64)
    assert chunks[(0, 0)][0] == [t.encode() for t in D.SAME16]


def test_the_decision_by_launch(programs, tmp_path):
    """N = 4: three values, then three new ones (the chunk falls back and stays PLAIN), then only old ones"""
    schema, mk = D.DECISION_SCHEMA, D.decision_batch
    batches = [mk([1, 2, 3] * 30), mk([4, 5, 6] * 30), mk([1, 2, 3] * 30)]
    path, report, chunks = write_and_check(programs, tmp_path, "fallback", schema, batches, 4, page_rows=64)
    for c in range(2):
        entries, pages = chunks[(0, c)]
        assert len(entries) == 3 and [p[0] for p in pages] == ["packed", "packed", "plain", "plain", "plain", "plain"]
    # exactly four entries stay
    _, _, chunks = write_and_check(programs, tmp_path, "four", schema, [mk([1, 2, 3] * 30), mk([4] * 90)], 4, page_rows=64)
    assert len(chunks[(0, 0)][0]) == 4 and [p[0] for p in chunks[(0, 0)][1]] == ["packed", "packed", "rle", "rle"]
    # five values in the first launch: byte for byte the file written without the option
    five = [mk([1, 2, 3, 4, 5] * 20), mk([1] * 10)]
    a, _, chunks = write_and_check(programs, tmp_path, "five", schema, five, 4, page_rows=64)
    assert chunks[(0, 0)][0] is None
    z, _, _ = write_and_check(programs, tmp_path, "five-off", schema, five, 0, page_rows=64)
    plain = W.build_program(tmp_path, False)
    W.host_write(plain, W.describe(schema, five, page_rows=64), str(tmp_path / "five-plain.parquet"), tmp_path)
    assert open(a, "rb").read() == open(z, "rb").read() == open(str(tmp_path / "five-plain.parquet"), "rb").read()


def test_damaged_files_are_reported_not_read_out_of_bounds(programs, tmp_path):
    """a written file, cut at every length and with every byte of its dictionary page header changed, under the sanitizers"""
    schema = pa.schema([pa.field("s", pa.string()), pa.field("v", pa.int64())])
    b = pa.RecordBatch.from_arrays([pa.array(["a", None, "bcd", "a"] * 25), pa.array([7, 8, None, 7] * 25, pa.int64())], schema=schema)
    path, _, _ = write_and_check(programs, tmp_path, "damage", schema, [b], 16, page_rows=64)
    r = subprocess.run([programs["sanitized"], "damage", path], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads(r.stdout)
    assert d["truncations"] == os.path.getsize(path) and d["flips"] >= 2 * d["header_len"], d
    # a 0x00 is thrift's STOP where a field begins and another number inside one: but for the header's own two STOP bytes it ends the
    # header before its sizes or its value count, or changes one of them, and the reader must refuse each (the 0x7f / 0xff changes come on top)
    assert d["errors"] >= d["header_len"] - 2, d


# ---- the library without a device ------------------------------------------------------------------------------------------------------
def _one_batch():
    schema = pa.schema([pa.field("v", pa.int32()), pa.field("s", pa.string())])
    return schema, pa.RecordBatch.from_arrays([pa.array([1, None, 3], pa.int32()), pa.array(["a", "", None])], schema=schema)


def _nothing_left(target):
    assert not os.path.exists(str(target)) and not os.path.exists(str(target) + ".dfx-partial")


@pytest.mark.parametrize("options", [{"dictionary": -1}, {"dictionary": 2 ** 20 + 1}, {"dictionary": 8, "dictionary_hash_bits": 0},
                                     {"dictionary": 8, "dictionary_hash_bits": 65}, {"page_rows": 2 ** 21, "dictionary": 8}])
def test_option_errors_need_no_device(tmp_path, options):
    schema, b = _one_batch()
    target = tmp_path / "o.parquet"
    with pytest.raises(ex.ExecutionError) as ei:
        ex.write_parquet(ex.DataSourceRelation(schema, [b]), str(target), options)
    assert ei.value.kind == "General" and list(options)[-1] + " = " in str(ei.value), ei.value
    _nothing_left(target)


def test_a_valid_call_without_a_device_fails_loudly(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_parquet_dict_write.py writes files")
    schema, b = _one_batch()
    target = tmp_path / "o.parquet"
    with pytest.raises(ex.ExecutionError) as ei:
        ex.write_parquet(ex.DataSourceRelation(schema, [b]), str(target), {"dictionary": 2 ** 20, "dictionary_hash_bits": 64, "page_rows": 64})
    assert ei.value.kind == "ExecutionError" and "no HIP device available" in str(ei.value), ei.value
    _nothing_left(target)
