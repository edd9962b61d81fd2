"""A resident table concatenated from several host batches (dfx_table_from_stream -> BatchGather, csrc/dfx_gather.cpp) against
pyarrow's concatenation of the same batches: empty batches in front and inside, Arrow slice offsets, a 3-bit bitmap tail, every
column kind once with nulls and once without, Utf8 columns of 0 bytes in all and of mixed lengths.  Then ORDER BY over slices of
such a table that carry a validity bitmap but no null (the sort drops the bitmap, the table keeps it: each operator's own rule)."""
import numpy as np
import pyarrow as pa
import pytest

import oracle
from datafusion_archive_amd import execution as ex
from datafusion_archive_amd.logicalplan import Column
from gpu_util import assert_batches_identical

pytestmark = pytest.mark.gpu

ROWS = (0, 65, 1, 0, 130, 63)    # 259 rows: 4 bitmap words and 3 bits
OFFSETS = (0, 3, 0, 0, 69, 0)    # Arrow offsets of the batches (two are slices)
STRINGS = ("", "x", "0123456789abcdefghijklmnopqrstuvwxyz+-*/")  # 0, 1 and 40 bytes
SCHEMA = pa.schema([pa.field("i64n", pa.int64()), pa.field("i64", pa.int64(), False), pa.field("i32n", pa.int32()),
                    pa.field("i32", pa.int32(), False), pa.field("f64n", pa.float64()), pa.field("f64", pa.float64(), False),
                    pa.field("bn", pa.bool_()), pa.field("b", pa.bool_(), False), pa.field("sn", pa.string()),
                    pa.field("s", pa.string(), False), pa.field("se", pa.string(), False)])


def _batch(rng, n, offset, null_rows):
    """n rows behind `offset` rows that are sliced away; null_rows(m): the mask of a nullable column of m rows"""
    m = n + offset
    f = rng.standard_normal(m)
    f[rng.random(m) < 0.1] = -0.0
    strs = [STRINGS[i] for i in rng.integers(0, 3, m)]
    cols = [pa.array(rng.integers(-2**62, 2**62, m), pa.int64(), mask=null_rows(m)), pa.array(rng.integers(-2**62, 2**62, m), pa.int64()),
            pa.array(rng.integers(-2**31, 2**31, m), pa.int32(), mask=null_rows(m)), pa.array(rng.integers(0, 5, m), pa.int32()),
            pa.array(f, pa.float64(), mask=null_rows(m)), pa.array(rng.standard_normal(m), pa.float64()),
            pa.array(rng.random(m) < 0.5, pa.bool_(), mask=null_rows(m)), pa.array(rng.random(m) < 0.5, pa.bool_()),
            pa.array(strs, pa.string(), mask=null_rows(m)), pa.array([STRINGS[i] for i in rng.integers(0, 3, m)], pa.string()),
            pa.array([""] * m, pa.string())]
    return pa.RecordBatch.from_arrays(cols, schema=SCHEMA).slice(offset, n)


def _batches(seed, null_rows):
    rng = np.random.default_rng(seed)
    return [_batch(rng, n, o, null_rows) for n, o in zip(ROWS, OFFSETS)]


def _assert_same(got, want, what):
    assert got.num_rows == want.num_rows, what
    for c, name in enumerate(SCHEMA.names):
        g, w = got.column(c).combine_chunks(), want.column(c).combine_chunks()
        assert g.null_count == w.null_count, (what, name)
        if pa.types.is_floating(w.type):
            assert [None if x is None else repr(x) for x in g.to_pylist()] == [None if x is None else repr(x) for x in w.to_pylist()], (what, name)
        else:
            assert g.to_pylist() == w.to_pylist(), (what, name)


def _scan(table, *args):
    return pa.Table.from_batches(list(table.scan(*args))).combine_chunks()


def test_table_of_six_batches_equals_their_concatenation():
    batches = _batches(7, lambda m: np.random.default_rng(m).random(m) < 0.25)
    want = pa.Table.from_batches(batches, schema=SCHEMA).combine_chunks()
    assert want.num_rows == 259 and want.column("i64n").null_count > 0 and want.column("sn").null_count > 0
    table = ex.DeviceTable.from_batches(SCHEMA, batches)
    assert table.num_rows() == 259
    _assert_same(_scan(table, 0), want, "scan(0)")
    _assert_same(_scan(table, 64), want, "scan(64)")
    _assert_same(_scan(table, 64, 64, 130), want.slice(64, 130), "scan(64, 64, 130)")


def test_one_batch_at_an_arrow_offset_is_copied_not_adopted():
    batches = _batches(8, lambda m: np.random.default_rng(m + 1).random(m) < 0.25)[1:2]  # 65 rows at offset 3
    want = pa.Table.from_batches(batches, schema=SCHEMA).combine_chunks()
    table = ex.DeviceTable.from_batches(SCHEMA, batches)
    assert table.num_rows() == 65
    _assert_same(_scan(table, 0), want, "scan(0)")


@pytest.mark.parametrize("limit", [None, 7])
def test_order_by_over_slices_with_a_bitmap_and_no_null(limit):
    """rows [64, 259) of a table whose nulls all lie in rows [0, 64): the slices carry a validity pointer and null_count -1"""
    def first_64(m):  # only the 65-row batch (68 rows before its slice; table rows 0 .. 64) has nulls: every other row up to 62
        mask = np.zeros(m, dtype=bool)
        if m == 68:
            mask[3:3 + 64:2] = True
        return mask
    batches = _batches(9, first_64)
    whole = pa.Table.from_batches(batches, schema=SCHEMA).combine_chunks()
    assert whole.column("i64n").null_count == 32 and whole.column("sn").null_count == 32
    rows = whole.slice(64, 195)
    assert rows.column("i64n").null_count == 0 and rows.column("sn").null_count == 0
    keys = [(Column(SCHEMA.get_field_index("i32")), True)]  # five distinct values: the sort's stability shows
    want = oracle.sort_batches(rows.to_batches(), keys)
    if limit is not None:
        want = want.slice(0, limit)
    table = ex.DeviceTable.from_batches(SCHEMA, batches)
    rel = ex.SortRelation(table.scan(64, 64, 195), [(ex.compile_scalar_expr(None, e, SCHEMA), asc) for e, asc in keys], SCHEMA)
    if limit is not None:
        rel = ex.LimitRelation(rel, limit, SCHEMA)
    got = list(rel)
    assert len(got) == 1
    assert_batches_identical(got[0], want, f"ORDER BY i32 LIMIT {limit}")
    assert got[0].column(0).null_count == 0 and got[0].column(8).null_count == 0
