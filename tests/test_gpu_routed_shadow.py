"""The routed shadow of a resident table (csrc/dfx_routed_shadow.hpp; DESIGN.md sections 3-5): pass 1's unfiltered output, kept per
window of the table, and pass 2's scan form (Pass2Rows::narrow8_pred) that reads a window and evaluates the predicate itself.  Windows
are 2^16 rows here (agg.routed_shadow_window_rows), batches two windows wide.

Every case runs with agg.routed_shadow = 0 and with the shadow built, and BOTH results are compared bit for bit with the CPU oracle
over the same generator rows -- never one GPU result with the other.  agg_routed_shadow_launches must grow by exactly the number of
windows the scan covers (the tail window included) when the shadow serves, and must not move otherwise: a silent fallback cannot pass.
Values are multiples of 2^-10 below 2^10 (SYNTH_F64_EXACT): a group's sum is exact in any order."""
import pyarrow as pa
import pytest

import oracle
from datafusion_archive_amd import execution as ex
from datafusion_archive_amd.logicalplan import AggregateFunction, BinaryExpr, Column, DataType, Literal, Operator, ScalarValue
from gpu_util import gpu_aggregate
from test_gpu_scale import _assert_bit_exact

pytestmark = pytest.mark.gpu

F64 = DataType.Float64
W = 1 << 16
BATCH = 2 * W
N = 3 * W + 1000 + 37  # three windows and a tail
SEED = 0xD5AD
FORCED = (("agg.strategy", 3), ("agg.narrow_keys", 1), ("agg.key_shadow", 1), ("agg.value_shadow", 1), ("agg.routed_shadow_window_rows", W))
RESET = (("agg.strategy", 0), ("agg.narrow_keys", -1), ("agg.key_shadow", -1), ("agg.value_shadow", -1), ("agg.routed_row8", -1),
         ("agg.routed_shadow", -1), ("agg.routed_shadow_window_rows", 1 << 27), ("agg.partition_cap_rows", 0), ("agg.capacity_log2", 0))
SCHEMA = pa.schema([("k", pa.int64()), ("v", pa.float64())])
SUM_V = AggregateFunction("SUM", [Column(1)], F64)


def f64(v):
    return Literal(ScalarValue.Float64(float(v)))


def between(lo, hi, lower=Operator.Gt, upper=Operator.Lt):
    return BinaryExpr(BinaryExpr(Column(1), lower, f64(lo)), Operator.And, BinaryExpr(Column(1), upper, f64(hi)))


HEAD = between(204.8, 409.6)


def syn(groups, k_kind=ex.SYNTH_I64_UNIFORM, v_kind=ex.SYNTH_F64_EXACT):
    p = (0.0, 1.0) if (v_kind & 0xFF) == ex.SYNTH_F64_UNIFORM else (0.0, 0.0)
    return [("k", k_kind, 0, float(groups), 0.0), ("v", v_kind, 1) + p]


def windows(n, row_begin=0):
    return -(-n // W) if row_begin % W == 0 else 0


@pytest.fixture(autouse=True)
def _options():
    for k, v in FORCED:
        ex.set_option(k, v)
    yield
    for k, v in RESET:
        ex.set_option(k, v)


def _query(table, pred, option, row_begin=0, n_rows=-1):
    """one query under agg.routed_shadow = option; returns (result, launches that scanned a window, shadows built)"""
    ex.set_option("agg.routed_shadow", option)
    l0, b0 = ex.counter_get("agg_routed_shadow_launches"), ex.counter_get("agg_routed_shadow_builds")
    got = gpu_aggregate([Column(0)], [SUM_V], SCHEMA, [], filter_expr=pred, source=table.scan(BATCH, row_begin, n_rows))
    return got, ex.counter_get("agg_routed_shadow_launches") - l0, ex.counter_get("agg_routed_shadow_builds") - b0


_WANT = {}


def _want(cols, seed, pred_name, pred, row_begin, n):
    key = (repr(cols), seed, pred_name, row_begin, n)
    if key not in _WANT:
        _WANT[key] = oracle.run_synth_query(cols, seed, row_begin, n, 1024, pred, [Column(0)], [SUM_V])[2]
    return _WANT[key]


def _prime(table, cols, seed, n, builds=1):
    """the table's first query (no predicate) builds both column shadows, binds the operand's, and leaves the routed shadow behind"""
    got, launches, built = _query(table, None, -1)
    assert launches == 0 and built == builds, (launches, built)
    _assert_bit_exact(got, _want(cols, seed, "none", None, 0, n), "the query that builds")


def _off_then_on(table, cols, seed, pred_name, pred, n, what, serves=True, row_begin=0, n_rows=-1):
    rows = n if n_rows < 0 else n_rows
    want = _want(cols, seed, pred_name, pred, row_begin, rows)
    got, launches, built = _query(table, pred, 0, row_begin, n_rows)
    assert launches == 0 and built == 0, f"{what}, option 0: {launches} launches, {built} builds"
    _assert_bit_exact(got, want, f"{what}, option 0")
    got, launches, built = _query(table, pred, -1, row_begin, n_rows)
    assert built == 0, f"{what}: a second build"
    assert launches == (windows(rows, row_begin) if serves else 0), f"{what}, option -1: {launches} launches scanned a window"
    _assert_bit_exact(got, want, f"{what}, option -1")
    return got


@pytest.mark.parametrize("groups", [1000, 200000])
def test_three_windows_and_a_tail(groups):
    """200000 groups: the partitioned strategy as the parity tests run it"""
    cols = syn(groups)
    t = ex.DeviceTable.synth(cols, SEED, 0, N)
    _prime(t, cols, SEED, N)
    _off_then_on(t, cols, SEED, "head", HEAD, N, f"headline, {groups} groups")
    _off_then_on(t, cols, SEED, "other", between(100.0, 900.5), N, "a second query with other literals")


@pytest.mark.parametrize("n", [2 * W + 40, W], ids=["tail_below_64", "exactly_one_window"])
def test_table_sizes(n):
    cols = syn(1000)
    t = ex.DeviceTable.synth(cols, SEED + 1, 0, n)
    _prime(t, cols, SEED + 1, n)
    _off_then_on(t, cols, SEED + 1, "head", HEAD, n, f"{n} rows")


PREDS = [("gt_lt", between(204.8, 409.6)), ("ge_lt", between(256.0, 512.0, Operator.GtEq)), ("gt_le", between(256.0, 512.0, Operator.Gt, Operator.LtEq)),
         ("ge_le", between(256.0, 512.0, Operator.GtEq, Operator.LtEq)), ("one_term", BinaryExpr(Column(1), Operator.Gt, f64(204.8))), ("none", None),
         ("nobody", between(2000.0, 3000.0)), ("everybody", between(-1.0, 5000.0))]


def test_predicate_forms():
    """the four range forms, a one-term predicate, no predicate, a predicate nobody passes and one everybody passes"""
    cols = syn(1000)
    t = ex.DeviceTable.synth(cols, SEED + 2, 0, N)
    _prime(t, cols, SEED + 2, N)
    for name, pred in PREDS:
        got = _off_then_on(t, cols, SEED + 2, name, pred, N, name)
        if name == "nobody":
            assert got.num_rows == 0, "a group appeared that has no passing row"
        if name in ("everybody", "none"):
            assert got.num_rows == 1000


def test_default_options_cold_query_two_more_then_the_fourth_scans():
    """agg.key_shadow = agg.value_shadow = agg.routed_shadow = -1: the second query builds the key shadow, the third the operand's --
    and, having bound it, the routed shadow after its last batch --, the fourth is served by it whole"""
    for k in ("agg.key_shadow", "agg.value_shadow"):
        ex.set_option(k, -1)
    cols = syn(1000)
    t = ex.DeviceTable.synth(cols, SEED + 3, 0, N)
    want = _want(cols, SEED + 3, "head", HEAD, 0, N)
    seen = []
    for q in range(4):
        got, launches, built = _query(t, HEAD, -1)
        _assert_bit_exact(got, want, f"query {q + 1}")
        seen.append((launches, built))
    assert seen == [(0, 0), (0, 0), (0, 1), (windows(N), 0)], seen


def test_scan_that_starts_off_the_window_grid():
    cols = syn(1000)
    t = ex.DeviceTable.synth(cols, SEED, 0, N)
    _prime(t, cols, SEED, N)
    _off_then_on(t, cols, SEED, "head", HEAD, N, "off the grid", serves=False, row_begin=64 * 5, n_rows=2 * W)
    _off_then_on(t, cols, SEED, "head", HEAD, N, "on the grid, from the second window", row_begin=W, n_rows=2 * W)


def test_operand_that_is_not_float32_exact():
    cols = syn(1000, v_kind=ex.SYNTH_F64_UNIFORM)
    t = ex.DeviceTable.synth(cols, SEED + 4, 0, N)
    pred = between(0.2, 0.4)
    min_v = AggregateFunction("MIN", [Column(1)], F64)  # (a sum of uniform doubles depends on the order)
    want = oracle.run_synth_query(cols, SEED + 4, 0, N, 1024, pred, [Column(0)], [min_v])[2]
    for q in range(3):
        l0, b0 = ex.counter_get("agg_routed_shadow_launches"), ex.counter_get("agg_routed_shadow_builds")
        gpu_aggregate([Column(0)], [SUM_V], SCHEMA, [], filter_expr=pred, source=t.scan(BATCH))
        got = gpu_aggregate([Column(0)], [min_v], SCHEMA, [], filter_expr=pred, source=t.scan(BATCH))
        assert ex.counter_get("agg_routed_shadow_launches") == l0 and ex.counter_get("agg_routed_shadow_builds") == b0, q
        _assert_bit_exact(got, want, f"MIN of a uniform operand, query {q + 1}")


def test_nullable_operand():
    cols = syn(1000, v_kind=ex.synth_nulls(ex.SYNTH_F64_EXACT, 100))
    t = ex.DeviceTable.synth(cols, SEED + 5, 0, N)
    want = _want(cols, SEED + 5, "head", HEAD, 0, N)
    for q in range(3):
        got, launches, built = _query(t, HEAD, -1)
        assert launches == 0 and built == 0, (q, launches, built)
        _assert_bit_exact(got, want, f"nullable operand, query {q + 1}")


def test_zipf_keys_overflow_the_regions_and_refuse_the_shadow():
    """regions of one quantum: the build's dense pass 1 spills, the pair is refused for good and keeps the two passes"""
    cols = syn(200000, k_kind=ex.SYNTH_I64_ZIPF)
    t = ex.DeviceTable.synth(cols, SEED + 6, 0, N)
    ex.set_option("agg.partition_cap_rows", 64)
    want = _want(cols, SEED + 6, "head", HEAD, 0, N)
    us0 = ex.counter_get("agg_routed_shadow_build_us")
    for q in range(3):
        got, launches, built = _query(t, HEAD, -1)
        assert launches == 0 and built == 0, (q, launches, built)
        _assert_bit_exact(got, want, f"zipf keys, query {q + 1}")
        if q == 0:
            us1 = ex.counter_get("agg_routed_shadow_build_us")
            assert us1 > us0, "the first query tried"
    ex.set_option("agg.partition_cap_rows", 0)
    got, launches, built = _query(t, HEAD, -1)  # (room now, but the refusal is for good)
    assert launches == 0 and built == 0
    _assert_bit_exact(got, want, "zipf keys, after the refusal")


def test_table_that_grows_mid_query_keeps_the_two_passes_until_the_geometry_matches():
    """2^14 slots to begin with, 200000 groups: every query starts with another block count than the shadow was routed for"""
    cols = syn(200000)
    t = ex.DeviceTable.synth(cols, SEED + 7, 0, N)
    ex.set_option("agg.capacity_log2", 14)
    want = _want(cols, SEED + 7, "head", HEAD, 0, N)
    got, launches, built = _query(t, HEAD, -1)
    assert launches == 0 and built <= 1
    _assert_bit_exact(got, want, "growing table, the query that builds")
    for q in range(2):
        got, launches, built = _query(t, HEAD, -1)
        assert launches < windows(N) and built == 0, (q, launches, built)  # (the first window meets the small table)
        _assert_bit_exact(got, want, f"growing table, query {q + 2}")
    got, launches, built = _query(t, HEAD, 0)
    assert launches == 0
    _assert_bit_exact(got, want, "growing table, option 0")


def test_two_tables_alive_at_once():
    cols_a, cols_b = syn(1000), syn(5000)
    n_b = 2 * W
    ta = ex.DeviceTable.synth(cols_a, SEED + 8, 0, N)
    tb = ex.DeviceTable.synth(cols_b, SEED + 9, 0, n_b)
    _prime(ta, cols_a, SEED + 8, N)
    _prime(tb, cols_b, SEED + 9, n_b)
    for _ in range(2):
        _off_then_on(ta, cols_a, SEED + 8, "head", HEAD, N, "table a")
        _off_then_on(tb, cols_b, SEED + 9, "head", HEAD, n_b, "table b")
