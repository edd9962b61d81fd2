"""8-byte routed rows (PTF_ROW8; DESIGN.md sections 3-5): when every pass-1 launch of a window binds both column shadows, the
one-value wave-specialised layout routes {hash image, Float32 bits of the operand} -- sixteen rows per 128-byte line -- and pass 2
widens the bits in front of the atomic.  The accumulator receives the bits it received from the 12-byte row, so no bit of any
result may change: every case is compared bit for bit with the CPU oracle over the same generator rows (or the same host batches),
once with agg.routed_row8 = 0 (the counter agg_row8_launches must not move) and once with -1 (it must).

Shapes and set-up as in test_gpu_value_shadow.py: 2^20 + 37 rows in batches of 2^18 + 64, the partitioned strategy with narrow rows
forced, both shadows built by a table's first query (which therefore keeps its 12-byte rows to its end)."""
import numpy as np
import pyarrow as pa
import pytest

import oracle
from datafusion_archive_amd import execution as ex
from datafusion_archive_amd.logicalplan import AggregateFunction, BinaryExpr, Column, DataType, Literal, Operator, ScalarValue
from gpu_util import assert_groups_identical, gpu_aggregate
from test_gpu_scale import _assert_bit_exact

pytestmark = pytest.mark.gpu

F64, U64 = DataType.Float64, DataType.UInt64
N = (1 << 20) + 37
BATCH = (1 << 18) + 64
SEED = 0xDF0C
FORCED = (("agg.strategy", 3), ("agg.narrow_keys", 1), ("agg.key_shadow", 1), ("agg.value_shadow", 1))
RESET = (("agg.strategy", 0), ("agg.narrow_keys", -1), ("agg.key_shadow", -1), ("agg.value_shadow", -1), ("agg.routed_row8", -1),
         ("agg.pass1_ws", 8), ("agg.partition_defer_batches", 8), ("agg.partition_cap_rows", 0))


def f64(v):
    return Literal(ScalarValue.Float64(float(v)))


def between(col, lo, hi, lower=Operator.Gt, upper=Operator.Lt):
    return BinaryExpr(BinaryExpr(Column(col), lower, f64(lo)), Operator.And, BinaryExpr(Column(col), upper, f64(hi)))


HEAD = between(1, 204.8, 409.6)
SUM_V = AggregateFunction("SUM", [Column(1)], F64)
MIN_V = AggregateFunction("MIN", [Column(1)], F64)
COUNT_V = AggregateFunction("COUNT", [Column(1)], U64)
SCHEMA = pa.schema([("k", pa.int64()), ("v", pa.float64())])


def syn(groups, v_kind=ex.SYNTH_F64_EXACT):
    p = (0.0, 1.0) if (v_kind & 0xFF) == ex.SYNTH_F64_UNIFORM else (0.0, 0.0)
    return [("k", ex.SYNTH_I64_UNIFORM, 0, float(groups), 0.0), ("v", v_kind, 1) + p]


@pytest.fixture(autouse=True)
def _options():
    for k, v in FORCED:
        ex.set_option(k, v)
    yield
    for k, v in RESET:
        ex.set_option(k, v)


def _query(table, pred, aggs, option, batch=BATCH, row_begin=0, n_rows=-1):
    """one query under agg.routed_row8 = option; returns (result, launches that routed 8-byte rows)"""
    ex.set_option("agg.routed_row8", option)
    r0 = ex.counter_get("agg_row8_launches")
    got = gpu_aggregate([Column(0)], aggs, SCHEMA, [], filter_expr=pred, source=table.scan(batch, row_begin, n_rows))
    return got, ex.counter_get("agg_row8_launches") - r0


_WANT = {}


def _want(name, cols, pred, aggs, row_begin=0, n=N):
    if name not in _WANT:
        _WANT[name] = oracle.run_synth_query(cols, SEED, row_begin, n, 1024, pred, [Column(0)], aggs)[2]
    return _WANT[name]


def _prime(table, pred=HEAD):
    """the table's first query builds both shadows; it keeps 12-byte rows"""
    v0 = ex.counter_get("agg_value_shadow_builds")
    _, row8 = _query(table, pred, [SUM_V], -1)
    assert row8 == 0 and ex.counter_get("agg_value_shadow_builds") == v0 + 1, (row8, ex.counter_get("agg_value_shadow_builds") - v0)


def _off_then_on(table, pred, aggs, want, what, binds=True, **scan):
    got, row8 = _query(table, pred, aggs, 0, **scan)
    assert row8 == 0, f"{what}, option 0: {row8} launches routed 8-byte rows"
    _assert_bit_exact(got, want, f"{what}, option 0")
    l0 = ex.counter_get("agg_value_shadow_launches")
    got, row8 = _query(table, pred, aggs, -1, **scan)
    if binds:
        assert row8 > 0 and row8 <= ex.counter_get("agg_value_shadow_launches") - l0, f"{what}, option -1: {row8}"
    else:
        assert row8 == 0, f"{what}, option -1: {row8} launches routed 8-byte rows"
    _assert_bit_exact(got, want, f"{what}, option -1")
    return got


@pytest.mark.parametrize("groups", [1000, 200000])
def test_headline_predicate(groups):
    cols = syn(groups)
    t = ex.DeviceTable.synth(cols, SEED, 0, N)
    _prime(t)
    _off_then_on(t, HEAD, [SUM_V], _want(f"head{groups}", cols, HEAD, [SUM_V]), f"headline, {groups} groups")


@pytest.mark.parametrize("ws", [8, 4])
def test_no_filter_every_row_routed(ws):
    """... and with agg.pass1_ws = 4 the dense split: four scanners that hash, twelve routers, eight row groups per trip"""
    cols = syn(200000)
    t = ex.DeviceTable.synth(cols, SEED, 0, N)
    ex.set_option("agg.pass1_ws", ws)
    _prime(t, None)
    _off_then_on(t, None, [SUM_V], _want("nofilter", cols, None, [SUM_V]), f"no filter, {ws} scanners")


def test_headline_predicate_dense_split():
    cols = syn(1000)
    t = ex.DeviceTable.synth(cols, SEED, 0, N)
    ex.set_option("agg.pass1_ws", 4)
    _prime(t)
    _off_then_on(t, HEAD, [SUM_V], _want("head1000", cols, HEAD, [SUM_V]), "headline, 4 + 12 waves")


def test_small_table_most_regions_hold_less_than_a_chunk():
    """2^16 + 5 rows, a fifth of them routed to 256 producers' regions: a few rows each, every region ends in a padded line"""
    n = (1 << 16) + 5
    cols = syn(1000)
    t = ex.DeviceTable.synth(cols, SEED, 0, n)
    _prime(t)
    _off_then_on(t, HEAD, [SUM_V], _want("small", cols, HEAD, [SUM_V], 0, n), "2^16 + 5 rows")


@pytest.mark.parametrize("defer", [2, 1])
def test_batches_per_pass2_window(defer):
    cols = syn(1000)
    t = ex.DeviceTable.synth(cols, SEED, 0, N)
    ex.set_option("agg.partition_defer_batches", defer)
    _prime(t)
    d0, p0 = ex.counter_get("agg_deferred_windows"), ex.counter_get("agg_pass2_launches")
    _off_then_on(t, HEAD, [SUM_V], _want("head1000", cols, HEAD, [SUM_V]), f"{defer} batches per window")
    assert (ex.counter_get("agg_deferred_windows") > d0) == (defer == 2), "windows of two batches"
    batches = -(-N // BATCH)  # (four)
    assert ex.counter_get("agg_pass2_launches") - p0 >= 2 * -(-batches // defer)  # (both queries)


def test_tiny_regions_overflow_into_the_spill_list():
    """Regions of one quantum (64 rows; the 12-byte layout rounds it up to its own, 320): pass 1 sends the rows that do not fit to the
    spill list, widened to the Float64 the list holds.  Eight groups and no filter: a producer's 1024 rows of a batch go to at most
    eight regions, 128 rows each on average."""
    cols = syn(8)
    t = ex.DeviceTable.synth(cols, SEED, 0, N)
    _prime(t, None)
    ex.set_option("agg.partition_cap_rows", 64)
    want = _want("nofilter8", cols, None, [SUM_V])
    got, row8 = _query(t, None, [SUM_V], 0)
    assert row8 == 0
    _assert_bit_exact(got, want, "tiny regions, option 0")
    s0 = ex.counter_get("agg_replays_in_place") + ex.counter_get("agg_growths")
    got, row8 = _query(t, None, [SUM_V], -1)
    spilled = ex.counter_get("agg_replays_in_place") + ex.counter_get("agg_growths") - s0
    assert row8 > 0 and spilled > 0, (row8, spilled)
    _assert_bit_exact(got, want, "tiny regions, option -1")


def test_scan_of_a_row_range_that_begins_inside_the_shadows():
    r0, rows = 64 * 4099, (1 << 19) + 5
    cols = syn(1000)
    t = ex.DeviceTable.synth(cols, SEED, 0, N)
    _prime(t)
    _off_then_on(t, HEAD, [SUM_V], _want(f"slice{r0}", cols, HEAD, [SUM_V], r0, rows), "slice", row_begin=r0, n_rows=rows)


LO, HI = 256.0, 512.0
F32 = np.float32
GRID = 2.0 ** -10
# on and one grid step beside both thresholds, both zeros (multiples of 2^-10 below 2^10: a group's sum is exact in any order)
MIXED = [LO - GRID, LO, LO + GRID, HI - GRID, HI, HI + GRID, 0.0, -0.0]
# a group of its own each, 50 rows of one value (50 x a 24-bit mantissa is exact)
ALONE = [float(np.finfo(F32).max), -float(np.finfo(F32).max), float(np.finfo(F32).tiny), -float(np.finfo(F32).tiny)]


@pytest.mark.parametrize("lower,upper", [(Operator.Gt, Operator.Lt), (Operator.GtEq, Operator.LtEq)])
def test_host_table_special_values_at_both_thresholds(lower, upper):
    rng = np.random.default_rng(23)
    k = rng.integers(0, 1000, N).astype(np.int64)
    v = rng.integers(0, 1 << 20, N).astype(np.float64) / 1024.0
    special = rng.choice(N - 64, 1200 + 50 * len(ALONE), replace=False)
    v[special[:1200]] = np.resize(np.array(MIXED), 1200)
    for i, x in enumerate(ALONE):
        rows = special[1200 + 50 * i:1250 + 50 * i]
        k[rows], v[rows] = 1000 + i, x
    v[N - len(MIXED):] = MIXED  # (the ragged last trip)
    whole = pa.RecordBatch.from_arrays([pa.array(k), pa.array(v)], names=["k", "v"])
    batches = [whole.slice(i, min(1 << 18, N - i)) for i in range(0, N, 1 << 18)]
    t = ex.DeviceTable.from_batches(whole.schema, batches)
    _prime(t)
    for pred in (between(1, LO, HI, lower, upper), None):
        want = oracle.aggregate([Column(0)], [SUM_V], [oracle.filter_next(pred, b) if pred is not None else b for b in batches])
        got = _off_then_on(t, pred, [SUM_V], want, f"special values, {'filtered' if pred is not None else 'no filter'}")
    sums = dict(zip(got.column(0).to_pylist(), got.column(1).to_pylist()))
    assert sums[1000] == 50 * float(np.finfo(F32).max) and sums[1003] == -50 * float(np.finfo(F32).tiny)


def test_refused_value_shadow_keeps_twelve_byte_rows():
    """uniform doubles are not Float32-exact: no value shadow, so no launch may meet 8-byte regions"""
    cols = syn(1000, ex.SYNTH_F64_UNIFORM)
    v = np.sort(oracle.synth_column(ex.SYNTH_F64_UNIFORM, 1, 0.0, 1.0, SEED, 0, N))
    pred = between(1, float(v[N // 5]), float(v[2 * N // 5]))
    t = ex.DeviceTable.synth(cols, SEED, 0, N)
    want = _want("uniform_min", cols, pred, [MIN_V])
    for q in range(2):
        got, row8 = _query(t, pred, [SUM_V], -1)
        assert row8 == 0, (q, row8)
    got, row8 = _query(t, pred, [MIN_V], -1)
    assert row8 == 0
    _assert_bit_exact(got, want, "MIN of a uniform operand")


def test_first_query_builds_the_shadows_second_routes_row8():
    cols = syn(1000)
    want = _want("head1000", cols, HEAD, [SUM_V])
    t = ex.DeviceTable.synth(cols, SEED, 0, N)
    b0, l0 = ex.counter_get("agg_value_shadow_builds"), ex.counter_get("agg_value_shadow_launches")
    first, row8 = _query(t, HEAD, [SUM_V], -1)
    assert row8 == 0 and ex.counter_get("agg_value_shadow_builds") == b0 + 1 and ex.counter_get("agg_value_shadow_launches") > l0
    _assert_bit_exact(first, want, "first query")
    second, row8 = _query(t, HEAD, [SUM_V], -1)
    assert row8 > 0 and ex.counter_get("agg_value_shadow_builds") == b0 + 1, row8
    _assert_bit_exact(second, want, "second query")
    assert_groups_identical(first, second, 1, "first against second")


@pytest.mark.parametrize("name,aggs", [("min", [MIN_V]), ("sum_count", [SUM_V, COUNT_V])])
def test_other_aggregates_keep_their_row_forms(name, aggs):
    cols = syn(1000)
    t = ex.DeviceTable.synth(cols, SEED, 0, N)
    _prime(t)
    _off_then_on(t, HEAD, aggs, _want(name, cols, HEAD, aggs), name, binds=False)
