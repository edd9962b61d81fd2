"""The Float32 shadow of a resident table's Float64 operand column (csrc/dfx_value_shadow.hpp): beside the key's
Int32 shadow, the two compile-time signatures of pass 1 (the headline's, key + SUM) read the operand from a 4-byte copy the table
makes once -- only if EVERY value of the column is exactly its float --, both columns as pair words (PTF_VAL4), 8 bytes per row
instead of 12.  The scanners widen the operand back, so no bit of any result may change: every case is compared bit for bit with
the CPU oracle over the same generator rows (or the same host batches), once with agg.value_shadow = 0 and once with = 1; the
counters say which path ran.

Shapes: 2^20 + 37 rows (odd, a ragged last trip), scanned in batches of 2^18 + 64 rows so that launches begin inside the shadows
on odd 64-row groups.  The tables are too small for a calibration slice, so the partitioned strategy with narrow rows is forced and
the key shadow is built at once (agg.strategy = 3, agg.narrow_keys = 1, agg.key_shadow = 1), as in test_gpu_key_shadow.py."""
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
FORCED = (("agg.strategy", 3), ("agg.narrow_keys", 1), ("agg.key_shadow", 1))
RESET = (("agg.strategy", 0), ("agg.narrow_keys", -1), ("agg.key_shadow", -1), ("agg.value_shadow", -1))


def f64(v):
    return Literal(ScalarValue.Float64(float(v)))


def between(col, lo, hi, lower=Operator.Gt, upper=Operator.Lt):
    return BinaryExpr(BinaryExpr(Column(col), lower, f64(lo)), Operator.And, BinaryExpr(Column(col), upper, f64(hi)))


HEAD = between(1, 204.8, 409.6)
SUM_V = AggregateFunction("SUM", [Column(1)], F64)
MIN_V = AggregateFunction("MIN", [Column(1)], F64)
MAX_V = AggregateFunction("MAX", [Column(1)], F64)
AVG_V = AggregateFunction("AVG", [Column(1)], F64)
COUNT_V = AggregateFunction("COUNT", [Column(1)], U64)
SCHEMA = pa.schema([("k", pa.int64()), ("v", pa.float64())])
SCHEMA3 = pa.schema([("k", pa.int64()), ("v", pa.float64()), ("w", pa.float64())])


def syn(groups, v_kind=ex.SYNTH_F64_EXACT, k_kind=ex.SYNTH_I64_UNIFORM):
    p = (0.0, 1.0) if (v_kind & 0xFF) == ex.SYNTH_F64_UNIFORM else (0.0, 0.0)
    return [("k", k_kind, 0, float(groups), 0.0), ("v", v_kind, 1) + p]


@pytest.fixture(autouse=True)
def _options():
    for k, v in FORCED:
        ex.set_option(k, v)
    yield
    for k, v in RESET:
        ex.set_option(k, v)
    ex.set_option("pool.inject_oom", 0)


def _counters():
    return ex.counter_get("agg_value_shadow_builds"), ex.counter_get("agg_value_shadow_launches")


def _query(table, schema, pred, aggs, option, batch=BATCH, row_begin=0, n_rows=-1):
    """one query over the table under agg.value_shadow = option; returns (result, value shadows built, launches that read one)"""
    ex.set_option("agg.value_shadow", option)
    b0, l0 = _counters()
    got = gpu_aggregate([Column(0)], aggs, schema, [], filter_expr=pred, source=table.scan(batch, row_begin, n_rows))
    b1, l1 = _counters()
    return got, b1 - b0, l1 - l0


_WANT = {}


def _want(name, cols, pred, aggs, row_begin=0, n=N):
    if name not in _WANT:
        _WANT[name] = oracle.run_synth_query(cols, SEED, row_begin, n, 1024, pred, [Column(0)], aggs)[2]
    return _WANT[name]


def _off_then_on(table, schema, pred, aggs, want, what, **scan):
    """The case's two runs: the 12-byte path (option 0: nothing built, nothing read), then over the shadow (option 1)."""
    got, built, launches = _query(table, schema, pred, aggs, 0, **scan)
    assert (built, launches) == (0, 0), f"{what}, option 0: {(built, launches)}"
    _assert_bit_exact(got, want, f"{what}, option 0")
    got, built, launches = _query(table, schema, pred, aggs, 1, **scan)
    assert built == 1 and launches > 0, f"{what}, option 1: {(built, launches)}"
    _assert_bit_exact(got, want, f"{what}, option 1")
    return got


@pytest.mark.parametrize("groups", [1000, 200000])
def test_headline_predicate_twice_on_one_table(groups):
    cols = syn(groups)
    want = _want(f"head{groups}", cols, HEAD, [SUM_V])
    t = ex.DeviceTable.synth(cols, SEED, 0, N)
    first = _off_then_on(t, SCHEMA, HEAD, [SUM_V], want, "first query")
    second, built2, launches2 = _query(t, SCHEMA, HEAD, [SUM_V], 1)
    assert built2 == 0 and launches2 > 0, (built2, launches2)
    assert second.column(1).type == pa.float64()
    _assert_bit_exact(second, want, "second query")
    assert_groups_identical(first, second, 1, "first against second")


def test_auto_rule_builds_with_the_second_query():
    cols = syn(1000)
    want = _want("head1000", cols, HEAD, [SUM_V])
    t = ex.DeviceTable.synth(cols, SEED, 0, N)
    seen = []
    for q in range(3):
        got, built, launches = _query(t, SCHEMA, HEAD, [SUM_V], -1)
        _assert_bit_exact(got, want, f"query {q + 1}")
        seen.append((built, launches > 0))
    assert seen == [(0, False), (1, True), (0, True)], seen


def test_default_options_key_shadow_with_the_second_query_value_shadow_with_the_third():
    """Both options at their default (-1).  A launch asks for the operand's shadow only once the key's is bound, so the table's
    second query builds the key shadow and is the operand column's first asker, and the third builds the value shadow."""
    ex.set_option("agg.key_shadow", -1)
    cols = syn(1000)
    want = _want("head1000", cols, HEAD, [SUM_V])
    t = ex.DeviceTable.synth(cols, SEED, 0, N)
    seen = []
    for q in range(4):
        kb0, kl0 = ex.counter_get("agg_key_shadow_builds"), ex.counter_get("agg_key_shadow_launches")
        got, built, launches = _query(t, SCHEMA, HEAD, [SUM_V], -1)
        _assert_bit_exact(got, want, f"query {q + 1}")
        seen.append((ex.counter_get("agg_key_shadow_builds") - kb0, ex.counter_get("agg_key_shadow_launches") > kl0, built, launches > 0))
    assert seen == [(0, False, 0, False), (1, True, 0, False), (0, True, 1, True), (0, True, 0, True)], seen


def test_option_zero_never_builds_or_reads_a_shadow_that_exists():
    cols = syn(1000)
    want = _want("head1000", cols, HEAD, [SUM_V])
    t = ex.DeviceTable.synth(cols, SEED, 0, N)
    for q, (option, expect) in enumerate(((0, (0, False)), (0, (0, False)), (1, (1, True)), (0, (0, False)))):
        got, built, launches = _query(t, SCHEMA, HEAD, [SUM_V], option)
        assert (built, launches > 0) == expect, (q, built, launches)
        _assert_bit_exact(got, want, f"query {q + 1}")


@pytest.mark.parametrize("r0,rows", [(64 * 3, N - 64 * 3), (64 * 4099, (1 << 19) + 5)])
def test_scan_of_a_slice_starts_inside_the_shadow(r0, rows):
    """A scan that starts at row 64 x 3 (64 x 4099) of the table; its second and later launches begin at row0 = 2^18 + 64, ... of the
    slice.  The shadows are of whole columns: a scan of a row range finds the key's and the operand's alike (Relation::column_memo),
    builds them from the whole column, and a later scan of the whole table reads the same copies."""
    cols = syn(1000)
    want = _want(f"slice{r0}", cols, HEAD, [SUM_V], r0, rows)
    t = ex.DeviceTable.synth(cols, SEED, 0, N)
    kb0, kl0 = ex.counter_get("agg_key_shadow_builds"), ex.counter_get("agg_key_shadow_launches")
    _off_then_on(t, SCHEMA, HEAD, [SUM_V], want, "slice", row_begin=r0, n_rows=rows)
    assert ex.counter_get("agg_key_shadow_builds") - kb0 == 1 and ex.counter_get("agg_key_shadow_launches") > kl0, "the slice's scans did not read the key shadow"
    got, built, launches = _query(t, SCHEMA, HEAD, [SUM_V], 1)
    assert built == 0 and launches > 0 and ex.counter_get("agg_key_shadow_builds") - kb0 == 1, "the whole table's scan made copies of its own"
    _assert_bit_exact(got, _want("head1000", cols, HEAD, [SUM_V]), "the whole table after the slice")


def test_no_filter_every_row_routed():
    cols = syn(200000)
    t = ex.DeviceTable.synth(cols, SEED, 0, N)
    _off_then_on(t, SCHEMA, None, [SUM_V], _want("nofilter", cols, None, [SUM_V]), "no filter")


@pytest.mark.parametrize("name,pred,groups", [("nofilter", None, 200000), ("head1000", HEAD, 1000), ("form_ge_le", between(1, 256.0, 512.0, Operator.GtEq, Operator.LtEq), 1000)])
def test_dense_split_four_scanners_eight_row_groups_per_trip(name, pred, groups):
    """The dense split of the wave-specialised kernel -- four scanner waves, three routers each, StaticKey4Val4Policy<8, SIG>: eight
    row groups (four pairs) per trip -- is the strategy's choice for scans that route most of their rows, made from a calibration
    slice these tables are too small for.  agg.pass1_ws = 4 forces it (as tests/test_gpu_plan.py does), without a filter (key + SUM's
    unit) and with one (the headline's unit, a compile-time form and the ragged last trip of eight groups)."""
    cols = syn(groups)
    t = ex.DeviceTable.synth(cols, SEED, 0, N)
    ex.set_option("agg.pass1_ws", 4)
    try:
        _off_then_on(t, SCHEMA, pred, [SUM_V], _want(name, cols, pred, [SUM_V]), f"4 + 12 waves, {name}")
    finally:
        ex.set_option("agg.pass1_ws", 8)


@pytest.mark.parametrize("lower,upper", [(Operator.Gt, Operator.Lt), (Operator.GtEq, Operator.Lt), (Operator.Gt, Operator.LtEq), (Operator.GtEq, Operator.LtEq)])
def test_comparison_forms_with_rows_at_both_thresholds(lower, upper):
    """The thresholds are values of the column (the 20 % and 40 % quantiles of its rows), so rows sit exactly on both: the four
    forms keep different rows, and the oracle's row counts say so."""
    cols = syn(1000)
    v = np.sort(oracle.synth_column(ex.SYNTH_F64_EXACT, 1, 0.0, 0.0, SEED, 0, N))
    lo, hi = float(v[N // 5]), float(v[2 * N // 5])
    assert lo < hi
    name = f"form{lower}{upper}"
    want = _want(name, cols, between(1, lo, hi, lower, upper), [SUM_V, COUNT_V])
    strict = _want(f"form{Operator.Gt}{Operator.Lt}", cols, between(1, lo, hi), [SUM_V, COUNT_V])
    at = int(np.sum(v == lo)) * (lower == Operator.GtEq) + int(np.sum(v == hi)) * (upper == Operator.LtEq)
    assert int(want.column(2).to_numpy().sum()) - int(strict.column(2).to_numpy().sum()) == at, "the oracle does not see the rows at the thresholds"
    t = ex.DeviceTable.synth(cols, SEED, 0, N)
    pred = between(1, lo, hi, lower, upper)
    sums = _want(name + "sum", cols, pred, [SUM_V])
    _off_then_on(t, SCHEMA, pred, [SUM_V], sums, f"{lower} {upper}")


@pytest.mark.parametrize("name,aggs,binds", [("sum_min", [SUM_V, MIN_V], True), ("avg", [AVG_V], True), ("min", [MIN_V], False), ("max", [MAX_V], False)])
def test_other_aggregates_of_the_operand(name, aggs, binds):
    """SUM, MIN, MAX, AVG of v on a table that has both shadows.  Two or three aggregates of the one operand (SUM + MIN; AVG = SUM +
    COUNT) route its RAW value -- the shape of the headline's signature, whose kernels read the value shadow; pass 2 applies each
    aggregate's transform.  A single MIN or MAX matches neither of the two signatures (they add): it runs the scan plan's kernels,
    which read the key shadow and the 8-byte operand, so nothing binds a value shadow.  All answer bit for bit either way."""
    cols = syn(1000)
    t = ex.DeviceTable.synth(cols, SEED, 0, N)
    _off_then_on(t, SCHEMA, HEAD, [SUM_V], _want("head1000", cols, HEAD, [SUM_V]), "SUM")
    want = _want(name, cols, HEAD, aggs)
    for option in (0, 1):
        got, built, launches = _query(t, SCHEMA, HEAD, aggs, option)
        assert built == 0 and (launches > 0) == (binds and option == 1), (name, option, built, launches)
        _assert_bit_exact(got, want, f"{name}, option {option}")


def _assert_never_shadowed(table, schema, pred, aggs, want, what, exact=True):
    for q, option in enumerate((0, 1, 1)):
        got, built, launches = _query(table, schema, pred, aggs, option)
        assert (built, launches) == (0, 0), f"{what}, query {q + 1}: {(built, launches)}"
        if exact:
            _assert_bit_exact(got, want, f"{what}, query {q + 1}")
        else:
            assert_groups_identical(got, want, 1, f"{what}, query {q + 1}")


def test_uniform_operand_is_refused_for_good():
    """A uniform Float64 operand is not Float32-exact: the first query that may build looks at the whole column, frees the copy and
    marks the column; nobody pays again.  MIN and MAX (order-free) over it are the oracle's bit for bit."""
    cols = syn(1000, ex.SYNTH_F64_UNIFORM)
    v = np.sort(oracle.synth_column(ex.SYNTH_F64_UNIFORM, 1, 0.0, 1.0, SEED, 0, N))
    pred = between(1, float(v[N // 5]), float(v[2 * N // 5]))
    t = ex.DeviceTable.synth(cols, SEED, 0, N)
    spent = []
    for q in range(3):
        us0 = ex.counter_get("agg_value_shadow_build_us")
        got, built, launches = _query(t, SCHEMA, pred, [SUM_V], 1)
        spent.append(ex.counter_get("agg_value_shadow_build_us") - us0)
        assert (built, launches) == (0, 0), f"query {q + 1}: {(built, launches)}"
    assert spent[0] > 0, "the first query never started a build"
    assert spent[1:] == [0, 0], f"a refused column was tried again: {spent}"
    want = _want("uniform_minmax", cols, pred, [MIN_V, MAX_V])
    _assert_never_shadowed(t, SCHEMA, pred, [MIN_V, MAX_V], want, "MIN, MAX of a uniform operand")


def test_nullable_operand_has_no_shadow():
    cols = syn(1000, ex.synth_nulls(ex.SYNTH_F64_EXACT, 5))
    t = ex.DeviceTable.synth(cols, SEED, 0, N)
    _assert_never_shadowed(t, SCHEMA, HEAD, [SUM_V], _want("nullable", cols, HEAD, [SUM_V]), "nullable v", exact=False)


def test_affine_argument_keeps_the_eight_byte_column():
    cols = syn(1000)
    aff = AggregateFunction("SUM", [BinaryExpr(Column(1), Operator.Multiply, f64(2.0))], F64)
    t = ex.DeviceTable.synth(cols, SEED, 0, N)
    _off_then_on(t, SCHEMA, HEAD, [SUM_V], _want("head1000", cols, HEAD, [SUM_V]), "SUM(v)")  # (the table has the shadow)
    _assert_never_shadowed(t, SCHEMA, HEAD, [aff], _want("affine", cols, HEAD, [aff]), "SUM(v * 2.0)")


def test_predicate_on_a_second_float64_column():
    cols = syn(1000) + [("w", ex.SYNTH_F64_EXACT, 2, 0.0, 0.0)]
    pred = between(2, 204.8, 409.6)
    t = ex.DeviceTable.synth(cols, SEED, 0, N)
    _assert_never_shadowed(t, SCHEMA3, pred, [SUM_V], _want("second_column", cols, pred, [SUM_V]), "WHERE w ... SUM(v)")


def test_no_value_shadow_without_the_key_shadow():
    """Wide keys: the key's build is refused, so no launch binds a key shadow -- and the operand's is not even asked for."""
    cols = syn(40000, k_kind=ex.SYNTH_I64_WIDE)
    t = ex.DeviceTable.synth(cols, SEED, 0, N)
    us0 = ex.counter_get("agg_value_shadow_build_us")
    _assert_never_shadowed(t, SCHEMA, HEAD, [SUM_V], _want("wide", cols, HEAD, [SUM_V]), "wide keys")
    assert ex.counter_get("agg_value_shadow_build_us") == us0, "a value shadow build was started"


LO, HI = 256.0, 512.0
F32 = np.float32
# mixed into the ordinary groups: the floats on and next to both thresholds, and both zeros (multiples of 2^-15 below 2^10: any
# order of adding a group's rows gives the same sum)
MIXED = [float(x) for x in (np.nextafter(F32(LO), F32(0)), F32(LO), np.nextafter(F32(LO), F32(1e9)),
                            np.nextafter(F32(HI), F32(0)), F32(HI), np.nextafter(F32(HI), F32(1e9)))] + [0.0, -0.0]
# a group of its own each, 50 rows of one value (50 x a 24-bit mantissa is exact; next to ordinary rows the sum would depend on
# the order of the rows, and +infinity beside -infinity has no value to compare)
ALONE = [float(np.finfo(F32).max), -float(np.finfo(F32).max), float(np.finfo(F32).tiny), -float(np.finfo(F32).tiny), float("inf"), -float("inf")]


def _host_table(k, v):
    whole = pa.RecordBatch.from_arrays([pa.array(k), pa.array(v)], names=["k", "v"])
    per = 1 << 18
    batches = [whole.slice(i, min(per, len(k) - i)) for i in range(0, len(k), per)]
    return ex.DeviceTable.from_batches(whole.schema, batches), batches


def _host_rows(seed):
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 1000, N).astype(np.int64)
    v = rng.integers(0, 1 << 20, N).astype(np.float64) / 1024.0
    return rng, k, v


def _host_want(batches, pred, aggs):
    return oracle.aggregate([Column(0)], aggs, [oracle.filter_next(pred, b) if pred is not None else b for b in batches])


@pytest.mark.parametrize("lower,upper", [(Operator.Gt, Operator.Lt), (Operator.GtEq, Operator.LtEq)])
def test_special_values_are_accepted_and_exact(lower, upper):
    """+0, -0, +-infinity, the largest and the smallest normal floats of both signs and the floats on and next to both thresholds,
    each many times over and in the ragged last trip.  The column is accepted, and the filtered and the unfiltered SUM are the oracle's."""
    rng, k, v = _host_rows(21)
    special = rng.choice(N - 64, 1200 + 50 * len(ALONE), replace=False)
    v[special[:1200]] = np.resize(np.array(MIXED), 1200)
    for i, x in enumerate(ALONE):
        rows = special[1200 + 50 * i:1250 + 50 * i]
        k[rows], v[rows] = 1000 + i, x
    tail = len(MIXED) + len(ALONE)  # (the last trip: every special value once more)
    v[N - tail:] = MIXED + ALONE
    k[N - len(ALONE):] = 1000 + np.arange(len(ALONE))
    t, batches = _host_table(k, v)
    pred = between(1, LO, HI, lower, upper)
    _off_then_on(t, SCHEMA, pred, [SUM_V], _host_want(batches, pred, [SUM_V]), "special values, filtered")
    want = _host_want(batches, None, [SUM_V])
    for option in (0, 1):
        got, built, launches = _query(t, SCHEMA, None, [SUM_V], option)
        assert built == 0 and (launches > 0) == (option == 1), (option, built, launches)
        _assert_bit_exact(got, want, f"special values, no filter, option {option}")
    sums = dict(zip(got.column(0).to_pylist(), got.column(1).to_pylist()))
    assert sums[1004] == float("inf") and sums[1005] == -float("inf") and sums[1000] == 51 * float(np.finfo(F32).max)


@pytest.mark.parametrize("name,odd", [("nan", float("nan")), ("denormal", 2.0 ** -140), ("mantissa25", 300.0 + 2.0 ** -16), ("out_of_range", 1e300)])
def test_one_inexact_element_refuses_the_column(name, odd):
    """One element late in the column that is not exactly a normal float -- a NaN, a Float32 denormal, 25 significant bits, a value
    beyond the Float32 range -- : the build sees it, the copy is freed, the column is never tried again."""
    _, k, v = _host_rows(22)
    v[N - 1000] = odd
    t, batches = _host_table(k, v)
    want = _host_want(batches, HEAD, [SUM_V])
    spent = []
    for q in range(3):
        us0 = ex.counter_get("agg_value_shadow_build_us")
        got, built, launches = _query(t, SCHEMA, HEAD, [SUM_V], 1)
        spent.append(ex.counter_get("agg_value_shadow_build_us") - us0)
        assert (built, launches) == (0, 0), f"{name}, query {q + 1}: {(built, launches)}"
        assert_groups_identical(got, want, 1, f"{name}, query {q + 1}")
    assert spent[0] > 0 and spent[1:] == [0, 0], spent


def test_injected_allocation_failure_during_the_build():
    """The key shadow exists already (one query with agg.value_shadow = 0 made it), so the launches of the query under injection
    bind it and ask for the operand's: that build's allocations are the ones that fail.  The attempt is dropped silently, the query
    answers over the key shadow and the 8-byte operand, the column stays eligible, and the next query builds."""
    cols = syn(1000)
    t = ex.DeviceTable.synth(cols, SEED, 0, N)
    want = _want("head1000", cols, HEAD, [SUM_V])
    got, built, launches = _query(t, SCHEMA, HEAD, [SUM_V], 0)
    assert (built, launches) == (0, 0) and ex.counter_get("agg_key_shadow_builds") >= 1
    _assert_bit_exact(got, want, "before the failure")
    kb0, kl0, us0 = ex.counter_get("agg_key_shadow_builds"), ex.counter_get("agg_key_shadow_launches"), ex.counter_get("agg_value_shadow_build_us")
    ex.set_option("pool.trim", 0)  # (every allocation below misses the pool: the value shadow's are among the failing ones)
    ex.set_option("pool.inject_oom", 64)
    got, built, launches = _query(t, SCHEMA, HEAD, [SUM_V], 1)
    ex.set_option("pool.inject_oom", 0)
    assert (built, launches) == (0, 0), (built, launches)
    assert ex.counter_get("agg_key_shadow_builds") == kb0 and ex.counter_get("agg_key_shadow_launches") > kl0, "the query under injection did not read the key shadow"
    _assert_bit_exact(got, want, "allocation failure during the build")
    got, built, launches = _query(t, SCHEMA, HEAD, [SUM_V], 1)  # the next query asks again: not refused
    assert built == 1 and launches > 0, (built, launches)
    assert ex.counter_get("agg_value_shadow_build_us") > us0
    _assert_bit_exact(got, want, "after the failure")
