"""The row source of the scan kernels (csrc/dfx_row_source.hpp) on the device: one small query per (ScanKernel, RowSource class)
that the launchers' switches can reach, each against the CPU oracle bit for bit (COUNT(DISTINCT), which the reference lacks:
against numpy) -- a wrong mapping from RowSource to template arguments, or a plan launch that reads the caller's columns, shows
at any size.  Three batches of 8 205 rows (not a multiple of 64, more than one workgroup); 5 groups for the register-accumulator
kernel (the first batch decides, the other two run it), 3 000 groups for the table kernels under agg.strategy 1 and 2 and for
the generic pass 1 under agg.strategy 3, no keys for the reduction.  The rungs are reached with the options that exist:
scan.fast 0 for the interpreter, scan.plan 0 / 1 / 2, a nullable or Int32 column for the plan, 2 / 4 / 5+ referenced columns
for the classes, the Q1 shape, filter.dense 1, filter.single_pass 0 / 1."""
import numpy as np
import pyarrow as pa
import pytest

import oracle
from datafusion_archive_amd import execution as ex
from datafusion_archive_amd.logicalplan import AggregateFunction, BinaryExpr, Column, DataType, Literal, Operator, ScalarValue
from gpu_util import assert_batches_identical, assert_groups_identical, gpu_aggregate, gpu_filter, gpu_project

pytestmark = pytest.mark.gpu

F64, I64, U64 = DataType.Float64, DataType.Int64, DataType.UInt64
BATCH = 8205
N = 3 * BATCH
SEED = 0xDF10
OPTIONS = (("agg.strategy", 0), ("scan.fast", 1), ("scan.plan", 1), ("agg.fewgroup", 1), ("filter.dense", -1), ("filter.single_pass", 1))


@pytest.fixture(autouse=True)
def _defaults():
    for k, v in OPTIONS:
        ex.set_option(k, v)
    yield
    for k, v in OPTIONS:
        ex.set_option(k, v)


def f64(v):
    return Literal(ScalarValue.Float64(v))


def i64(v):
    return Literal(ScalarValue.Int64(v))


def AND(*terms):
    e = terms[0]
    for t in terms[1:]:
        e = BinaryExpr(e, Operator.And, t)
    return e


def agg(f, col, t):
    return AggregateFunction(f, [Column(col)], t)


# columns: 0 k Int64 in [0, groups), 1 v Float64 exact (m * 2^-10), 2 w Int64 in [0, 1000), 3 x Float64 in [0, 1), 4 y Float64 exact
def syn(groups, v_nulls=0, w_kind=None, w_range=1000.0):
    return [("k", ex.SYNTH_I64_UNIFORM, 0, float(groups), 0.0), ("v", ex.synth_nulls(ex.SYNTH_F64_EXACT, v_nulls), 1, 0.0, 0.0),
            ("w", ex.SYNTH_I64_UNIFORM if w_kind is None else w_kind, 2, w_range, 0.0), ("x", ex.SYNTH_F64_UNIFORM, 3, 0.0, 1.0),
            ("y", ex.SYNTH_F64_EXACT, 4, 0.0, 0.0)]


def schema_of(cols):
    t = {ex.SYNTH_I64_UNIFORM: pa.int64(), ex.SYNTH_I32_UNIFORM: pa.int32()}
    return pa.schema([(c[0], t.get(c[1] & 0xFF, pa.float64())) for c in cols])


HEAD = AND(BinaryExpr(Column(1), Operator.Gt, f64(204.8)), BinaryExpr(Column(1), Operator.Lt, f64(409.6)))   # columns: v
W_LT = BinaryExpr(Column(2), Operator.Lt, i64(700))                                                          # ... w
W32_LT = BinaryExpr(Column(2), Operator.Lt, Literal(ScalarValue.Int32(700)))
X_LT = BinaryExpr(Column(3), Operator.Lt, f64(0.75))                                                         # ... x
SUM_V, MIN_V, COUNT_V, SUM_Y, MAX_W = agg("SUM", 1, F64), agg("MIN", 1, F64), agg("COUNT", 1, U64), agg("SUM", 4, F64), agg("MAX", 2, I64)

# the Q1 shape (dfx_sigs.hpp: SigQ1): exact columns, so the SUMs of products do not depend on the order
def syn_q1(g0, g1):
    return [("rf", ex.SYNTH_I64_UNIFORM, 0, float(g0), 0.0), ("ls", ex.SYNTH_I64_UNIFORM, 1, float(g1), 0.0), ("qty", ex.SYNTH_F64_EXACT, 2, 12.0, 2.0),
            ("price", ex.SYNTH_F64_EXACT, 3, 12.0, 2.0), ("disc", ex.SYNTH_F64_EXACT, 4, 2.0, 2.0), ("tax", ex.SYNTH_F64_EXACT, 5, 2.0, 2.0),
            ("ship", ex.SYNTH_F64_UNIFORM, 6, 0.0, 2526.0)]


_DP = BinaryExpr(Column(3), Operator.Multiply, BinaryExpr(f64(1.0), Operator.Minus, Column(4)))
Q1_AGGS = [agg("sum", 2, F64), agg("sum", 3, F64), AggregateFunction("sum", [_DP], F64),
           AggregateFunction("sum", [BinaryExpr(_DP, Operator.Multiply, BinaryExpr(f64(1.0), Operator.Plus, Column(5)))], F64)]
Q1_PRED = AND(BinaryExpr(Column(6), Operator.LtEq, f64(2436.0)), BinaryExpr(Column(4), Operator.GtEq, f64(0.0)))

# programs by referenced columns and what makes them miss every signature: (predicate, aggregates, group columns -> columns referenced)
C2 = (HEAD, [MIN_V])                    # v, k            (MIN: no signature)
C4 = (AND(HEAD, W_LT, X_LT), [MIN_V])   # v, w, x, k
C8 = (AND(HEAD, W_LT, X_LT), [SUM_Y])   # v, w, x, k, y
R2 = (HEAD, [MIN_V, MAX_W])             # ungrouped: v, w
R4 = (AND(HEAD, X_LT), [MIN_V, MAX_W, SUM_Y])   # v, x, w, y; three accumulators: the kernel for up to eight
R8 = (AND(HEAD, W_LT, X_LT), [MIN_V, SUM_Y, agg("MIN", 0, I64)])  # v, w, x, y, k


def run_agg(cols, group, pred, aggs, opts):
    for k, v in opts:
        ex.set_option(k, v)
    t = ex.DeviceTable.synth(cols, SEED, 0, N)
    got = gpu_aggregate(group, aggs, schema_of(cols), [], filter_expr=pred, source=t.scan(BATCH))
    _s, _kept, want = oracle.run_synth_query(cols, SEED, 0, N, 1024, pred, group, aggs)
    return got, want


K = [Column(0)]
PLAN0, PLAN2, INTERP = ("scan.plan", 0), ("scan.plan", 2), ("scan.fast", 0)

# id -> (synthetic columns, group, (predicate, aggregates), options); the table kernels run each under agg.strategy 1 and 2
HASH_AGG = {
    "sig_key_sum_pred2_f64": (syn(3000), K, (HEAD, [SUM_V]), ()),                     # static shape KeySumPred2F64
    "sig_key_sum": (syn(3000), K, (None, [SUM_V]), ()),                               # static shape KeySum
    "sig_q1": (syn_q1(60, 50), [Column(0), Column(1)], (Q1_PRED, Q1_AGGS), ()),       # static shape Q1 in the table kernel (3 000 groups)
    "plan_c2_nullable": (syn(3000, v_nulls=100), K, (HEAD, [SUM_V]), ()),             # plan_c2: a validity bitmap asks for the plan
    "plan_c2_first": (syn(3000), K, C2, (PLAN2,)),                                    # plan_c2: scan.plan = 2 asks for it
    "plan_c4_int32": (syn(3000, w_kind=ex.SYNTH_I32_UNIFORM), K, (AND(HEAD, W32_LT), [MIN_V]), ()),  # plan_c4: a 4-byte column, three plan columns
    "fast_c2": (syn(3000), K, C2, ()),
    "fast_c4": (syn(3000), K, C4, ()),
    "fast_c8": (syn(3000), K, C8, ()),
    "fast_c2_no_plan": (syn(3000), K, C2, (PLAN0,)),
    "interp_c2": (syn(3000), K, C2, (INTERP,)),                                       # scan.fast = 0: the interpreter, three classes
    "interp_c4": (syn(3000), K, C4, (INTERP,)),
    "interp_c8": (syn(3000), K, C8, (INTERP,)),
    "interp_c2_nulls_no_plan": (syn(3000, v_nulls=100), K, (None, [MIN_V]), (PLAN0,)),  # nulls without a plan: the interpreter
}


@pytest.mark.parametrize("strategy", [1, 2])
@pytest.mark.parametrize("name", list(HASH_AGG))
def test_hash_agg(name, strategy):
    """k_hash_agg: each case reaches the rung its name says, under the table-only strategy and the LDS front cache"""
    cols, group, (pred, aggs), opts = HASH_AGG[name]
    before = ex.counter_get("agg_fewgroup_launches")
    got, want = run_agg(cols, group, pred, aggs, (("agg.strategy", strategy),) + opts)
    assert_groups_identical(got, want, len(group), f"hash_agg {name} strategy {strategy}")
    assert want.num_rows > 1000 and ex.counter_get("agg_fewgroup_launches") == before


FEWGROUP = {
    "sig_q1": (syn_q1(5, 1), [Column(0), Column(1)], (Q1_PRED, Q1_AGGS), ()),         # static shape Q1 in the register kernel (5 groups)
    "plan_c2_nullable": (syn(5, v_nulls=100), K, (HEAD, [SUM_V]), ()),                # plan_c2, one key word
    "plan_c4_int32_two_keys": (syn(5, w_kind=ex.SYNTH_I32_UNIFORM, w_range=1.0), [Column(0), Column(2)], (HEAD, [MIN_V]), ()),  # plan_c4, two key words (the second an Int32 constant)
    "plan_c4_first": (syn(5), K, C4, (PLAN2,)),                                       # plan_c4: scan.plan = 2
    "fast_c2": (syn(5), K, C2, ()),
    "fast_c4": (syn(5), K, C4, ()),
    "fast_c8": (syn(5), K, C8, ()),
    "fast_c2_sum": (syn(5), K, (HEAD, [SUM_V]), ()),                                  # the headline's shape: no signature in this kernel, fast_c2
}


@pytest.mark.parametrize("name", list(FEWGROUP))
def test_fewgroup(name):
    """k_fewgroup_agg: the first batch goes through the table kernel and finds <= 8 groups, the other two run on register accumulators"""
    cols, group, (pred, aggs), opts = FEWGROUP[name]
    before = ex.counter_get("agg_fewgroup_launches")
    got, want = run_agg(cols, group, pred, aggs, opts)
    assert_groups_identical(got, want, len(group), f"fewgroup {name}")
    assert ex.counter_get("agg_fewgroup_launches") == before + 2


REDUCE = {
    "sig_count_pred2_f64": (syn(5), (HEAD, [COUNT_V]), ()),                           # static shape CountPred2F64
    "sig_sum_count_pred2_f64": (syn(5), (HEAD, [SUM_V, COUNT_V]), ()),                # static shape SumCountPred2F64
    "plan_c2_nullable": (syn(5, v_nulls=100), (HEAD, [MIN_V, COUNT_V]), ()),          # plan_c2, two accumulators
    "plan_c2_nullable_count": (syn(5, v_nulls=100), (HEAD, [COUNT_V]), ()),           # plan_c2: the signature refuses nulls
    "plan_c4_int32": (syn(5, w_kind=ex.SYNTH_I32_UNIFORM), (AND(HEAD, W32_LT, X_LT), [MIN_V, SUM_Y, COUNT_V]), ()),  # plan_c4, three accumulators
    "plan_c2_first": (syn(5), R2, (PLAN2,)),
    "fast_c2": (syn(5), R2, ()),
    "fast_c4": (syn(5), R4, ()),
    "fast_c8": (syn(5), R8, ()),
    "interp_c2": (syn(5), R2, (INTERP,)),
    "interp_c4": (syn(5), R4, (INTERP,)),
    "interp_c8": (syn(5), R8, (INTERP,)),
    "interp_c2_nulls_no_plan": (syn(5, v_nulls=100), (HEAD, [MIN_V, COUNT_V]), (PLAN0,)),  # nulls without a plan (the Filter is un-fused): the interpreter
}


@pytest.mark.parametrize("name", list(REDUCE))
def test_reduce(name):
    """k_reduce: ungrouped aggregates, each case the rung its name says"""
    cols, (pred, aggs), opts = REDUCE[name]
    got, want = run_agg(cols, [], pred, aggs, opts)
    assert_groups_identical(got, want, 0, f"reduce {name}")


PASS1 = {"fast_c2": (C2, (PLAN0,)), "fast_c4": (C4, (PLAN0,)), "fast_c8": (C8, (PLAN0,)),
         "interp_c2": (C2, (PLAN0, INTERP)), "interp_c4": (C4, (PLAN0, INTERP)), "interp_c8": (C8, (PLAN0, INTERP))}


@pytest.mark.parametrize("name", list(PASS1))
def test_pass1_generic(name):
    """the generic pass 1 of the partitioned strategy (agg.strategy = 3, scan.plan = 0: neither a signature nor the plan takes the launch)"""
    (pred, aggs), opts = PASS1[name]
    before = ex.counter_get("agg_pass2_launches")
    got, want = run_agg(syn(3000), K, pred, aggs, (("agg.strategy", 3),) + opts)
    assert_groups_identical(got, want, 1, f"pass 1 {name}")
    assert ex.counter_get("agg_pass2_launches") > before


def _distinct_truth(cols, keep):
    k = oracle.synth_column(*cols[0][1:], SEED, 0, N)[keep]
    w = oracle.synth_column(*cols[2][1:], SEED, 0, N)[keep]
    pairs = np.unique(k * 1000 + w)
    ks, counts = np.unique(pairs // 1000, return_counts=True)
    return dict(zip(ks.tolist(), counts.tolist()))


DISTINCT = {
    "plan_c2": (None, ()),                                   # k, w: the plan for plain columns
    "plan_c4": ("v_x", ()),                                  # v, x, k, w: four plan columns
    "interp_c4": ("v_x", (PLAN0,)),                          # no plan: the interpreter, <= 4 columns
    "interp_c4_two_columns": (None, (PLAN0,)),               # ... which is also the class of two columns (no <= 2 class in this kernel)
    "interp_c8": ("v_x_y", ()),                              # v, x, y, k, w: more columns than a plan binds
}


@pytest.mark.parametrize("name", list(DISTINCT))
def test_distinct_insert(name):
    """k_distinct_insert: COUNT(DISTINCT w) GROUP BY k over 3 000 groups, against numpy"""
    which, opts = DISTINCT[name]
    cols = syn(3000)
    v, x, y = (oracle.synth_column(*cols[i][1:], SEED, 0, N) for i in (1, 3, 4))
    keep = np.ones(N, dtype=bool)
    pred = None
    if which is not None:
        keep = (v > 204.8) & (v < 409.6) & (x < 0.75)
        pred = AND(HEAD, X_LT)
        if which == "v_x_y":
            keep &= y >= 100.0
            pred = AND(pred, BinaryExpr(Column(4), Operator.GtEq, f64(100.0)))
    for k, val in opts:
        ex.set_option(k, val)
    t = ex.DeviceTable.synth(cols, SEED, 0, N)
    got = gpu_aggregate(K, [AggregateFunction("COUNT_DISTINCT", [Column(2)], U64)], schema_of(cols), [], filter_expr=pred, source=t.scan(BATCH))
    assert dict(zip(got.column(0).to_pylist(), got.column(1).to_pylist())) == _distinct_truth(cols, keep), name


def _host_batches(cols):
    return [oracle.synth_batch(cols, SEED, i * BATCH, BATCH) for i in range(3)]


FILTER = {
    "sig_pred2_f64": (syn(5), HEAD, ()),                                             # static shape Pred2F64
    "fast_c2": (syn(5), AND(HEAD, W_LT), ()),
    "fast_c4": (syn(5), AND(HEAD, W_LT, X_LT), ()),
    # (no fast_c8: a decoded conjunction has at most four terms, so at most four columns)
    "interp_c2": (syn(5), AND(HEAD, W_LT), (INTERP,)),
    "interp_c4": (syn(5), AND(HEAD, W_LT, X_LT), (INTERP,)),
    "interp_c8": (syn(5), AND(HEAD, W_LT, X_LT, BinaryExpr(Column(4), Operator.GtEq, f64(100.0)), BinaryExpr(Column(0), Operator.NotEq, i64(3))), (INTERP,)),
    "interp_c2_nulls": (syn(5, v_nulls=100), HEAD, ()),                               # a batch with nulls: the interpreter
}


@pytest.mark.parametrize("single_pass", [1, 0])
@pytest.mark.parametrize("name", list(FILTER))
def test_filter(name, single_pass):
    """FilterRelation on its own: k_filter_fused (filter.single_pass = 1) and k_predicate_mask + k_compact (0)"""
    cols, pred, opts = FILTER[name]
    for k, v in (("filter.single_pass", single_pass),) + opts:
        ex.set_option(k, v)
    batches = _host_batches(cols)
    got = gpu_filter(pred, batches[0].schema, batches)
    assert len(got) == 3
    for i, (g, b) in enumerate(zip(got, batches)):
        assert_batches_identical(g, oracle.filter_next(pred, b), f"filter {name} single_pass {single_pass} batch {i}")


@pytest.mark.parametrize("op_lo,op_hi", [(Operator.Gt, Operator.Lt), (Operator.GtEq, Operator.Lt), (Operator.Gt, Operator.LtEq), (Operator.GtEq, Operator.LtEq)])
def test_filter_dense_forms(op_lo, op_hi):
    """k_filter_fused_dense (filter.dense = 1): the signature's dense forms, one kernel per comparison form"""
    ex.set_option("filter.dense", 1)
    cols = [("v", ex.SYNTH_F64_EXACT, 1, 0.0, 0.0)]
    pred = AND(BinaryExpr(Column(0), op_lo, f64(204.75)), BinaryExpr(Column(0), op_hi, f64(819.25)))
    batches = _host_batches(cols)
    got = gpu_filter(pred, batches[0].schema, batches)
    for i, (g, b) in enumerate(zip(got, batches)):
        assert_batches_identical(g, oracle.filter_next(pred, b), f"dense batch {i}")


PROJECT = {
    "interp_c2": [BinaryExpr(Column(1), Operator.Plus, Column(4)), BinaryExpr(Column(1), Operator.Lt, Column(4))],
    "interp_c4": [BinaryExpr(BinaryExpr(Column(1), Operator.Multiply, Column(3)), Operator.Minus, Column(4)), BinaryExpr(Column(0), Operator.Plus, i64(7))],
    "interp_c8": [BinaryExpr(BinaryExpr(Column(1), Operator.Multiply, Column(3)), Operator.Minus, Column(4)), BinaryExpr(Column(0), Operator.Multiply, Column(2))],
}


@pytest.mark.parametrize("nulls", [0, 100])
@pytest.mark.parametrize("name", list(PROJECT))
def test_project(name, nulls):
    """ProjectRelation on its own: the interpreter over 2, 4 and 5 referenced columns, with and without a validity bitmap"""
    batches = _host_batches(syn(5, v_nulls=nulls))
    got = gpu_project(PROJECT[name], batches[0].schema, batches)
    assert len(got) == 3
    for i, (g, b) in enumerate(zip(got, batches)):
        assert_batches_identical(g, oracle.project_next(PROJECT[name], b), f"project {name} batch {i}")
