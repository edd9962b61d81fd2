"""Oracle-bound fuzz of the grouped aggregate's strategy state machine (csrc/dfx_aggregate_strategy.cpp and
dfx_aggregate_launch.cpp; its states are listed above `enum class Phase` in csrc/dfx_aggregate_impl.hpp).

Every case of tests/agg_stream_cases.py is a stream of 2^21..2^23 rows in 3-6 ragged host batches whose keys, predicate pass
rate or nulls CHANGE after the operator has taken its strategy decision (behind the calibration slice, at a batch boundary), run
with 0-3 per-operator options together.  The device result is compared with the CPU oracle over the same batches: every group,
every column, bit patterns, the group count, no duplicates (the data is exact, there is no tolerance anywhere).  The truth is
never another device run.  COUNT_DISTINCT columns are checked against numpy (the oracle has no such aggregate).  A share of the
cases also runs over a resident table, twice, so that the second run decides from the table's memo.

No case may be refused: any ExecutionError fails the test.  The last test asserts from the library's counters that the module
as a whole reached every transition it is there for.  A failure prints the case's replay line.

Run time (one MI355X, measured once): the module alone 47 s for its 53 tests (46 streams, 3 of them again over a resident table,
twice); the whole -m gpu suite with it 480 s (500 passed), i.e. about 433 s without it (by difference, not a run of its own).  Its
share is dominated by the one-core oracle and by the Python dictionaries of up to 1.6 million groups; the two streams that cross
the 2^20-group load limit take 6-8 s each and cannot be smaller.  46 streams is what it took to witness every transition with
each option of the list in use at least once; nothing was dropped to reach the minute."""
import numpy as np
import pyarrow as pa
import pytest

import oracle
from agg_stream_cases import AGG_SETS, SLICE, cases, distinct_truth
from datafusion_archive_amd import execution as ex
from gpu_util import assert_groups_identical, groups_as_dict

pytestmark = pytest.mark.gpu

SEED = 0xA66
CASES = cases(SEED)
RESIDENT = [c for c in CASES if c.resident]
_RAN = set()
_START = {}

TRANSITIONS = {
    "agg_calibrations": "a calibration slice",
    "agg_memo_decisions": "a decision taken from a resident table's memo",
    "agg_growths": "a table growth",
    "agg_calibration_replays": "a growth or replay during the calibration slice itself",
    "agg_replays_in_place": "a spill list replayed in place without growth",
    "agg_narrow_to_wide": "the narrow -> wide switch of the routed rows",
    "agg_pair_launches": "a pair-scan launch",
    "agg_plane_launches": "a plane launch",
    "agg_shared_operand_launches": "a shared-operand launch",
    "agg_pair_fallbacks": "a fall-back from the pair scan / the planes",
    "agg_pair_fallbacks_pending": "... with a deferred window pending",
    "agg_deferred_windows": "a deferred window that held more than one pass-1 launch",
    "agg_held_runs": "a held-batch run",
    "agg_fewgroup_launches": "a few-group kernel launch",
    "agg_hot_key_launches": "a hot-key launch",
    "agg_unfused_batches": "a batch un-fused because of nulls under the predicate",
    "distinct_set_growths": "a COUNT(DISTINCT) set growth",
    "distinct_spill_rows": "a COUNT(DISTINCT) spill replay",
}


@pytest.fixture(scope="module", autouse=True)
def _counters_at_start():
    for name in TRANSITIONS:
        _START[name] = ex.counter_get(name)
        assert _START[name] >= 0, f"the library has no counter {name}"
    yield


def _device(case, batches=None, source=None):
    schema = case.schema
    rel = source if source is not None else ex.DataSourceRelation(schema, batches)
    if case.pred is not None:
        rel = ex.FilterRelation(rel, ex.compile_scalar_expr(None, case.pred, schema), schema)
    rel = ex.AggregateRelation(None, rel, [ex.compile_scalar_expr(None, g, schema) for g in case.group],
                               [ex.compile_expr(None, a, schema) for a in case.aggs], case.options or None)
    out = rel.next()
    assert out is not None and rel.next() is None
    return out


def _oracle(case, batches):
    pred = case.pred
    fed = [oracle.filter_next(pred, b) for b in batches] if pred is not None else batches
    return oracle.aggregate(case.group, case.plain_aggs, fed)


def _compare(case, got, want, batches, what):
    dpos = case.distinct_positions
    plain = [i for i in range(got.num_columns) if i - case.n_keys not in dpos]
    assert got.num_columns == case.n_keys + len(case.aggs)
    got_plain = pa.RecordBatch.from_arrays([got.column(i) for i in plain], names=["c%d" % i for i in plain])
    assert_groups_identical(got_plain, want, case.n_keys, what)
    for pos in dpos:
        truth = distinct_truth(case, batches, AGG_SETS[case.agg_set][pos][1])
        cols = [got.column(i) for i in range(case.n_keys)] + [got.column(case.n_keys + pos)]
        g = groups_as_dict(pa.RecordBatch.from_arrays(cols, names=["c%d" % i for i in range(len(cols))]), case.n_keys)
        bad = [k for k in truth if g.get(k) != (truth[k],)]
        assert len(g) == len(truth) and not bad, f"{what}: COUNT_DISTINCT column {pos}: {len(bad)} groups differ, e.g. {bad[:1]}: got {g.get(bad[0]) if bad else None} want {truth[bad[0]] if bad else None}"


def _check_crossing(case, batches, final_groups):
    """the generator's promise, at full size: the slice's group count and the final one lie on opposite sides of the threshold"""
    if not case.crosses:
        return
    thr, way = case.crosses
    first = next(b for b in batches if b.num_rows)
    k = first.column(0).to_numpy()[:SLICE]
    if case.pred is not None:
        c = first.column(case.columns.index(case.pred_col)).to_numpy()[:SLICE]
        k = k[(c > 204.8) & (c < 409.6)]
    seen = len(np.unique(k))
    print(f"  {case.name}: slice saw {seen} groups, final {final_groups}, threshold {thr} ({way})")
    if way == "few->many":
        assert seen <= thr < final_groups, (case.line, seen, final_groups)
    else:
        assert seen >= thr, (case.line, seen)


@pytest.mark.parametrize("index", range(len(CASES)), ids=[c.name for c in CASES])
def test_stream_matches_oracle(index):
    case = CASES[index]
    batches = case.batches()
    try:
        got = _device(case, batches)
    except ex.ExecutionError as e:  # no case may be refused: the generator draws only shapes the device claims
        pytest.fail(f"replay: {case.line}\n{e.kind}: {e.message}")
    want = _oracle(case, batches)
    try:
        _compare(case, got, want, batches, "host batches")
        _check_crossing(case, batches, want.num_rows)
    except AssertionError as e:
        raise AssertionError(f"replay: {case.line}\n{e}") from None
    _RAN.add(("host", index))


@pytest.mark.parametrize("which", range(len(RESIDENT)), ids=[c.name for c in RESIDENT])
def test_resident_table_twice_matches_oracle(which):
    """the same stream as one resident table scanned in batches of one fixed width above 2^21 rows (a table scan cannot be ragged);
    the second run takes its strategy from the memo the first one left with the table.  Both against the oracle."""
    case = RESIDENT[which]
    batches = [b for b in case.batches() if b.num_rows]
    whole = pa.Table.from_batches(batches, schema=case.schema).combine_chunks().to_batches()[0]
    width = (1 << 21) + 64 * (37 + 2 * which)
    slices = [whole.slice(i, width) for i in range(0, whole.num_rows, width)]
    want = _oracle(case, slices)
    table = ex.DeviceTable.from_batches(case.schema, batches)
    assert table.num_rows() == whole.num_rows
    memo = ex.counter_get("agg_memo_decisions")
    for run in (1, 2):
        try:
            got = _device(case, source=table.scan(width))
            _compare(case, got, want, slices, f"resident table, run {run}")
        except ex.ExecutionError as e:
            pytest.fail(f"replay (resident table, width {width}, run {run}): {case.line}\n{e.kind}: {e.message}")
        except AssertionError as e:
            raise AssertionError(f"replay (resident table, width {width}, run {run}): {case.line}\n{e}") from None
    assert ex.counter_get("agg_memo_decisions") > memo, f"the second run did not decide from the memo: {case.line}"
    _RAN.add(("resident", which))


def test_small_table_slice_overflow_regression():
    """Hand-written twin of the round-6 lost-groups bug: the calibration slice overflows a table of 2^14 slots, and its spilled rows
    must be replayed before the strategy decision replaces the spill list.  With that replay removed from a scratch build this
    stream (SUM(v), MIN(w) over 200 000 then 400 000 uniform keys under the headline predicate) came back with 240 596 of 242 909
    groups; the same stream from 2^11 or 2^13 slots did not show the loss."""
    case = next(c for c in CASES if c.name == "small_table_pair")
    assert case.options["agg.capacity_log2"] == 14 and case.first_big
    batches = case.batches()
    before = ex.counter_get("agg_calibration_replays")
    got = _device(case, batches)
    assert ex.counter_get("agg_calibration_replays") == before + 1
    try:
        _compare(case, got, _oracle(case, batches), batches, "small table")
    except AssertionError as e:
        raise AssertionError(f"replay: {case.line}\n{e}") from None


def test_every_transition_was_seen():
    """runs last: the counters' growth over this module"""
    missing_runs = [c.name for i, c in enumerate(CASES) if ("host", i) not in _RAN] + [c.name + " (resident)" for i, c in enumerate(RESIDENT) if ("resident", i) not in _RAN]
    assert not missing_runs, f"this test sums up the whole module; cases that did not pass in this process: {missing_runs}"
    seen = {name: ex.counter_get(name) - _START[name] for name in TRANSITIONS}
    for name, what in TRANSITIONS.items():
        print(f"  {name:32s} {seen[name]:8d}   {what}")
    never = [f"{name} ({TRANSITIONS[name]})" for name, v in seen.items() if v <= 0]
    assert not never, f"transitions no case reached: {never}"
