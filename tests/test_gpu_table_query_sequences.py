"""Oracle-bound fuzz of query SEQUENCES over one resident table (csrc/dfx_aggregate_shadow.cpp, dfx_key_shadow.hpp,
dfx_value_shadow.hpp, dfx_routed_shadow.hpp; DESIGN.md sections 2 and 11.2).

A resident table keeps its column shadows, its routed shadows and its calibration memo between queries, found again by the address
of a batch's column slice.  Every sequence of tests/table_query_cases.py builds ONE table of nine columns (263 181 rows: four routed
windows of 2^16 rows and a tail) from three ragged host batches and asks it 8..14 DIFFERENT questions in order: other keys,
aggregates and predicates, other batch widths and row ranges, agg.merge_scan_batches 0 and 1, the shadow options flipped per query,
another table geometry.  Each result is compared with the CPU oracle over the rows of the range -- every group, every column, bit
patterns, the group count, no duplicates; the data is exact, there is no tolerance anywhere, and the truth is never another device
run.  No query may be refused: any ExecutionError fails the test.

Counters, per query, each from a condition in the code: a query that cannot be served by a routed shadow (an option at 0, another
shape than one key and one SUM of a plain Float64 operand, a predicate term off the operand, a column without a shadow, a refused
pair) moves neither agg_routed_shadow_launches nor agg_routed_shadow_builds; any other grows the launches by at most the whole grid
windows inside its range, and by exactly that many in the configuration tests/test_gpu_routed_shadow.py pins (batches of 2 W on the
grid, merge 0) once the pair's shadow exists.  A column shadow whose option is 0 is neither built nor bound.  The last test asserts
that the module as a whole built and bound every kind of shadow.  A failure prints the sequence's replay line, the index of the
failing query and the queries before it.

Run time (one MI355X, measured once): the module alone 58 s in a process of its own -- 53 s of them the first test's setup, the
library's first use of the device -- and 5 s for its 11 tests (0.1-1.1 s per sequence); the whole -m gpu suite with it 553 s, i.e.
about 548 s without it (by difference, not a run of its own).  The first run on a device found nothing wrong in the library."""
import pytest

import oracle
from datafusion_archive_amd import execution as ex
from gpu_util import assert_groups_identical
from table_query_cases import SCHEMA, sequences

pytestmark = pytest.mark.gpu

SEED = 0x7AB1E
SEQS = sequences(SEED)
# every option a query of this module sets travels with its operator (Query.options); should one leak into the process after all,
# this puts back what tests/conftest.py does not
RESET = (("agg.strategy", 0), ("agg.narrow_keys", -1), ("agg.key_shadow", -1), ("agg.value_shadow", -1), ("agg.routed_row8", -1), ("agg.routed_shadow", -1),
         ("agg.routed_shadow_window_rows", 1 << 27), ("agg.partition_cap_rows", 0), ("agg.capacity_log2", 0), ("agg.merge_scan_batches", 0))
COUNTERS = ("agg_key_shadow_builds", "agg_key_shadow_launches", "agg_value_shadow_builds", "agg_value_shadow_launches", "agg_row8_launches",
            "agg_routed_shadow_builds", "agg_routed_shadow_launches")
_RAN = set()
_START = {}


@pytest.fixture(scope="module", autouse=True)
def _counters_at_start():
    for name in COUNTERS:
        _START[name] = ex.counter_get(name)
        assert _START[name] >= 0, f"the library has no counter {name}"
    yield


@pytest.fixture(autouse=True)
def _options():
    yield
    for k, v in RESET:
        ex.set_option(k, v)


def _device(table, q):
    b, n, _rows = q.row_range
    rel = table.scan(q.batch_rows, b, n)
    if q.pred is not None:
        rel = ex.FilterRelation(rel, ex.compile_scalar_expr(None, q.pred, SCHEMA), SCHEMA)
    rel = ex.AggregateRelation(None, rel, [ex.compile_scalar_expr(None, g, SCHEMA) for g in q.group], [ex.compile_expr(None, a, SCHEMA) for a in q.aggs], q.options)
    out = rel.next()
    assert out is not None and rel.next() is None
    return out


def _oracle(whole, q, cache):
    key = (q.key, q.agg_set, q.pred_family, q.range_name)
    if key not in cache:  # (computed once per distinct question of the sequence, never changed)
        b, _n, rows = q.row_range
        part = whole.slice(b, rows)
        cache[key] = oracle.aggregate(q.group, q.aggs, [oracle.filter_next(q.pred, part) if q.pred is not None else part])
    return cache[key]


def _check_counters(s, q, d, built):
    """d: what the counters grew by over the query; built: {pair: (agg.capacity_log2, forced strategy) of the query that built its routed shadow}, before the query"""
    launches, builds = d["agg_routed_shadow_launches"], d["agg_routed_shadow_builds"]
    if not s.eligible(q):
        assert (launches, builds) == (0, 0), f"a query that no routed shadow can serve: {launches} launches scanned a window, {builds} builds"
    else:
        assert builds <= 1 and launches <= q.grid_windows, f"{launches} launches scanned a window, the range holds {q.grid_windows} whole windows of the grid; {builds} builds"
        if builds:
            assert q.pair not in built, "a second build of one pair"
        if q.pinned and q.capacity == 0 and built.get(q.pair) == (0, True):  # (the geometry it was routed for is this query's)
            assert launches == q.grid_windows, f"batches of 2 W on the grid, merge 0, the pair's shadow exists: {launches} launches scanned a window, not {q.grid_windows}"
    if q.key_shadow == 0:
        assert (d["agg_key_shadow_builds"], d["agg_key_shadow_launches"]) == (0, 0), "agg.key_shadow = 0: neither built nor used"
    if q.value_shadow == 0:
        assert (d["agg_value_shadow_builds"], d["agg_value_shadow_launches"]) == (0, 0), "agg.value_shadow = 0: neither built nor used"
    if q.row8 == 0:
        assert d["agg_row8_launches"] == 0, "agg.routed_row8 = 0: no launch routes 8-byte rows"


@pytest.mark.parametrize("index", range(len(SEQS)), ids=[s.name for s in SEQS])
def test_sequence_matches_oracle(index):
    s = SEQS[index]
    whole = s.table.whole()
    table = ex.DeviceTable.from_batches(SCHEMA, s.table.batches())
    assert table.num_rows() == whole.num_rows
    truths, built = {}, {}
    for i, q in enumerate(s.queries):
        where = f"replay: {s.line}\nquery {i} failed; the queries so far:\n{s.history(i)}"
        before = {name: ex.counter_get(name) for name in COUNTERS}
        try:
            got = _device(table, q)
        except ex.ExecutionError as e:  # no query may be refused: the generator draws only shapes the device claims
            pytest.fail(f"{where}\n{e.kind}: {e.message}")
        d = {name: ex.counter_get(name) - before[name] for name in COUNTERS}
        try:
            assert_groups_identical(got, _oracle(whole, q, truths), 1, f"query {i}")
            _check_counters(s, q, d, built)
        except AssertionError as e:
            raise AssertionError(f"{where}\ncounters: {d}\n{e}") from None
        if d["agg_routed_shadow_builds"]:
            built[q.pair] = (q.capacity, q.forced)
        if i == s.build_point:
            assert built, f"{where}\nby the rules of dfx_key_shadow.hpp a routed shadow exists after this query at the latest; none was built"
        print(f"  [{i}] launches {d['agg_routed_shadow_launches']} of {q.grid_windows}, builds k/v/r {d['agg_key_shadow_builds']}/{d['agg_value_shadow_builds']}/{d['agg_routed_shadow_builds']}  {q.line}")
    if s.refused_pairs:
        assert not built, f"replay: {s.line}\na pair that spills was built: {built}"
    _RAN.add(index)


def test_every_shadow_was_built_and_bound():
    """runs last: the counters' growth over this module"""
    missing = [s.name for i, s in enumerate(SEQS) if i not in _RAN]
    assert not missing, f"this test sums up the whole module; sequences that did not pass in this process: {missing}"
    seen = {name: ex.counter_get(name) - _START[name] for name in COUNTERS}
    for name in COUNTERS:
        print(f"  {name:32s} {seen[name]:8d}")
    never = [name for name, v in seen.items() if v <= 0]
    assert not never, f"counters no sequence moved: {never}"
