"""ORDER BY / LIMIT on the device against the case matrix of tests/sort_cases.py: every case of every family runs through
DataSourceRelation / DeviceTable.scan -> SortRelation -> optional LimitRelation and must equal oracle.sort_batches bit for bit
(the oracle itself is held against a second reference on the same cases by tests/test_sort_cases_host.py).  Three counters that
decide nothing (sort_passes_run, sort_passes_skipped, sort_topk_selects) witness that the cases reach the paths they are for."""
import pytest

import oracle
import sort_cases as sc
from datafusion_archive_amd import execution as ex
from gpu_util import assert_batches_identical

pytestmark = pytest.mark.gpu

CASES = {name: fam() for name, fam in sc.FAMILIES.items()}
_FULL = {}


def _by(family, key):
    groups = {}
    for c in CASES[family]:
        groups.setdefault(key(c), []).append(c)
    return groups


TYPES = _by("types", lambda c: c.tags[0])
ROWS = _by("row_edges", lambda c: c.tags[0])
OFFSETS = _by("offsets", lambda c: c.tags[0])
NULLS = _by("null_layout", lambda c: c.name)
UTF8 = _by("utf8", lambda c: c.name)
TOPK = _by("topk", lambda c: c.data.name)
MIXES = _by("mixes", lambda c: "mix%03d-%03d" % (int(c.name[3:]) // 25 * 25, int(c.name[3:]) // 25 * 25 + 24))


def full_sort(case):
    key = (case.data.name, case.key_text)
    if key not in _FULL:
        _FULL[key] = oracle.sort_batches(case.data.batches, case.keys)
    return _FULL[key]


def gpu_sort(case):
    schema = case.schema
    if case.source == "resident":
        table = ex.DeviceTable.from_batches(schema, case.table_batches())
        rel = table.scan(sc.RESIDENT_BATCH, sc.RESIDENT_BEGIN, case.data.num_rows)
    else:
        rel = ex.DataSourceRelation(schema, case.batches())
    rel = ex.SortRelation(rel, [(ex.compile_scalar_expr(None, e, schema), asc) for e, asc in case.keys], schema)
    if case.limit is not None:
        rel = ex.LimitRelation(rel, case.limit, schema)
    return list(rel)


def check(case):
    got = gpu_sort(case)
    want = sc.expected(case, full_sort(case))
    if want is None:
        assert got == [], case.line
        return
    assert len(got) == 1, (case.line, [b.num_rows for b in got])
    assert_batches_identical(got[0], want, case.line)


def counters():
    return {n: ex.counter_get(n) for n in ("sort_passes_run", "sort_passes_skipped", "sort_topk_selects")}


def test_counters_reset_to_zero():
    check(sc.witness_passes())
    assert ex.counter_get("sort_passes_run") > 0
    ex.counter_reset()
    assert counters() == {"sort_passes_run": 0, "sort_passes_skipped": 0, "sort_topk_selects": 0}


def test_int64_below_2_20_costs_three_passes():
    """"an Int64 key below 2^20 costs 3 passes, not 8" """
    case = sc.witness_passes()
    ex.counter_reset()
    check(case)
    assert counters() == {"sort_passes_run": 3, "sort_passes_skipped": 5, "sort_topk_selects": 0}, case.line


@pytest.mark.parametrize("group", list(TYPES))
def test_key_types(group):
    ex.counter_reset()
    for case in TYPES[group]:
        check(case)
    c = counters()
    assert c["sort_passes_run"] > 0 and c["sort_passes_skipped"] > 0 and c["sort_topk_selects"] == 0, (group, c)


@pytest.mark.parametrize("group", list(ROWS))
def test_row_count_edges(group):
    for case in ROWS[group]:
        check(case)


@pytest.mark.parametrize("group", list(OFFSETS))
def test_offsets(group):
    """as built, sliced at odd offsets and scanned from a resident table: one expected result for all of them"""
    assert {c.source for c in OFFSETS[group]} == {"host", "sliced", "resident"}
    assert len({(c.data.name, c.key_text) for c in OFFSETS[group]}) == 1
    for case in OFFSETS[group]:
        check(case)


@pytest.mark.parametrize("name", list(NULLS))
def test_null_layout(name):
    (case,) = NULLS[name]
    ex.counter_reset()
    check(case)
    if "no-pass" in case.tags:  # all-null, all-equal and literal keys: every digit of every image is constant
        c = counters()
        assert c["sort_passes_run"] == 0 and c["sort_passes_skipped"] >= 8, (case.line, c)


@pytest.mark.parametrize("name", list(UTF8))
def test_utf8_keys(name):
    (case,) = UTF8[name]
    check(case)


@pytest.mark.parametrize("group", list(TOPK))
def test_top_k(group):
    """the prefix of the full sort for every k; the radix select runs for exactly the cases the documented rule predicts"""
    ex.counter_reset()
    predicted = 0
    for case in TOPK[group]:
        check(case)
        predicted += int(case.selects())
        assert ex.counter_get("sort_topk_selects") == predicted, case.line


@pytest.mark.parametrize("group", list(MIXES))
def test_random_mixes(group):
    for case in MIXES[group]:
        check(case)
