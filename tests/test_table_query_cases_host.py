"""CPU side of the resident-table query fuzz (tests/table_query_cases.py, tests/test_gpu_table_query_sequences.py): the generator is
deterministic and keeps its promises about the table, it covers every family it lists, and the oracle agrees bit for bit with an
independent numpy truth on every query that touches no nullable column (numpy adds in another order than the oracle: equal bits prove
that the values are exact).  Everything runs at full size: the table has 263 181 rows."""
import numpy as np
import pyarrow as pa
import pytest

import oracle
from gpu_util import assert_groups_identical
from table_query_cases import (AGG_SETS, BATCH_WIDTHS, COLUMNS, HI, KEYS, LO, PRED_FAMILIES, RANGES, ROWS, SCHEMA, W, numpy_truth, sequences)

SEED = 0x7AB1E
SEQS = sequences(SEED)
QUERIES = [q for s in SEQS for q in s.queries]


def test_sequences_are_deterministic():
    again = sequences(SEED)
    assert [s.line for s in SEQS] == [s.line for s in again]
    assert [[q.line for q in s.queries] for s in SEQS] == [[q.line for q in s.queries] for s in again]
    assert len({s.name for s in SEQS}) == len(SEQS)
    for a, b in list(zip(SEQS, again))[::4]:
        assert a.table.batch_lengths() == b.table.batch_lengths()
        assert a.table.whole().equals(b.table.whole())
    assert not sequences(SEED + 1)[0].table.whole().equals(SEQS[0].table.whole())
    assert [q.line for q in sequences(SEED + 1)[0].queries] != [q.line for q in SEQS[0].queries]  # (the drawn part)


def test_tables_keep_their_promises():
    assert ROWS == 4 * W + 1000 + 37 and (ROWS - 4 * W) % 64 != 0 and ROWS % 64 != 0
    assert 9 <= len(SEQS) <= 12
    assert {s.table.groups for s in SEQS} == {1000, 200000} and sum(s.table.skew for s in SEQS) == 1
    for s in SEQS:
        assert (8 <= len(s.queries) <= 14) and (s.table.groups == 1000 or len(s.queries) <= 8 or s.table.skew), s.line
    for s in (SEQS[0], SEQS[5], SEQS[6]):
        c, valid = s.table.columns()
        whole = s.table.whole()
        assert whole.num_rows == ROWS and whole.schema == SCHEMA
        lens = s.table.batch_lengths()
        assert len(lens) == 3 and sum(lens) == ROWS and all(n % 64 for n in lens)
        bs = s.table.batches()
        assert [b.num_rows for b in bs] == lens and bs[1].column(0).offset != 0 and bs[2].column(0).offset != 0
        assert pa.Table.from_batches(bs).combine_chunks().to_batches()[0].equals(whole)
        # kw: wide keys in the last window only; every special value; the narrow edges of the image beside them
        kw = c["kw"]
        wide = (kw < 0) | (kw >= 2 ** 32)
        assert wide.sum() >= 8 and not wide[:4 * W].any()
        for special in (-(2 ** 63), 2 ** 32, 0, 2 ** 32 - 1):
            assert (kw[4 * W:] == special).any(), special
        assert (c["k"] >= 0).all() and (c["k"] < s.table.groups).all() and (c["k2"] < 3000).all()
        # nulls: about a tenth of kn and vn, nowhere else
        for name in COLUMNS:
            nulls = whole.column(COLUMNS.index(name)).null_count
            assert (0.08 * ROWS < nulls < 0.12 * ROWS) if name in ("kn", "vn") else nulls == 0, name
        # v, vn, p are their own float32; x is not
        for name in ("v", "vn", "p"):
            assert (c[name].astype(np.float32).astype(np.float64) == c[name]).all(), name
            assert (c[name] * 1024 == np.round(c[name] * 1024)).all() and c[name].max() < 1024
        assert (c["x"].astype(np.float32).astype(np.float64) != c["x"]).any()
        # every sum stays below 2^53 units (of 2^-10 for v, v * 2 + 1, vn and p; of 2^-20 for x): exact in any order
        assert float(np.abs(c["v"] * 2 + 1).sum()) * 2 ** 10 < 2 ** 53 and float(c["x"].sum()) * 2 ** 20 < 2 ** 53
        assert (c["x"] * 2 ** 20 == np.round(c["x"] * 2 ** 20)).all()
        # rows on both thresholds in every window, the tail included
        for name in ("v", "vn", "p", "x"):
            for w0 in range(0, ROWS, W):
                win = c[name][w0:w0 + W]
                assert (win == LO).any() and (win == HI).any(), (name, w0)
        assert (np.abs(c["w"].astype(np.float64)) > 2.0 ** 62).mean() > 0.4  # (full range: a group of a few rows already wraps)
    skewed = SEQS[6].table.columns()[0]["k"]
    assert np.bincount(skewed).max() > 0.5 * ROWS and SEQS[6].refused_pairs == (("k", "v"),) and SEQS[6].build_point is None


def test_every_family_occurs():
    tags = {}
    for s in SEQS:
        for q in s.queries:
            for t in q.tags:
                tags[t] = tags.get(t, 0) + 1
    want = ["key:" + k for k in KEYS] + ["aggs:" + a for a in AGG_SETS] + ["pred:" + p for p in PRED_FAMILIES] + ["batch:" + b for b in BATCH_WIDTHS]
    want += ["range:" + r for r in RANGES] + ["merge:0", "merge:1", "off-grid", "strategy:forced", "strategy:default"]
    want += ["agg.%s=%d" % (o, v) for o in ("routed_shadow", "key_shadow", "value_shadow") for v in (-1, 0, 1)]
    want += ["agg.routed_row8=-1", "agg.routed_row8=0", "agg.capacity_log2=0", "agg.capacity_log2=14", "agg.partition_defer=0", "agg.partition_defer=1", "agg.partition_defer=4"]
    missing = [t for t in want if t not in tags]
    assert not missing, missing
    assert tags["strategy:forced"] > 4 * tags["strategy:default"] >= 12
    # the headline is SELECT k, SUM(v) WHERE 204.8 < v < 409.6 GROUP BY k; every sequence asks it, and asks something else
    for s in SEQS:
        heads = [q for q in s.queries if (q.key, q.agg_set, q.pred_family) == ("k", "sum_v", "head")]
        assert heads and len(heads) < len(s.queries), s.line
    # every sequence that builds has at least three queries after the build point that are not eligible for the routed scan, and one that is
    for s in SEQS:
        if s.build_point is None:
            assert s.refused_pairs, s.line
            continue
        after = s.queries[s.build_point + 1:]
        assert sum(1 for q in after if not s.eligible(q)) >= 3, s.line
        assert any(s.eligible(q) for q in after), s.line
    assert sum(1 for s in SEQS if s.build_point is not None) >= 8
    # the exact window count is asserted somewhere: pinned, eligible queries behind a build point; and every range is scanned by an eligible query
    pinned = [q for s in SEQS if s.build_point is not None for q in s.queries[s.build_point + 1:] if s.eligible(q) and q.pinned and q.capacity == 0]
    assert len(pinned) >= 15 and {q.range_name for q in pinned} >= {"whole", "W..3W", "W..end"}
    assert {q.range_name for s in SEQS for q in s.queries if s.eligible(q)} == set(RANGES)
    assert {q.grid_windows for q in QUERIES} == {5, 2, 4, 1}


def test_grid_windows_and_eligibility():
    from table_query_cases import Query
    assert Query().grid_windows == 5 and Query(rows="W..3W").grid_windows == 2 and Query(rows="W..end").grid_windows == 4
    assert Query(rows="off_grid").grid_windows == 1 and Query(rows="2W..3W+192").grid_windows == 1
    assert Query().routed_eligible() and Query(pred="none").routed_eligible() and Query(key="k2", pred="ge_le").routed_eligible()
    for kw in (dict(routed=0), dict(key_shadow=0), dict(value_shadow=0), dict(row8=0), dict(aggs="min_v"), dict(aggs="avg_v"), dict(aggs="sum_min_v"),
               dict(aggs="sum_affine"), dict(aggs="sum_key", pred="none"), dict(aggs="sum_w", pred="none"), dict(pred="p_range"), dict(aggs="sum_x"),
               dict(aggs="sum_vn"), dict(key="kw"), dict(key="kn"), dict(aggs="sum_x", pred="v_other"), dict(aggs="count_v")):
        assert not Query(**kw).routed_eligible(), kw
    assert not Query().routed_eligible(pair_refused=True)


def _oracle(whole, q):
    b, _n, n = q.row_range
    rows = whole.slice(b, n)
    fed = oracle.filter_next(q.pred, rows) if q.pred is not None else rows
    return oracle.aggregate(q.group, q.aggs, [fed])


@pytest.mark.parametrize("index", range(len(SEQS)), ids=[s.name for s in SEQS])
def test_oracle_agrees_with_numpy(index):
    s = SEQS[index]
    whole = s.table.whole()
    checked = 0
    for i, q in enumerate(s.queries):
        if q.nullable:
            continue
        want = numpy_truth(s.table, q)
        got = _oracle(whole, q)
        assert got.num_columns == want.num_columns == 1 + len(AGG_SETS[q.agg_set])
        assert_groups_identical(got, want, 1, "%s\nquery %d: %s" % (s.line, i, q.line))
        if q.pred_family == "nobody":
            assert got.num_rows == 0
        if q.pred_family in ("none", "everybody") and q.key in ("k", "k2") and s.table.groups == 1000 and not s.table.skew:
            assert got.num_rows == (1000 if q.key == "k" else 3000)
        checked += 1
    assert checked >= len(s.queries) // 2, s.line


def test_every_query_compiles_on_the_host():
    """every operator tree is built with its option set: expression compilation and option validation run without a device"""
    from datafusion_archive_amd import execution as ex
    one = pa.RecordBatch.from_arrays([pa.array([], f.type) for f in SCHEMA], schema=SCHEMA)
    for q in QUERIES:
        rel = ex.DataSourceRelation(SCHEMA, [one])
        if q.pred is not None:
            rel = ex.FilterRelation(rel, ex.compile_scalar_expr(None, q.pred, SCHEMA), SCHEMA)
        rel = ex.AggregateRelation(None, rel, [ex.compile_scalar_expr(None, g, SCHEMA) for g in q.group], [ex.compile_expr(None, a, SCHEMA) for a in q.aggs], q.options)
        assert "Aggregate" in ex.explain(rel).split("\n")[0], q.line
