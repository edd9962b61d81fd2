"""CPU side of the state-machine fuzz (tests/agg_stream_cases.py, tests/test_gpu_agg_state_machine.py): the generator is
deterministic and covers every family it promises, the oracle agrees bit for bit with an independent numpy truth on every case
(numpy adds in another order than the oracle: equal bits prove that the values are exact), and every case compiles on the host
with its options -- so "no case is skipped" holds as far as a machine without a GPU can tell.

The streams run at 1/16 of their rows here (same phases, same group counts): this file validates the generator and the
reference; whether a group count sits on the promised side of a threshold is asserted at full size by the GPU module."""
import numpy as np
import pyarrow as pa
import pytest

import oracle
from agg_stream_cases import AGG_SETS, OPTION_POOL, THRESHOLDS, cases, concat_filtered, distinct_truth, group_ids
from datafusion_archive_amd import execution as ex
from gpu_util import assert_groups_identical

SEED = 0xA66
SCALE = 1.0 / 16
CASES = cases(SEED, SCALE)


def test_cases_are_deterministic():
    again = cases(SEED, SCALE)
    assert [c.line for c in CASES] == [c.line for c in again]
    assert len({c.line for c in CASES}) == len(CASES)
    for a, b in list(zip(CASES, again))[::5]:
        for x, y in zip(a.batches(), b.batches()):
            assert x.equals(y) and x.schema == y.schema
    assert cases(SEED + 1, SCALE)[0].batches()[0] != CASES[0].batches()[0]


def test_every_family_occurs():
    tags = {}
    for c in CASES:
        for t in c.tags:
            tags.setdefault(t, []).append(c.index)
    want = ["change@slice", "change@batch", "narrow->wide@slice", "narrow->wide@batch", "uniform->skew", "skew->uniform",
            "selective->dense", "dense->selective", "nulls@batch2", "nulls@batch3", "nulls-under-predicate", "empty:first", "empty:middle",
            "empty:last", "first:big", "first:small", "keys:i64", "keys:two", "keys:utf8", "pred:none", "pred:v", "pred:p", "resident",
            "crosses:16384:many->few"]
    want += ["crosses:%d:few->many" % t for t in THRESHOLDS]
    want += ["aggs:" + s for s in AGG_SETS]
    want += ["opt:" + k for k, _v in OPTION_POOL] + ["opt:agg.distinct_capacity_log2", "opt:agg.dict_capacity_log2"]
    missing = [t for t in want if t not in tags]
    assert not missing, missing
    # a change behind the slice and one at a batch boundary each occur with a first batch that is large enough for a slice
    big = [c for c in CASES if c.first_big]
    assert 2 * len(big) > len(CASES) and len(big) < len(CASES)
    assert any("change@slice" in c.tags for c in big) and any("change@batch" in c.tags for c in big)
    # options come 2-3 together; about a quarter of the cases run the defaults
    defaults = len(tags.get("options:0", []))
    assert 0.15 * len(CASES) <= defaults <= 0.4 * len(CASES), defaults
    assert len(tags.get("options:2", [])) + len(tags.get("options:3", [])) >= 0.4 * len(CASES)
    pairs = {(a, b) for c in CASES for a in c.options for b in c.options if a < b}
    assert len(pairs) >= 20, sorted(pairs)
    # more than 8 accumulators in a few cases, a COUNT_DISTINCT beside plain aggregates in a few, minorities of two keys / Utf8 keys
    assert len(tags["aggs:chunks"]) >= 2 and len(tags["aggs:distinct"]) >= 2
    assert 2 <= len(tags["keys:two"]) < len(CASES) // 4 and 2 <= len(tags["keys:utf8"]) < len(CASES) // 4


def test_streams_have_the_promised_shape():
    for c in cases(SEED):  # full size: only the lengths are looked at (nothing is generated)
        rng = np.random.default_rng([c.seed, c.index])
        lens = c._lengths(rng)
        assert 3 <= len(lens) <= 6 and all(n % 64 for n in lens), c.line
        assert (lens[0] > (1 << 21)) == c.first_big, c.line
        assert (1 << 21) <= sum(lens) <= (1 << 23), (c.line, sum(lens))
    for c in CASES[::4]:
        bs = c.batches()
        assert any(b.num_rows and b.column(0).offset != 0 for b in bs), c.line
        assert ([b.num_rows for b in bs].count(0) == 1) == bool(c.empty), c.line
    wide = [c for c in CASES if any(p[0] == "wide" for p in c.keys) and c.key_kind == "i64"]
    for c in wide[:3]:
        k = np.concatenate([b.column(0).to_numpy() for b in c.batches()])
        for special in (-(2 ** 63), 0, 2 ** 32 - 1, 2 ** 32):
            assert (k == special).any(), (c.line, special)
        assert (k < 0).any() and (k >= 2 ** 32).any()


def numpy_truth(case, batches):
    """the result of the plain aggregates as a RecordBatch, by np.unique / np.add.at / np.minimum.at"""
    vals, valid = concat_filtered(case, batches)
    g, inv, keys = group_ids(case, vals)
    cols = [pa.array(k, pa.string() if case.key_kind == "utf8" else pa.int64()) for k in keys]
    for f, c in AGG_SETS[case.agg_set]:
        if f == "COUNT_DISTINCT":
            continue
        # the reference's grouped accumulators read value(row) without a null check (aggregate.rs:548-612): SUM, MIN and MAX take
        # whatever a null slot holds, only the counts (COUNT, and the divisor of AVG) look at the validity
        x, gi = vals[c], inv
        cnt = np.bincount(inv[valid[c]], minlength=g)
        if f == "COUNT":
            cols.append(pa.array(cnt.astype(np.uint64)))
            continue
        if f in ("SUM", "AVG"):
            acc = np.zeros(g, dtype=x.dtype)
            np.add.at(acc, gi, x)  # (Int64: wraps)
            if f == "AVG":
                acc = acc / np.maximum(cnt, 1)
        elif f == "MIN":
            acc = np.full(g, np.inf if x.dtype == np.float64 else np.iinfo(np.int64).max, dtype=x.dtype)
            np.minimum.at(acc, gi, x)
        else:
            acc = np.full(g, -np.inf if x.dtype == np.float64 else np.iinfo(np.int64).min, dtype=x.dtype)
            np.maximum.at(acc, gi, x)
        cols.append(pa.array(acc, mask=(cnt == 0) if f == "AVG" else None))
    return pa.RecordBatch.from_arrays(cols, names=["c%d" % i for i in range(len(cols))])


def oracle_result(case, batches):
    pred = case.pred
    fed = [oracle.filter_next(pred, b) for b in batches] if pred is not None else batches
    return oracle.aggregate(case.group, case.plain_aggs, fed)


@pytest.mark.parametrize("index", range(len(CASES)), ids=[c.name for c in CASES])
def test_oracle_agrees_with_numpy(index):
    case = CASES[index]
    batches = case.batches()
    want = numpy_truth(case, batches)
    got = oracle_result(case, batches)
    assert got.num_columns == want.num_columns
    assert_groups_identical(got, want, case.n_keys, case.line)
    for pos in case.distinct_positions:  # the numpy truth of COUNT_DISTINCT names the same groups
        assert len(distinct_truth(case, batches, AGG_SETS[case.agg_set][pos][1])) == want.num_rows


def test_every_case_compiles_on_the_host():
    """the operator tree of every case is built with its options and explained: expression compilation, option validation and the
    host-side choice of kernel families all run without a device (what only a device can refuse is left to the GPU module)"""
    for case in CASES:
        schema = case.schema
        one = pa.RecordBatch.from_arrays([pa.array([], f.type) for f in schema], schema=schema)
        rel = ex.DataSourceRelation(schema, [one])
        if case.pred is not None:
            rel = ex.FilterRelation(rel, ex.compile_scalar_expr(None, case.pred, schema), schema)
        rel = ex.AggregateRelation(None, rel, [ex.compile_scalar_expr(None, g, schema) for g in case.group],
                                   [ex.compile_expr(None, a, schema) for a in case.aggs], case.options or None)
        text = ex.explain(rel)
        assert "Aggregate" in text.split("\n")[0], (case.line, text)
