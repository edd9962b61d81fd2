"""CPU tests of COUNT(DISTINCT x) (deviation D8): the name compiles, the operator tree it builds, the limits it returns at creation
and its option.  No compute calls here."""
import pyarrow as pa
import pytest

from datafusion_archive_amd import execution as ex
from datafusion_archive_amd.logicalplan import AggregateFunction, BinaryExpr, Column, DataType, Literal, Operator, ScalarValue

SCHEMA = pa.schema([("k", pa.int64()), ("v", pa.int64()), ("w", pa.float64()), ("s", pa.string())])


def _source(schema=SCHEMA):
    batch = pa.RecordBatch.from_pydict({f.name: pa.array([], f.type) for f in schema}, schema=schema)
    return ex.DataSourceRelation(schema, [batch])


def _agg(group, aggs, schema=SCHEMA, filter_expr=None, options=None):
    rel = _source(schema)
    if filter_expr is not None:
        rel = ex.FilterRelation(rel, ex.compile_scalar_expr(None, filter_expr, schema), schema)
    return ex.AggregateRelation(None, rel, [ex.compile_scalar_expr(None, g, schema) for g in group],
                                [ex.compile_expr(None, a, schema) for a in aggs], options)


def test_compile_expr_accepts_count_distinct():
    for name in ("count_distinct", "COUNT_DISTINCT", "Count_Distinct"):
        e = ex.compile_expr(None, AggregateFunction(name, [Column(1)], DataType.UInt64), SCHEMA)
        assert e.is_aggregate() and e.get_name() == name and e.get_type() == DataType.UInt64
    with pytest.raises(ex.ExecutionError) as want:  # exactly as COUNT: assert_eq!(1, args.len())
        ex.compile_expr(None, AggregateFunction("count", [Column(1), Column(2)], DataType.UInt64), SCHEMA)
    with pytest.raises(ex.ExecutionError) as got:
        ex.compile_expr(None, AggregateFunction("count_distinct", [Column(1), Column(2)], DataType.UInt64), SCHEMA)
    assert (got.value.kind, got.value.message) == (want.value.kind, want.value.message) == ("InternalError", want.value.message)


def test_explain_shows_the_distinct_side_and_the_inner_aggregate():
    cd = AggregateFunction("COUNT_DISTINCT", [Column(1)], DataType.UInt64)
    lines = ex.explain(_agg([Column(0)], [AggregateFunction("SUM", [Column(2)], DataType.Float64), cd])).splitlines()
    assert lines[0].startswith("DistinctAggregate: 1 COUNT_DISTINCT set of 2-word tuples"), lines
    assert "k_distinct_insert" in lines[0], lines
    assert lines[1].startswith("  Aggregate: 1 keys, 1 accumulators"), lines
    ungrouped = ex.explain(_agg([], [cd, AggregateFunction("count_distinct", [Column(1)], DataType.UInt64)])).splitlines()
    assert ungrouped[0].startswith("DistinctAggregate: 1 COUNT_DISTINCT set of 1-word tuples"), ungrouped  # one shared set
    assert ungrouped[1].startswith("  Aggregate: 0 keys"), ungrouped
    pred = BinaryExpr(Column(1), Operator.Gt, Literal(ScalarValue.Int64(3)))
    filtered = ex.explain(_agg([Column(0)], [cd], filter_expr=pred)).splitlines()
    assert [ln.strip().split(":")[0] for ln in filtered[:3]] == ["DistinctAggregate", "Aggregate", "Filter"], filtered
    assert "compacted by FilterRelation" in filtered[0]
    text = ex.explain(_agg([Column(3)], [AggregateFunction("COUNT_DISTINCT", [Column(3)], DataType.UInt64)]))
    assert "Utf8 columns dictionary-encoded" in text.splitlines()[0], text


def test_output_schema_keeps_the_order_and_the_names():
    aggs = [AggregateFunction("SUM", [Column(1)], DataType.Int64), AggregateFunction("COUNT_DISTINCT", [Column(2)], DataType.UInt64),
            AggregateFunction("AVG", [Column(2)], DataType.Float64), AggregateFunction("COUNT_DISTINCT", [Column(1)], DataType.UInt64)]
    s = _agg([Column(0)], aggs).schema()
    assert [f.name for f in s] == ["k", "SUM", "COUNT_DISTINCT", "AVG", "COUNT_DISTINCT"]
    assert [f.type for f in s] == [pa.int64(), pa.int64(), pa.uint64(), pa.float64(), pa.uint64()]


def test_eight_key_words_with_a_distinct_aggregate_is_not_implemented_at_creation():
    schema = pa.schema([(f"k{i}", pa.int32()) for i in range(8)] + [("v", pa.int64())])
    cd = AggregateFunction("COUNT_DISTINCT", [Column(8)], DataType.UInt64)
    with pytest.raises(ex.ExecutionError) as ei:
        _agg([Column(i) for i in range(8)], [cd], schema=schema)
    assert ei.value.kind == "NotImplemented" and "COUNT_DISTINCT" in ei.value.message
    _agg([Column(i) for i in range(7)], [cd], schema=schema)  # seven keys + the argument: eight words
    _agg([Column(i) for i in range(8)], [AggregateFunction("COUNT", [Column(8)], DataType.UInt64)], schema=schema)  # plain: unchanged


def test_distinct_capacity_option_is_per_operator():
    cd = AggregateFunction("COUNT_DISTINCT", [Column(1)], DataType.UInt64)
    _agg([Column(0)], [cd], options={"agg.distinct_capacity_log2": 9})
    with pytest.raises(ex.ExecutionError):
        _agg([Column(0)], [cd], options={"agg.distinct_capacity_lg": 9})
    # process-wide as well, next to agg.capacity_log2
    ex.set_option("agg.distinct_capacity_log2", 0)
