"""CPU tests of MIN / MAX of a Utf8 column (deviation D10): the names compile with a Utf8 argument, the operator tree they build (the
distinct-set tower of COUNT_DISTINCT, one set per argument column), the refusals returned at creation, and the Python restatement
the GPU tests compare with.  No compute calls here."""
import pyarrow as pa
import pytest

from datafusion_archive_amd import execution as ex
from datafusion_archive_amd.logicalplan import AggregateFunction, BinaryExpr, Cast, Column, DataType, Literal, Operator, ScalarValue
from utf8_minmax_truth import utf8_extrema

SCHEMA = pa.schema([("k", pa.int64()), ("v", pa.int64()), ("w", pa.float64()), ("s", pa.string()), ("t", pa.string())])
U8 = DataType.Utf8


def smin(c, t=U8):
    return AggregateFunction("MIN", [c if not isinstance(c, int) else Column(c)], t)


def smax(c, t=U8):
    return AggregateFunction("MAX", [c if not isinstance(c, int) else Column(c)], t)


def _agg(group, aggs, schema=SCHEMA, filter_expr=None, options=None):
    batch = pa.RecordBatch.from_pydict({f.name: pa.array([], f.type) for f in schema}, schema=schema)
    rel = ex.DataSourceRelation(schema, [batch])
    if filter_expr is not None:
        rel = ex.FilterRelation(rel, ex.compile_scalar_expr(None, filter_expr, schema), schema)
    return ex.AggregateRelation(None, rel, [ex.compile_scalar_expr(None, g, schema) for g in group],
                                [ex.compile_expr(None, a, schema) for a in aggs], options)


def test_compile_expr_accepts_min_and_max_of_a_utf8_column():
    for name in ("min", "MAX", "Min"):
        e = ex.compile_expr(None, AggregateFunction(name, [Column(3)], U8), SCHEMA)
        assert e.is_aggregate() and e.get_name() == name and e.get_type() == U8


def test_the_operator_builds_without_a_device_and_types_its_columns():
    aggs = [AggregateFunction("SUM", [Column(1)], DataType.Int64), smin(3), smax(3), AggregateFunction("COUNT_DISTINCT", [Column(3)], DataType.UInt64),
            smax(4)]
    for group, kw in (([Column(0)], 1), ([], 0), ([Column(4), Column(0)], 2)):
        s = _agg(group, aggs).schema()
        assert [f.name for f in s][kw:] == ["SUM", "MIN", "MAX", "COUNT_DISTINCT", "MAX"]
        assert [f.type for f in s][kw:] == [pa.int64(), pa.string(), pa.string(), pa.uint64(), pa.string()]
        assert all(f.nullable for f in list(s)[kw + 1:kw + 3])


def test_explain_names_the_extrema_beside_the_set_they_read():
    cd = AggregateFunction("COUNT_DISTINCT", [Column(3)], DataType.UInt64)
    lines = ex.explain(_agg([Column(0)], [cd, smin(3), smax(3)])).splitlines()
    assert lines[0].startswith("DistinctAggregate: 1 COUNT_DISTINCT + Utf8 MIN/MAX set of 2-word tuples"), lines  # one shared set, one dictionary
    assert "set 0 of #3 read by COUNT_DISTINCT MIN MAX" in lines[0] and "k_utf8_extrema_fold" in lines[0], lines
    assert "1 Utf8 columns dictionary-encoded" in lines[0], lines
    assert lines[1].startswith("  Aggregate: 1 keys, 0 accumulators"), lines  # the inner aggregate has no aggregates: it keeps the groups
    only = ex.explain(_agg([], [smin(3), smax(4), smin(4)])).splitlines()
    assert only[0].startswith("DistinctAggregate: 2 Utf8 MIN/MAX sets of 1-word tuples"), only
    assert "set 0 of #3 read by MIN, set 1 of #4 read by MIN MAX" in only[0], only
    assert only[1].startswith("  Aggregate: 0 keys"), only
    six = ex.explain(_agg([Column(0), Column(1), Column(0), Column(1), Column(0), Column(1)], [smax(3)])).splitlines()
    assert six[0].startswith("DistinctAggregate: 1 Utf8 MIN/MAX set of 8-word tuples (group keys + argument, keys padded to 7 words)"), six
    pred = BinaryExpr(Column(1), Operator.Gt, Literal(ScalarValue.Int64(3)))
    filtered = ex.explain(_agg([Column(0)], [smin(3)], filter_expr=pred)).splitlines()
    assert [ln.strip().split(":")[0] for ln in filtered[:3]] == ["DistinctAggregate", "Aggregate", "Filter"], filtered
    # COUNT_DISTINCT alone keeps its words, numeric MIN / MAX stay with the plain aggregate
    assert ex.explain(_agg([Column(0)], [cd])).startswith("DistinctAggregate: 1 COUNT_DISTINCT set of 2-word tuples")
    assert ex.explain(_agg([Column(0)], [AggregateFunction("MIN", [Column(1)], DataType.Int64)])).startswith("Aggregate: 1 keys")


def test_refusals_are_returned_at_creation():
    # A Utf8 argument that is not a bare column.  The compiler types no such expression yet (a cast to Utf8 is its NotImplemented, a
    # Utf8 literal outside a string term its ExecutionError), so the operator's own check of the same thing is out of a test's reach.
    for name in ("MIN", "MAX", "COUNT_DISTINCT"):
        with pytest.raises(ex.ExecutionError) as ei:
            _agg([Column(0)], [AggregateFunction(name, [Cast(Column(1), U8)], U8)])
        assert ei.value.kind == "NotImplemented", name
    with pytest.raises(ex.ExecutionError) as ei:
        _agg([Column(0)], [smin(Literal(ScalarValue.Utf8("x")))])
    assert ei.value.kind == "ExecutionError"
    # a declared return type other than Utf8: the InternalError of a numeric mismatch (there: argument Int64, declared Float64)
    with pytest.raises(ex.ExecutionError) as ei:
        _agg([Column(0)], [smax(3, DataType.Int64)])
    assert ei.value.kind == "InternalError"
    assert ei.value.message == "called `Option::unwrap()` on a `None` value (aggregate argument is Utf8, declared Int64)"
    # more GROUP BY expressions than COUNT_DISTINCT takes: its limit, its wording
    schema = pa.schema([(f"k{i}", pa.int32()) for i in range(8)] + [("s", pa.string())])
    with pytest.raises(ex.ExecutionError) as ei:
        _agg([Column(i) for i in range(8)], [smin(8)], schema=schema)
    with pytest.raises(ex.ExecutionError) as cd:
        _agg([Column(i) for i in range(8)], [AggregateFunction("COUNT_DISTINCT", [Column(8)], DataType.UInt64)], schema=schema)
    assert ei.value.kind == cd.value.kind == "NotImplemented"
    assert ei.value.message.startswith("MIN/MAX of Utf8 with more than 7 GROUP BY expressions")
    assert ei.value.message.split(" with ", 1)[1] == cd.value.message.split(" with ", 1)[1]
    _agg([Column(i) for i in range(7)], [smin(8), smax(8)], schema=schema)  # seven keys + the argument: eight words


def test_the_python_restatement_orders_like_rust_str():
    vals = ["b", "", None, "ab", "abc", "é", "z", "a" * 8 + "b", "a" * 8 + "a", None]
    assert utf8_extrema([], vals) == {(): (b"", "é".encode())}  # the empty string is the smallest, 0xC3 sorts after 'z'
    assert utf8_extrema([], ["ab", "abc", "abd"]) == {(): (b"ab", b"abd")}  # a proper prefix first
    assert utf8_extrema([[1, 1, 2, 3], ["x", "x", "y", "z"]], ["q", None, None, ""]) == {(1, "x"): (b"q", b"q"), (2, "y"): (None, None), (3, "z"): (b"", b"")}
    assert utf8_extrema([], []) == {(): (None, None)} and utf8_extrema([[]], []) == {}
