"""GPU tests of the CSV writer (deviation D11: dfx_csv_write, the executor of PhysicalPlan::Write that the reference never had).
The truth has two independent parts: the Python restatement of the format (csv_write_truth.py) applied to the whole input gives
the expected file BYTES, and the library's own reader (dfx_csv_datasource_new) must give the input back bit for bit -- apart
from the documented exceptions, which the comparison applies explicitly: a null Utf8 slot returns as the empty string, every
NaN payload returns as one NaN."""
import os
import random
import sys

import numpy as np
import pyarrow as pa
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import csv_write_truth as truth  # noqa: E402
import fixtures  # noqa: E402
from gpu_util import bits  # noqa: E402

from datafusion_archive_amd import execution as ex  # noqa: E402
from datafusion_archive_amd.logicalplan import (AggregateFunction, BinaryExpr, Column, DataType, Literal, Operator,  # noqa: E402
                                                ScalarValue)

pytestmark = pytest.mark.gpu
DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")

ALL_TYPES = pa.schema([("c_bool", pa.bool_()), ("c_int8", pa.int8()), ("c_int16", pa.int16()), ("c_int32", pa.int32()), ("c_int64", pa.int64()),
                       ("c_uint8", pa.uint8()), ("c_uint16", pa.uint16()), ("c_uint32", pa.uint32()), ("c_uint64", pa.uint64()),
                       ("c_float32", pa.float32()), ("c_float64", pa.float64()), ("c_utf8", pa.string())])
INT_RANGE = {pa.int8(): (-2 ** 7, 2 ** 7 - 1), pa.int16(): (-2 ** 15, 2 ** 15 - 1), pa.int32(): (-2 ** 31, 2 ** 31 - 1), pa.int64(): (-2 ** 63, 2 ** 63 - 1),
             pa.uint8(): (0, 2 ** 8 - 1), pa.uint16(): (0, 2 ** 16 - 1), pa.uint32(): (0, 2 ** 32 - 1), pa.uint64(): (0, 2 ** 64 - 1)}
WORDS = ["", "a", "plain", "a,b", 'say "hi"', "line\nbreak", "cr\rhere", '"', '""', "grüß dich", "漢字, \"quoted\"\r\n", " spaced ", "x" * 40]


def random_string(rng):
    if rng.random() < 0.5:
        return rng.choice(WORDS)
    return "".join(rng.choice(["a", "b", "Z", " ", ",", '"', "\r", "\n", "é", "漢"]) for _ in range(rng.randrange(0, 14)))[:40]


def all_types_batch(n, seed, utf8_nulls=False):
    """n rows of all twelve types, nulls in every primitive column, the extremes of every type among the values"""
    rng = random.Random(seed)
    f64s, f32s = truth.special_f64_bits(), truth.special_f32_bits()
    null = lambda: rng.random() < 0.15
    cols = []
    for f in ALL_TYPES:
        if pa.types.is_boolean(f.type):
            vals = [None if null() else rng.random() < 0.5 for _ in range(n)]
        elif f.type in INT_RANGE:
            lo, hi = INT_RANGE[f.type]
            vals = [None if null() else rng.choice([lo, hi, 0, rng.randint(lo, hi), rng.randint(-99, 99) if lo < 0 else rng.randint(0, 99)]) for _ in range(n)]
        elif f.type == pa.float64():
            raw = np.array([rng.choice(f64s) if rng.random() < 0.3 else rng.getrandbits(64) for _ in range(n)], dtype=np.uint64).view(np.float64)
            cols.append(pa.array(raw, mask=np.array([null() for _ in range(n)], dtype=bool)))
            continue
        elif f.type == pa.float32():
            raw = np.array([rng.choice(f32s) if rng.random() < 0.3 else rng.getrandbits(32) for _ in range(n)], dtype=np.uint32).view(np.float32)
            cols.append(pa.array(raw, mask=np.array([null() for _ in range(n)], dtype=bool)))
            continue
        else:
            vals = [None if (utf8_nulls and null()) else random_string(rng) for _ in range(n)]
        cols.append(pa.array(vals, f.type))
    return pa.RecordBatch.from_arrays(cols, schema=ALL_TYPES)


def canonical(arr):
    """a column as comparable values with the round trip's exceptions applied: Utf8 null -> "", every NaN -> one NaN"""
    if isinstance(arr, pa.ChunkedArray):
        arr = arr.combine_chunks()
    if pa.types.is_string(arr.type):
        return ["" if v is None else v for v in arr.to_pylist()]
    if pa.types.is_floating(arr.type):
        vals = arr.fill_null(0).to_numpy(zero_copy_only=False)
        nan = np.isnan(vals).tolist()
        return [None if b is None else ("NaN" if is_nan else b) for b, is_nan in zip(bits(arr), nan)]
    return arr.to_pylist()


def read_back(path, schema):
    got = list(ex.CsvDataSource(path, schema, 1 << 20))
    return pa.Table.from_batches(got, schema=got[0].schema if got else schema)


def assert_round_trip(path, schema, batches):
    got = read_back(path, schema)
    want = pa.Table.from_batches(batches, schema=schema)
    assert got.num_rows == want.num_rows
    for i, f in enumerate(schema):
        g, w = canonical(got.column(i)), canonical(want.column(i))
        if g != w:
            bad = [j for j, (a, b) in enumerate(zip(g, w)) if a != b]
            raise AssertionError(f"column {f.name}: {len(bad)} rows differ after the round trip, first at {bad[0]}: {g[bad[0]]!r} != {w[bad[0]]!r}")


def write_and_check(tmp_path, schema, batches, relation=None, name="out.csv"):
    """writes `relation` (default: the batches as a host stream), compares the file with the restatement; returns the path"""
    path = str(tmp_path / name)
    rel = relation if relation is not None else ex.DataSourceRelation(schema, batches)
    rows, nbytes = ex.write_csv(rel, path)
    want = truth.expected_file(schema, batches)
    got = open(path, "rb").read()
    assert rows == sum(b.num_rows for b in batches)
    assert nbytes == len(got)
    if got != want:
        at = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError(f"file differs from the restatement at byte {at} of {len(got)} / {len(want)}: {got[max(0, at - 40):at + 40]!r} != {want[max(0, at - 40):at + 40]!r}")
    assert not os.path.exists(path + ".dfx-partial")  # renamed, nothing partial is left
    return path


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1000])
def test_all_types_bytes_and_round_trip(tmp_path, n):
    """the tile edges; nulls in every primitive column and (second file) in the Utf8 column too"""
    for k, utf8_nulls in enumerate((False, True)):
        b = all_types_batch(n, 100 + n, utf8_nulls)
        path = write_and_check(tmp_path, ALL_TYPES, [b], name=f"t{k}.csv")
        assert_round_trip(path, ALL_TYPES, [b])


def test_counters(tmp_path):
    ex.counter_reset()
    b = all_types_batch(130, 7)
    path = write_and_check(tmp_path, ALL_TYPES, [b])  # (short Utf8 cells: every tile fits the LDS window)
    assert ex.counter_get("csv_write_cells") == 130 * 12
    assert ex.counter_get("csv_write_bytes") == os.path.getsize(path)
    assert ex.counter_get("csv_write_general_tiles") == 0


def test_float_columns(tmp_path):
    """2^16 random bit patterns plus the special list, one column each: bytes by the restatement, bits by the reader"""
    rng = random.Random(21)
    f64 = np.array(truth.special_f64_bits() + [rng.getrandbits(64) for _ in range(1 << 16)], dtype=np.uint64).view(np.float64)
    f32 = np.array(truth.special_f32_bits() + [rng.getrandbits(32) for _ in range(1 << 16)], dtype=np.uint32).view(np.float32)
    for name, arr in (("d", pa.array(f64)), ("f", pa.array(f32))):
        schema = pa.schema([pa.field(name, arr.type)])
        b = pa.RecordBatch.from_arrays([arr], schema=schema)
        path = write_and_check(tmp_path, schema, [b], name=name + ".csv")
        assert_round_trip(path, schema, [b])


def test_utf8_cells_and_the_general_path(tmp_path):
    rng = random.Random(31)
    schema = pa.schema([pa.field("id", pa.int32()), pa.field("s", pa.string()), pa.field("t", pa.string())])
    n = 64 * 6
    s = [random_string(rng) for _ in range(n)]
    t = [random_string(rng) for _ in range(n)]
    big = ("0123456789,\"q\"\r\n" * 1300)[:20000]  # 20 kB with every special byte, in the middle of tile 2
    s[64 * 2 + 31] = big
    t[64 * 2 + 31] = "after the long one"
    for i in range(64 * 4, 64 * 5):  # a tile of only empty strings
        s[i], t[i] = "", ""
    b = pa.RecordBatch.from_arrays([pa.array(range(n), pa.int32()), pa.array(s), pa.array(t)], schema=schema)
    ex.counter_reset()
    path = write_and_check(tmp_path, schema, [b])
    assert ex.counter_get("csv_write_general_tiles") == 1  # the tile with the long string, and only that one
    assert_round_trip(path, schema, [b])


def test_single_column_files(tmp_path):
    """the reader skips blank lines: an empty cell of a one-column file is written "" -- the empty string, a null string (which
    returns as the empty string) and a null Int32 (which returns as a null: the reader turns "" of a primitive column into one)"""
    us = pa.schema([pa.field("s", pa.string())])
    b = pa.RecordBatch.from_arrays([pa.array(["", "a", None, "", 'q"', "", "z"] * 20)], schema=us)
    path = write_and_check(tmp_path, us, [b], name="s.csv")
    assert open(path, "rb").read().startswith(b's\n""\na\n""\n""\n"q"""\n')
    assert_round_trip(path, us, [b])
    ns = pa.schema([pa.field("v", pa.int32())])
    b = pa.RecordBatch.from_arrays([pa.array([None, 1, None, -5, None] * 30, pa.int32())], schema=ns)
    path = write_and_check(tmp_path, ns, [b], name="n.csv")
    assert open(path, "rb").read().startswith(b'v\n""\n1\n""\n-5\n')
    assert_round_trip(path, ns, [b])


def test_multi_batch_and_sliced_inputs(tmp_path):
    n = (1 << 12) + 5
    batches = [all_types_batch(n, 40 + i) for i in range(3)]
    path = write_and_check(tmp_path, ALL_TYPES, batches, name="host.csv")  # a foreign (host) stream of 3 batches
    assert_round_trip(path, ALL_TYPES, batches)
    table = ex.DeviceTable.from_batches(ALL_TYPES, batches)
    write_and_check(tmp_path, ALL_TYPES, batches, relation=table.scan(1000), name="scan.csv")  # resident, in batches of 1000 rows
    whole = pa.Table.from_batches(batches)
    for begin, rows in ((64, 200), (4096 + 64, -1), (128, 64 * 3 + 1)):  # slices: Arrow offsets in every buffer and bitmap
        want = whole.slice(begin, None if rows < 0 else rows).combine_chunks().to_batches()
        write_and_check(tmp_path, ALL_TYPES, want, relation=table.scan(0, begin, rows), name=f"slice{begin}.csv")


def test_more_rows_than_one_launch(tmp_path):
    """batches beyond the writer's internal row limit (2^20) are split"""
    n = (1 << 20) + 77
    schema = pa.schema([pa.field("v", pa.int32()), pa.field("b", pa.bool_())])
    v = np.arange(n, dtype=np.int32) * 2047 - (1 << 30)
    bl = (np.arange(n) % 3) == 0
    b = pa.RecordBatch.from_arrays([pa.array(v), pa.array(bl)], schema=schema)
    path = str(tmp_path / "big.csv")
    assert ex.write_csv(ex.DataSourceRelation(schema, [b]), path)[0] == n
    want = b"v,b\n" + "".join(f"{x},{'true' if y else 'false'}\n" for x, y in zip(v.tolist(), bl.tolist())).encode()
    assert open(path, "rb").read() == want


def _cities():
    schema = fixtures.uk_cities_schema()
    return schema, lambda: ex.CsvDataSource(os.path.join(DATA, "uk_cities.csv"), schema, 1024)


def test_operator_outputs(tmp_path):
    """what Filter, Aggregate (Utf8 key) and Sort + Limit hand on is written as the restatement writes the batches they return
    (eleven types: FilterRelation, like the reference's fn filter, takes no Boolean column)"""
    schema = pa.schema(list(ALL_TYPES)[1:])
    batches = [pa.RecordBatch.from_arrays(b.columns[1:], schema=schema) for b in (all_types_batch(3000, 60 + i) for i in range(2))]
    i32, i64, f64, utf8 = (schema.get_field_index(n) for n in ("c_int32", "c_int64", "c_float64", "c_utf8"))
    table = ex.DeviceTable.from_batches(schema, batches)
    pred = BinaryExpr(Column(i32), Operator.Gt, Literal(ScalarValue.Int32(0)))
    flt = lambda: ex.FilterRelation(table.scan(1024), ex.compile_scalar_expr(None, pred, schema), schema)
    want = list(flt())
    assert 0 < sum(b.num_rows for b in want) < 6000
    write_and_check(tmp_path, schema, want, relation=flt(), name="filter.csv")

    srt = lambda: ex.LimitRelation(ex.SortRelation(table.scan(1024), [(ex.compile_scalar_expr(None, Column(f64), schema), False)], schema), 777, schema)
    want = list(srt())
    assert sum(b.num_rows for b in want) == 777
    write_and_check(tmp_path, schema, want, relation=srt(), name="sort.csv")

    agg = lambda: ex.AggregateRelation(None, table.scan(1024), [ex.compile_scalar_expr(None, Column(utf8), schema)],
                                       [ex.compile_expr(None, AggregateFunction("MAX", [Column(f64)], DataType.Float64), schema),
                                        ex.compile_expr(None, AggregateFunction("COUNT", [Column(i64)], DataType.UInt64), schema)])
    rel = agg()
    out_schema = rel.schema()
    want = list(rel)
    path = str(tmp_path / "agg.csv")
    rows, _ = ex.write_csv(agg(), path)
    assert rows == sum(b.num_rows for b in want) > 10
    # (two runs of a hash aggregate may emit their groups in different orders: the records are compared as a multiset, the
    # header in place; every record is still the restatement's, byte for byte.  No key holds a line break unquoted: records
    # are split where the restatement's are)
    expect = [truth.expected_file(out_schema, [b.slice(i, 1)]) for b in want for i in range(b.num_rows)]
    header = truth.expected_file(out_schema, [])
    got = open(path, "rb").read()
    assert got.startswith(header) and len(got) == len(header) + sum(len(r) - len(header) for r in expect)
    rest = got[len(header):]
    for rec in sorted((r[len(header):] for r in expect), key=len, reverse=True):
        assert rec in rest, rec
        rest = rest.replace(rec, b"", 1)
    assert rest == b""


def test_end_to_end_csv_filter_write_read(tmp_path):
    """uk_cities.csv -> Filter (lat > 51) -> write_csv -> read back == the filter's own output"""
    schema, src = _cities()
    pred = ex.compile_scalar_expr(None, BinaryExpr(Column(1), Operator.Gt, Literal(ScalarValue.Float64(51.0))), schema)
    want = list(ex.FilterRelation(src(), pred, schema))
    path = write_and_check(tmp_path, schema, want, relation=ex.FilterRelation(src(), pred, schema))
    assert 0 < sum(b.num_rows for b in want) < 36
    got = read_back(path, schema)
    assert got.num_rows == sum(b.num_rows for b in want)
    for i in range(len(schema)):
        assert bits(got.column(i)) == bits(pa.Table.from_batches(want).column(i))


def test_errors(tmp_path):
    schema = pa.schema([pa.field("a,b", pa.int32()), pa.field('q"', pa.string()), pa.field("plain", pa.float64())])
    b = pa.RecordBatch.from_arrays([pa.array([1], pa.int32()), pa.array(["x"]), pa.array([0.5])], schema=schema)
    path = write_and_check(tmp_path, schema, [b], name="names.csv")
    assert open(path, "rb").read() == b'"a,b","q""",plain\n1,x,0.5\n'
    missing = tmp_path / "no" / "such" / "dir" / "o.csv"
    with pytest.raises(ex.ExecutionError) as ei:
        ex.write_csv(ex.DataSourceRelation(schema, [b]), str(missing))
    assert ei.value.kind == "IoError"
    assert not missing.exists() and not (tmp_path / "no").exists()
    ro = tmp_path / "ro"
    ro.mkdir()
    os.chmod(ro, 0o500)
    try:
        if not os.access(ro, os.W_OK):  # (root writes anywhere: the missing directory above is the case that always holds)
            with pytest.raises(ex.ExecutionError) as ei:
                ex.write_csv(ex.DataSourceRelation(schema, [b]), str(ro / "o.csv"))
            assert ei.value.kind == "IoError" and os.listdir(ro) == []
    finally:
        os.chmod(ro, 0o700)
