"""GPU tests of the Parquet writer's "dictionary" option (dfx_parquet_write, deviation D13; kernels: csrc/dfx_k_parquet_write_dict.hip).
Every file is held the three ways tests/test_gpu_parquet_write.py holds its files: pyarrow reads back the table that went in, bit for
bit, with the chunk metadata and every chunk's dictionary (pyarrow.compute.unique: first-occurrence order); the library's own source
(dfx_parquet_datasource_new) reads back the same table; and the file's BYTES equal what the sequential host encoder
(tests/native/parquet_dict_write_check.cpp over csrc/dfx_parquet_dict_enc.hpp) writes for the same batches and options.  The counters
are held against the rules restated in Python.  The one case without byte equality is the forced hash collision: the host encoder
knows no hash.  No test feeds a kernel damaged input or tries to trip a guard."""
import os
import sys

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fixtures  # noqa: E402
import parquet_dict_write_cases as D  # noqa: E402
import parquet_write_cases as W  # noqa: E402
from gpu_util import assert_groups_identical  # noqa: E402

from datafusion_archive_amd import execution as ex  # noqa: E402
from datafusion_archive_amd.logicalplan import AggregateFunction, BinaryExpr, Column, DataType, Literal, Operator, ScalarValue  # noqa: E402

pytestmark = pytest.mark.gpu
DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")
COUNTERS = ["parquet_write_pages", "parquet_write_bytes", "parquet_write_row_groups", "parquet_write_dict_pages", "parquet_write_dict_entries",
            "parquet_write_dict_index_pages", "parquet_write_dict_rle_index_pages", "parquet_write_dict_fallback_chunks"]
TOP = D.MAX_DICTIONARY


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return D.build_program(tmp_path_factory.mktemp("parquet_dict_write_check"), False)


def read_back(path):
    src = ex.ParquetDataSource(path)
    schema = src.schema()
    return pa.Table.from_batches(list(src), schema=schema)


def write(path, schema, batches, relation, options):
    rel = relation if relation is not None else ex.DataSourceRelation(schema, batches)
    ex.counter_reset()
    rows, nbytes = ex.write_parquet(rel, path, options)
    counters = {k: ex.counter_get(k) for k in COUNTERS}
    assert rows == sum(b.num_rows for b in batches)
    assert nbytes == os.path.getsize(path) == counters["parquet_write_bytes"]
    assert not os.path.exists(path + ".dfx-partial")
    return counters


def assert_same_bytes(path, other, name):
    got, want = open(path, "rb").read(), open(other, "rb").read()
    if got != want:
        at = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError(f"{name}: the file differs from {os.path.basename(other)} at byte {at} of {len(got)} / {len(want)}: "
                             f"{got[max(0, at - 16):at + 16].hex()} != {want[max(0, at - 16):at + 16].hex()}")


def write_and_check(program, tmp_path, schema, batches, limit, relation=None, options=None, name="out.parquet"):
    """writes `relation` (default: the batches as a host stream) under dictionary = limit and holds the file the three ways; `batches`:
    the batches as the sink receives them.  Returns (path, counters of the call, {(row group, column): (entries, pages)})."""
    path = str(tmp_path / name)
    options = dict(options or {})
    rg, pr = options.get("row_group_rows", W.DEFAULT_ROW_GROUP_ROWS), options.get("page_rows", W.DEFAULT_PAGE_ROWS)
    options["dictionary"] = limit
    counters = write(path, schema, batches, relation, options)
    report = D.host_write(program, W.describe(schema, batches, rg, pr), path + ".host", tmp_path, limit)
    assert report["code"] == 0 and report["reader_code"] == 0 and report["mismatch"] == "", {k: report[k] for k in report if k != "row_groups"}
    assert_same_bytes(path, path + ".host", name)
    chunks = D.check_file(path, schema, batches, limit, rg, pr, what=name, report=report)
    W.assert_same_table(read_back(path), pa.Table.from_batches(batches, schema=schema), name + " through dfx_parquet_datasource_new")
    pages = [p for _, ps in chunks.values() for p in ps]
    want = {"parquet_write_row_groups": 1 + max((g for g, _ in chunks), default=-1), "parquet_write_pages": len(pages),
            "parquet_write_dict_pages": sum(1 for e, _ in chunks.values() if e is not None),
            "parquet_write_dict_entries": sum(len(e) for e, _ in chunks.values() if e is not None),
            "parquet_write_dict_index_pages": sum(1 for p in pages if p[0] != "plain"),
            "parquet_write_dict_rle_index_pages": sum(1 for p in pages if p[0] == "rle"),
            "parquet_write_dict_fallback_chunks": sum(1 for (g, c), (e, ps) in chunks.items()
                                                      if limit > 0 and schema.field(c).type != pa.bool_() and any(p[0] == "plain" for p in ps))}
    assert {k: counters[k] for k in want} == want, name
    return path, counters, chunks


SMALL = {"row_group_rows": 250, "page_rows": 128}


@pytest.mark.parametrize("nullable", [True, False])
@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 63, 64, 65, 1000])
def test_all_types_at_the_row_count_edges(program, tmp_path, n, nullable):
    """the eleven non-Boolean types and a Boolean column, which stays PLAIN beside them"""
    b = D.cardinality_batch(n, 5, nullable, n)
    schema = D.eleven_schema(nullable)
    write_and_check(program, tmp_path, schema, [b], TOP, name="default.parquet")
    _, c, chunks = write_and_check(program, tmp_path, schema, [b], 16, options=SMALL, name="small.parquet")
    if n > 0:
        assert chunks[(0, 0)][0] is None and all(chunks[(0, k)][0] is not None for k in range(1, 12))
        assert c["parquet_write_dict_fallback_chunks"] == 0


@pytest.mark.parametrize("page_rows", [64, 128])
@pytest.mark.parametrize("distinct", [1, 2, 3, 4, 256, 257, 900])
def test_cardinalities_over_pieces_and_groups(program, tmp_path, distinct, page_rows):
    """batches of 300 rows into groups of 250 (700 where a group has to hold 256 entries and more): several pieces per group, several
    groups per batch, dictionaries that grow over launches and start empty at every group.  1: RLE index pages; 2 -> 3, 4: width 1 -> 2;
    256 -> 257: width 8 -> 9, where indices straddle bytes and 32-bit words; 900 in 300-row batches: nearly every row distinct"""
    nullable = distinct < 256
    schema = D.eleven_schema(nullable)
    batches = [D.cardinality_batch(300, distinct, nullable, 40 + i) for i in range(3)]
    options = {"row_group_rows": 250 if distinct < 256 else 700, "page_rows": page_rows}
    _, c, chunks = write_and_check(program, tmp_path, schema, batches, TOP, options=options)
    widths = {p[1] for (g, k), (e, ps) in chunks.items() if k == 3 for p in ps}
    if distinct == 1:
        assert c["parquet_write_dict_rle_index_pages"] == c["parquet_write_dict_index_pages"] > 0, c
    if distinct in (3, 4):
        assert 2 in widths, widths
    if distinct in (256, 257):
        assert max(widths) == (8 if distinct == 256 else 9), widths
    if page_rows == 64 and distinct == 2:  # the same rows from a resident table, in slices of 320 rows
        table = ex.DeviceTable.from_batches(schema, batches)
        whole = pa.Table.from_batches(batches, schema=schema).combine_chunks()
        seen = [whole.slice(r, 320).to_batches()[0] for r in range(0, 900, 320)]
        write_and_check(program, tmp_path, schema, seen, TOP, relation=table.scan(320), options=options, name="resident.parquet")


def test_every_row_distinct_special_values_and_the_empty_word(program, tmp_path):
    b = W.all_types_batch(1000, True, 77)  # two NaN payloads and more, -0.0 and +0.0, the integer extremes, UInt64 above 2^63
    _, _, chunks = write_and_check(program, tmp_path, W.all_types_schema(True), [b], TOP, options={"page_rows": 128}, name="distinct.parquet")
    assert {0x7FF8000000000001, 0xFFF8000000000000, 0x0, 0x8000000000000000} <= set(chunks[(0, 10)][0])
    assert any(k >= 2 ** 63 for k in chunks[(0, 8)][0])
    schema, edge = D.edge_batch()  # UInt64 2^64 - 1 and Int64 -1: the key that equals the table's empty word
    _, _, chunks = write_and_check(program, tmp_path, schema, [edge], 4, options={"page_rows": 64}, name="all-ones.parquet")
    assert chunks[(0, 0)][0] == [2 ** 64 - 1, 0, 2 ** 63] == chunks[(0, 1)][0]


def test_a_page_of_equal_indices_inside_a_mixed_chunk(program, tmp_path):
    schema = pa.schema([pa.field("v", pa.int16()), pa.field("s", pa.string())])
    v = [i % 7 for i in range(64)] + [3] * 64 + [i % 5 for i in range(40)]
    b = pa.RecordBatch.from_arrays([pa.array(v, pa.int16(), mask=np.arange(168) % 8 == 5), pa.array([f"k{x}" for x in v])], schema=schema)
    _, c, chunks = write_and_check(program, tmp_path, schema, [b], TOP, options={"page_rows": 64})
    assert [p[0] for p in chunks[(0, 0)][1]] == ["packed", "rle", "packed"] == [p[0] for p in chunks[(0, 1)][1]]
    assert c["parquet_write_dict_rle_index_pages"] == 2


def test_nulls(program, tmp_path):
    schema, b = D.nulls_batch()
    path, _, chunks = write_and_check(program, tmp_path, schema, [b], 64, options={"page_rows": 64})
    assert [p[0] for p in chunks[(0, 0)][1]] == ["packed", "none", "packed"]
    assert chunks[(0, 1)][0] == [] and [p[0] for p in chunks[(0, 1)][1]] == ["none"] * 3  # a zero-entry dictionary page
    assert chunks[(0, 2)][0] == [f"w{i}".encode() for i in (1, 2, 3, 4, 0)] and b"hidden" not in open(path, "rb").read()


def test_utf8_values(program, tmp_path):
    schema, b = W.utf8_batch()  # the empty string, multi-byte characters, a 20 kB value in the middle of a tile, a tile of empty strings
    write_and_check(program, tmp_path, schema, [b], TOP, options={"page_rows": 64}, name="u64.parquet")
    write_and_check(program, tmp_path, schema, [b], TOP, name="u.parquet")
    schema, b = D.same16_batch()  # equal in their first 16 bytes; a 316-byte value
    _, _, chunks = write_and_check(program, tmp_path, schema, [b], 4, options={"page_rows": 64}, name="same16.parquet")
    assert chunks[(0, 0)][0] == [t.encode() for t in D.SAME16]


def test_the_decision_by_launch(program, tmp_path):
    schema, mk = D.DECISION_SCHEMA, D.decision_batch
    # three values, then three new ones, then only old ones: dictionary pages, then PLAIN pages, then PLAIN pages
    batches = [mk([1, 2, 3] * 30), mk([4, 5, 6] * 30), mk([1, 2, 3] * 30)]
    path, c, chunks = write_and_check(program, tmp_path, schema, batches, 4, options={"page_rows": 64}, name="fallback.parquet")
    for k in range(2):
        assert len(chunks[(0, k)][0]) == 3 and [p[0] for p in chunks[(0, k)][1]] == ["packed", "packed", "plain", "plain", "plain", "plain"]
        assert set(pq.ParquetFile(path).metadata.row_group(0).column(k).encodings) == {"PLAIN", "RLE", "RLE_DICTIONARY"}
    assert c["parquet_write_dict_fallback_chunks"] == 2 and c["parquet_write_dict_pages"] == 2 and c["parquet_write_dict_entries"] == 6, c
    # exactly four entries stay
    _, c, chunks = write_and_check(program, tmp_path, schema, [mk([1, 2, 3] * 30), mk([4] * 90)], 4, options={"page_rows": 64}, name="four.parquet")
    assert len(chunks[(0, 0)][0]) == 4 and [p[0] for p in chunks[(0, 0)][1]] == ["packed", "packed", "rle", "rle"] and c["parquet_write_dict_fallback_chunks"] == 0
    # five values in the first batch: byte for byte the file written without the option
    five = [mk([1, 2, 3, 4, 5] * 20), mk([1] * 10)]
    path, c, chunks = write_and_check(program, tmp_path, schema, five, 4, options={"page_rows": 64}, name="five.parquet")
    assert chunks[(0, 0)][0] is None and c["parquet_write_dict_fallback_chunks"] == 2 and c["parquet_write_dict_pages"] == 0, c
    write(path + ".without", schema, five, None, {"page_rows": 64})
    assert_same_bytes(path, path + ".without", "five.parquet")


def test_the_option_at_zero_is_the_file_written_without_it(program, tmp_path):
    schema = D.eleven_schema(True)
    batches = [D.cardinality_batch(300, 3, True, 90 + i) for i in range(2)]
    path, c, _ = write_and_check(program, tmp_path, schema, batches, 0, options=SMALL, name="zero.parquet")
    assert all(c[k] == 0 for k in COUNTERS if "dict" in k), c
    write(path + ".without", schema, batches, None, SMALL)
    assert_same_bytes(path, path + ".without", "zero.parquet")


def test_a_forced_hash_collision_falls_back(tmp_path):
    """dictionary_hash_bits = 4: a hundred distinct strings share sixteen hashes, the compare of k_pqwd_mark sees it and the chunk is
    written PLAIN; the Int32 column beside it keeps its dictionary.  Only the two read-backs: the host encoder knows no hash."""
    schema = pa.schema([pa.field("s", pa.string()), pa.field("v", pa.int32())])
    b = pa.RecordBatch.from_arrays([pa.array([f"string-{i % 100}" for i in range(300)]), pa.array(np.arange(300, dtype=np.int32) % 100)], schema=schema)
    path = str(tmp_path / "collide.parquet")
    c = write(path, schema, [b], None, {"dictionary": 1 << 10, "dictionary_hash_bits": 4, "page_rows": 64})
    assert c["parquet_write_dict_fallback_chunks"] == 1 and c["parquet_write_dict_pages"] == 1 and c["parquet_write_dict_entries"] == 100, c
    want = pa.Table.from_batches([b], schema=schema)
    W.assert_same_table(pq.read_table(path), want, "collide through pyarrow")
    W.assert_same_table(read_back(path), want, "collide through dfx_parquet_datasource_new")
    md = pq.ParquetFile(path).metadata.row_group(0)
    assert not md.column(0).has_dictionary_page and md.column(1).has_dictionary_page
    # the same strings at 64 bits: a dictionary
    c = write(path, schema, [b], None, {"dictionary": 1 << 10, "page_rows": 64})
    assert c["parquet_write_dict_fallback_chunks"] == 0 and c["parquet_write_dict_entries"] == 200, c


def test_the_source_walks_the_dictionary_only(program, tmp_path):
    """the library's own reader walks a length in front of every string it has to find: the dictionary's entries with the option, every
    non-null row without"""
    schema = pa.schema([pa.field("s", pa.string())])
    b = pa.RecordBatch.from_arrays([pa.array([None if i % 9 == 0 else f"city-{i % 37}" for i in range(1000)])], schema=schema)
    for limit, want in ((TOP, 37), (0, 1000 - b.column(0).null_count)):
        path, _, _ = write_and_check(program, tmp_path, schema, [b], limit, options={"page_rows": 128}, name=f"walk{limit}.parquet")
        ex.counter_reset()
        read_back(path)
        assert ex.counter_get("parquet_host_walked_strings") == want, limit


def test_two_launches_inside_one_piece(program, tmp_path):
    """2^20 + 65 rows in one batch, 1000 distinct values: the second launch meets the first launch's entries (the row group ends with the
    first launch, so the 65 rows start a dictionary of their own: the group of 2^21 rows keeps both launches in one chunk)"""
    n = (1 << 20) + 65
    schema = pa.schema([pa.field("v", pa.int32()), pa.field("s", pa.string(), nullable=False)])
    k = (np.arange(n, dtype=np.int64) * 7919) % 1000
    k[-65:] = np.arange(65) % 2 * 997 + np.arange(65) % 3  # old entries only, in the second launch
    pool = np.array([f"value-{i:04d}" for i in range(1000)])
    b = pa.RecordBatch.from_arrays([pa.array((k * 3 - 1500).astype(np.int32), mask=np.arange(n) % 1001 == 7), pa.array(pool[k])], schema=schema)
    path = str(tmp_path / "big.parquet")
    options = {"dictionary": 1 << 10, "row_group_rows": 1 << 21}
    c = write(path, schema, [b], None, options)
    report = D.host_write(program, W.describe(schema, [b], 1 << 21), path + ".host", tmp_path, 1 << 10)
    assert report["code"] == 0 and report["mismatch"] == "", {k: report[k] for k in report if k != "row_groups"}
    assert_same_bytes(path, path + ".host", "big.parquet")
    want = pa.Table.from_batches([b], schema=schema)
    W.assert_same_table(pq.read_table(path), want, "big through pyarrow")
    W.assert_same_table(read_back(path), want, "big through dfx_parquet_datasource_new")
    assert c["parquet_write_row_groups"] == 1 and c["parquet_write_pages"] == 2 * 33 == c["parquet_write_dict_index_pages"], c
    assert c["parquet_write_dict_pages"] == 2 and c["parquet_write_dict_entries"] == 2000 and c["parquet_write_dict_fallback_chunks"] == 0, c
    assert [p["width"] for p in report["row_groups"][0]["chunks"][0]["pages"]] == [10] * 33


def _operator_input():
    """eleven types (FilterRelation takes no Boolean column); the Utf8 column without nulls: it is the key"""
    rng = np.random.default_rng(77)
    schema = pa.schema([pa.field(n, t) for n, t in W.ALL_TYPES[1:]])
    batches = []
    for i in range(2):
        b = D.cardinality_batch(3000, 40, True, 60 + i)
        batches.append(pa.RecordBatch.from_arrays(b.columns[1:-1] + [W.column(pa.string(), 3000, rng)], schema=schema))
    return schema, batches


def test_operator_outputs(program, tmp_path):
    schema, batches = _operator_input()
    i32, i64, f64, utf8 = (schema.get_field_index(n) for n in ("i32", "i64", "f64", "s"))
    table = ex.DeviceTable.from_batches(schema, batches)
    pred = BinaryExpr(Column(i32), Operator.Gt, Literal(ScalarValue.Int32(0)))
    flt = lambda: ex.FilterRelation(table.scan(1024), ex.compile_scalar_expr(None, pred, schema), schema)
    rel = flt()
    out_schema, want = rel.schema(), list(rel)
    assert 0 < sum(b.num_rows for b in want) < 6000
    write_and_check(program, tmp_path, out_schema, want, TOP, relation=flt(), options={"page_rows": 256}, name="filter.parquet")

    srt = lambda: ex.LimitRelation(ex.SortRelation(table.scan(1024), [(ex.compile_scalar_expr(None, Column(f64), schema), False)], schema), 777, schema)
    rel = srt()
    out_schema, want = rel.schema(), list(rel)
    assert sum(b.num_rows for b in want) == 777
    write_and_check(program, tmp_path, out_schema, want, TOP, relation=srt(), options={"page_rows": 256}, name="sort.parquet")

    agg = lambda: ex.AggregateRelation(None, table.scan(1024), [ex.compile_scalar_expr(None, Column(utf8), schema)],
                                       [ex.compile_expr(None, AggregateFunction("MAX", [Column(f64)], DataType.Float64), schema),
                                        ex.compile_expr(None, AggregateFunction("COUNT", [Column(i64)], DataType.UInt64), schema)])
    rel = agg()
    out_schema, want = rel.schema(), list(rel)
    assert len(want) == 1 and want[0].num_rows > 10
    # (two runs of a hash aggregate may emit their groups in different orders: the file must hold the same groups, and its bytes must
    # be the host encoder's for the rows in the order the file has them)
    path = str(tmp_path / "agg.parquet")
    rows, _ = ex.write_parquet(agg(), path, {"page_rows": 64, "dictionary": TOP})
    assert rows == want[0].num_rows
    got = pq.read_table(path)
    assert got.schema.names == out_schema.names and got.schema.types == out_schema.types
    assert_groups_identical(got.combine_chunks().to_batches()[0], want[0], 1, "GROUP BY written as Parquet with dictionaries")
    again = got.combine_chunks().to_batches()
    D.host_write(program, W.describe(out_schema, again, page_rows=64), path + ".host", tmp_path, TOP)
    assert_same_bytes(path, path + ".host", "agg.parquet")
    assert pq.ParquetFile(path).metadata.row_group(0).column(0).has_dictionary_page
    W.assert_same_table(read_back(path), got, "GROUP BY through dfx_parquet_datasource_new")


@pytest.mark.parametrize("offset", [0, 3, 67])
def test_source_offsets_and_sliced_resident_tables(program, tmp_path, offset):
    """every buffer and bitmap of the source starts `offset` rows / bits in: sliced batches through a host stream; and a resident table
    scanned from row 64 * offset (a resident scan begins at a multiple of 64: General otherwise), where the scan's batches are slices"""
    schema = D.eleven_schema(True)
    options = {"page_rows": 64, "row_group_rows": 250}
    batches = [D.cardinality_batch(500, 9, True, 300).slice(offset, 300), D.cardinality_batch(400, 9, True, 301).slice(offset), D.cardinality_batch(70, 9, True, 302).slice(offset)]
    assert batches[0].column(1).offset == offset
    write_and_check(program, tmp_path, schema, batches, 16, options=options, name="host.parquet")
    whole = [D.cardinality_batch(2500, 9, True, 310 + i) for i in range(2)]
    table = ex.DeviceTable.from_batches(schema, whole)
    begin = 64 * offset
    seen = pa.Table.from_batches(whole, schema=schema).combine_chunks().slice(begin, 600).to_batches()
    write_and_check(program, tmp_path, schema, seen, 16, relation=table.scan(0, begin, 600), options=options, name="resident.parquet")


def test_csv_to_parquet_to_group_by(program, tmp_path):
    """uk_cities.csv -> write_parquet with dictionaries -> SUM(lat) GROUP BY city over the Parquet file == the same query over the CSV"""
    schema = fixtures.uk_cities_schema()
    csv = lambda: ex.CsvDataSource(os.path.join(DATA, "uk_cities.csv"), schema, 1024)
    rel = csv()
    out_schema, seen = rel.schema(), list(rel)
    path, c, _ = write_and_check(program, tmp_path, out_schema, seen, TOP, relation=csv(), name="uk_cities.parquet")
    assert c["parquet_write_dict_pages"] == len(out_schema)

    def query(src):
        s = src.schema()
        r = ex.AggregateRelation(None, src, [ex.compile_scalar_expr(None, Column(0), s)],
                                 [ex.compile_expr(None, AggregateFunction("SUM", [Column(1)], DataType.Float64), s),
                                  ex.compile_expr(None, AggregateFunction("MIN", [Column(2)], DataType.Float64), s)])
        return r.next()

    over_csv, over_parquet = query(csv()), query(ex.ParquetDataSource(path))
    assert over_csv.num_rows == sum(b.num_rows for b in seen) > 30
    assert_groups_identical(over_parquet, over_csv, 1, "SUM GROUP BY over the written Parquet file")
