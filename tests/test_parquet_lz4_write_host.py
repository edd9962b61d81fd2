"""CPU tests of the Parquet writer's "compression" option: csrc/dfx_parquet_lz4_enc.hpp (the block rule and its sequential encoder) with
the additions to csrc/dfx_parquet_thrift_write.hpp and csrc/dfx_parquet_enc.hpp, through tests/native/parquet_lz4_write_check.cpp, a
stand-alone program built once plain and once under the host sanitizers.  Every block is held against the library's own decoder
(lz4_decode_block, inside the program), against pyarrow's (pa.Codec('lz4_raw')), against its bound, against LZ4's end-of-block rules and
against the rule restated in Python, byte for byte.  Every file is held against pyarrow (the table that went in by bit patterns, the
chunk metadata) and against the library's reader headers, called from the same program.  dfx_parquet_write itself needs a GPU: what it
refuses without one is at the end."""
import os

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import parquet_dict_write_cases as D
import parquet_lz4_write_cases as Z
import parquet_write_cases as W

from datafusion_archive_amd import execution as ex


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("parquet_lz4_write_check")
    return {"plain": Z.build_program(d, False), "sanitized": Z.build_program(d, True)}


CODEC = pa.Codec("lz4_raw")


def check_block(programs, tmp_path, name, data, which="sanitized"):
    """the four checks of a block; returns (block, report)"""
    block, rep = Z.host_block(programs[which], data, tmp_path, name)
    n = len(data)
    assert rep["n"] == n and rep["bytes"] == len(block) and rep["bound"] == Z.bound(n), (name, rep)
    assert rep["decodes"] and rep["equal"], (name, "lz4_decode_block")
    assert CODEC.decompress(block, decompressed_size=n).to_pybytes() == data, (name, "pyarrow")
    assert len(block) <= Z.bound(n), (name, len(block))
    assert rep["walked"] and rep["walked_sequences"] == rep["sequences"] == rep["decoder_sequences"], (name, rep)
    if rep["matches"]:  # the last match starts at or before n - 12, the last 5 bytes are literals
        assert rep["last_match_start"] <= n - 12 and rep["last_match_end"] <= n - 5, (name, rep)
    assert rep["max_offset"] <= 65535, (name, rep)
    want, seqs = Z.encode(data)
    assert block == want and rep["sequences"] == len(seqs), (name, "the rule restated in Python")
    return block, rep


# ---- blocks ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,data", Z.block_inputs(), ids=[n for n, _ in Z.block_inputs()])
def test_blocks(programs, tmp_path, name, data):
    block, rep = check_block(programs, tmp_path, name, data)
    n = len(data)
    if n < 13:
        assert rep["sequences"] == 1 and len(block) == n + 1, rep  # one literal-only sequence; n == 0: the token alone
    if name.startswith("random-"):
        assert rep["matches"] == 0 and len(block) == 1 + (0 if n < 15 else (n - 15) // 255 + 1) + n, rep
    if name == "far-repeat":  # the repeat lies beyond the window
        assert rep["matches"] == 0 and rep["lit_extensions"] == (144000 - 15) // 255 + 1, rep
    if name == "period-40000":
        assert rep["max_offset"] == 40000, rep
    if name == "arange":
        assert rep["sequences"] > 10000 and len(block) < n * 0.6, rep


def test_zeros_4096_is_90_bytes_in_2_sequences(programs, tmp_path):
    block, rep = check_block(programs, tmp_path, "zeros", bytes(4096), which="plain")
    # 66 bytes: the first sequence's token, one extension byte and 64 literals; 2 of offset; 16 of match extension; 6: the last sequence
    assert len(block) == 90 == 66 + 2 + 16 + 6 and rep["sequences"] == 2, rep
    assert rep["seqs"] == [[64, 1, 4027], [5, 0, 0]] and rep["match_extensions"] == 16 and rep["lit_extensions"] == 1, rep
    assert rep["steps_without_pick"] == 1, rep


@pytest.mark.parametrize("lit", [14, 15, 16, 269, 270, 271])
def test_literal_run_lengths(programs, tmp_path, lit):
    """the token's nibble below, at and past 15; the extension chain below, at and past one 255"""
    data = Z.seeded(Z.literal_run_input, lit, lambda seqs: len(seqs) == 3 and seqs[1][0] == lit)
    _, rep = check_block(programs, tmp_path, f"lit-{lit}", data)
    assert rep["seqs"][1][0] == lit and rep["seqs"][1][2] == 8, rep["seqs"]


@pytest.mark.parametrize("match_len", [18, 19, 20, 273, 274])
def test_match_lengths(programs, tmp_path, match_len):
    data = Z.seeded(Z.match_input, match_len, lambda seqs: len(seqs) == 2 and seqs[0][2] == match_len)
    _, rep = check_block(programs, tmp_path, f"match-{match_len}", data)
    assert rep["seqs"][0] == [101 + match_len, 101 + match_len, match_len], rep["seqs"]
    assert rep["match_extensions"] == (0 if match_len < 19 else (match_len - 19) // 255 + 1), rep


def test_the_candidate_rule_at_its_edges(programs):
    # distance 65535 holds, 65536 does not; ref == p does not; an empty entry does not
    assert Z.rules(programs["sanitized"], "candidate") == [1, 0, 0, 0]


def test_the_i32_rule_on_made_up_sizes(programs):
    """a body whose block's bound, n + n // 255 + 16, exceeds 2^31 - 1 is refused: the page header holds the compressed size in an i32"""
    top = 2 ** 31 - 1
    n = (top - 16) * 255 // 256 - 2
    while Z.bound(n + 1) <= top:  # the largest n that fits
        n += 1
    assert Z.bound(n) <= top < Z.bound(n + 1)
    sizes = [0, 12, 13, 4096, n - 1, n, n + 1, top, top + 1, 2 ** 32, 2 ** 63]
    got = Z.rules(programs["sanitized"], "fits", sizes)
    assert [g[0] for g in got[:8]] == [Z.bound(v) for v in sizes[:8]]
    assert [g[1] for g in got] == [1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], got


# ---- whole files ----------------------------------------------------------------------------------------------------------------------
def write_and_check(programs, tmp_path, name, schema, batches, dictionary=0, row_group_rows=W.DEFAULT_ROW_GROUP_ROWS, page_rows=W.DEFAULT_PAGE_ROWS, which="sanitized"):
    path = str(tmp_path / f"{name}.parquet")
    report = Z.host_write(programs[which], W.describe(schema, batches, row_group_rows, page_rows), path, tmp_path, dictionary)
    return path, report, Z.check_file(path, schema, batches, report, row_group_rows, page_rows, what=name)


@pytest.mark.parametrize("dictionary", [0, 16])
@pytest.mark.parametrize("page_rows", [64, 128])
@pytest.mark.parametrize("nullable", [True, False])
@pytest.mark.parametrize("n", [0, 1, 7, 64, 65, 1000])
def test_all_types(programs, tmp_path, n, nullable, page_rows, dictionary):
    b = D.cardinality_batch(n, 5, nullable, n) if dictionary else W.all_types_batch(n, nullable, n)
    schema = D.eleven_schema(nullable) if dictionary else W.all_types_schema(nullable)
    _, report, pages = write_and_check(programs, tmp_path, "all", schema, [b], dictionary, row_group_rows=250, page_rows=page_rows,
                                       which="sanitized" if page_rows == 64 else "plain")
    if n == 0:
        assert pages == [] and report["row_groups"] == []
    if dictionary and n > 0:
        chunks = report["row_groups"][0]["chunks"]
        assert not chunks[0]["has_dict"] and all(c["has_dict"] and c["pages"][0]["type"] == 2 for c in chunks[1:]), "the dictionary pages are blocks too"


def test_a_chunk_that_falls_back_mid_chunk(programs, tmp_path):
    schema, batches = Z.fallback_batches()
    path, report, _ = write_and_check(programs, tmp_path, "fallback", schema, batches, 4, page_rows=64)
    for c in range(2):
        assert set(pq.ParquetFile(path).metadata.row_group(0).column(c).encodings) == {"PLAIN", "RLE", "RLE_DICTIONARY"}
        assert [p["type"] for p in report["row_groups"][0]["chunks"][c]["pages"]] == [2, 0, 0, 0, 0, 0, 0]


def test_an_all_null_column_with_a_dictionary(programs, tmp_path):
    """a dictionary without an entry: its page's body is empty, and its block is the token of no literals (one byte)"""
    schema, b = D.nulls_batch()
    _, report, _ = write_and_check(programs, tmp_path, "nulls", schema, [b], 64, page_rows=64)
    first = report["row_groups"][0]["chunks"][1]["pages"][0]
    assert first["type"] == 2 and first["uncompressed"] == 0 and first["compressed"] == 1, first


@pytest.mark.parametrize("shape", Z.shapes(), ids=[s[0] for s in Z.shapes()])
def test_shapes(programs, tmp_path, shape):
    name, schema, batch, page_rows, dictionary = shape
    _, report, pages = write_and_check(programs, tmp_path, name, schema, [batch], dictionary, page_rows=page_rows, which="plain")
    if name == "random":
        assert pages[0]["compressed"] > pages[0]["uncompressed"] and report["row_groups"][0]["chunks"][0]["oversized_v1_pages"] == 1, pages
    if name == "zeros":
        assert pages[0]["sequences"] == 2 and pages[0]["uncompressed"] == 40000, pages
    if name == "single":
        assert pages[0]["uncompressed"] == 8 and pages[0]["compressed"] == 9 and pages[0]["sequences"] == 1, pages
    if name == "period-40000":
        assert len(pages) == 1 and pages[0]["uncompressed"] > 65536, pages
    if name == "far-repeat":
        assert pages[0]["sequences"] == 1, pages


def test_without_the_codec_the_writer_is_what_it_was(tmp_path):
    """A guard of the defaults, not a test of the option (it passes without it): tests/native/parquet_write_check.cpp compiles untouched
    against the changed FileWriter and writes UNCOMPRESSED files as before"""
    exe = W.build_program(tmp_path, False)
    schema, b = W.all_types_schema(True), W.all_types_batch(100, True, 3)
    path = str(tmp_path / "plain.parquet")
    report = W.host_write(exe, W.describe(schema, [b], page_rows=64), path, tmp_path)
    assert report["code"] == 0 and report["mismatch"] == ""
    W.check_file(path, schema, [b], page_rows=64)


# ---- the library without a device -----------------------------------------------------------------------------------------------------
def _one_batch():
    schema = pa.schema([pa.field("v", pa.int32()), pa.field("s", pa.string())])
    return schema, pa.RecordBatch.from_arrays([pa.array([1, None, 3], pa.int32()), pa.array(["a", "", None])], schema=schema)


def _nothing_left(target):
    assert not os.path.exists(str(target)) and not os.path.exists(str(target) + ".dfx-partial")


@pytest.mark.parametrize("codec", [-1, 1, 2, 5, 6, 8])
def test_other_codecs_are_refused_without_a_device(tmp_path, codec):
    schema, b = _one_batch()
    target = tmp_path / "o.parquet"
    with pytest.raises(ex.ExecutionError) as ei:
        ex.write_parquet(ex.DataSourceRelation(schema, [b]), str(target), {"compression": codec})
    assert ei.value.kind == "General" and "compression = %d" % codec in str(ei.value), ei.value
    _nothing_left(target)


def test_the_named_constant():
    assert ex.PARQUET_COMPRESSION_LZ4_RAW == 7 and ex.PARQUET_COMPRESSION_UNCOMPRESSED == 0


def test_a_valid_call_without_a_device_fails_for_want_of_a_device(tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: tests/test_gpu_parquet_lz4_write.py writes files")
    schema, b = _one_batch()
    target = tmp_path / "o.parquet"
    with pytest.raises(ex.ExecutionError) as ei:
        ex.write_parquet(ex.DataSourceRelation(schema, [b]), str(target), {"compression": ex.PARQUET_COMPRESSION_LZ4_RAW, "dictionary": 16})
    assert ei.value.kind == "ExecutionError" and "no HIP device available" in str(ei.value), ei.value
    _nothing_left(target)
