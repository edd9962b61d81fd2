"""What the CPU tests (tests/test_parquet_lz4_write_host.py) and the GPU tests (tests/test_gpu_parquet_lz4_write.py) of the Parquet
writer's "compression" option share: the stand-alone program tests/native/parquet_lz4_write_check.cpp built at test time, the block
rule of csrc/dfx_parquet_lz4_enc.hpp restated in Python, the inputs chosen for the sequences the rule makes of them, and the comparison
of a written file with the table that went in -- pyarrow's reader bit for bit, pyarrow's metadata, and the program's own report, which
takes the file back through the library's reader headers.  The description of the batches and the value comparison are
parquet_write_cases.py's; the periods are parquet_lz4_cases.py's.  No binary fixture is committed."""
from __future__ import annotations

import json
import os
import subprocess

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq

import parquet_lz4_cases as L
import parquet_write_cases as W

SRC = os.path.join(W.ROOT, "tests", "native", "parquet_lz4_write_check.cpp")
LZ4_RAW = 7
SEED = W.SEED + 4242
BLOCK_SIZES = [0, 1, 4, 5, 11, 12, 13, 14, 63, 64, 65, 67, 68, 127, 128, 129, 269, 270, 271, 4095, 4096, 4097]


def build_program(directory, sanitized: bool) -> str:
    exe = os.path.join(str(directory), "parquet_lz4_write_check_" + ("sanitized" if sanitized else "plain"))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitized else []
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror"] + flags + ["-o", exe, SRC])
    return exe


def host_write(exe: str, desc: bytes, out_path: str, tmp_dir, dictionary: int = 0) -> dict:
    """runs `write` of the program: the file at out_path (compression = 7) and the program's JSON report"""
    desc_path = os.path.join(str(tmp_dir), os.path.basename(out_path) + ".desc")
    with open(desc_path, "wb") as fh:
        fh.write(desc)
    r = subprocess.run([exe, "write", desc_path, out_path, str(dictionary)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"{os.path.basename(exe)} write: exit {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}"
    os.remove(desc_path)
    return json.loads(r.stdout)


def host_block(exe: str, data: bytes, tmp_dir, name: str = "block"):
    """runs `block` of the program: (the block's bytes, the program's JSON report)"""
    in_path, out_path = os.path.join(str(tmp_dir), name + ".in"), os.path.join(str(tmp_dir), name + ".lz4")
    with open(in_path, "wb") as fh:
        fh.write(data)
    r = subprocess.run([exe, "block", in_path, out_path], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"{os.path.basename(exe)} block {name}: exit {r.returncode}\n{r.stdout[-1500:]}\n{r.stderr[-3000:]}"
    block = open(out_path, "rb").read()
    os.remove(in_path)
    os.remove(out_path)
    return block, json.loads(r.stdout)


def rules(exe: str, command: str, numbers=()) -> list:
    r = subprocess.run([exe, command] + [str(v) for v in numbers], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


# ---- the rule, restated ---------------------------------------------------------------------------------------------------------------
def bound(n: int) -> int:
    return n + n // 255 + 16


def _ext(v: int) -> bytes:
    """the extension chain of a length whose nibble is 15"""
    if v < 15:
        return b""
    v -= 15
    return b"\xff" * (v // 255) + bytes([v % 255])


def _sequence(lits: bytes, offset: int = 0, match_len: int = 0) -> bytes:
    ml = match_len - 4 if match_len else 0
    out = bytes([min(len(lits), 15) << 4 | min(ml, 15)]) + _ext(len(lits)) + lits
    return out + (offset.to_bytes(2, "little") + _ext(ml) if match_len else b"")


def encode(data: bytes):
    """(the block, its sequences as (literals, offset, match length)) by the rule of csrc/dfx_parquet_lz4_enc.hpp, restated"""
    n, out, seqs, anchor, cur, table = len(data), [], [], 0, 0, [0] * 4096
    slot = lambda p: ((int.from_bytes(data[p:p + 4], "little") * 2654435761) & 0xFFFFFFFF) >> 20
    while n >= 13 and cur <= n - 12:
        step = range(cur, min(cur + 64, n - 12 + 1))
        before = [table[slot(p)] - 1 for p in step]  # every position reads the table as it stood before the step
        held = [(p, r) for p, r in zip(step, before) if 0 <= r < p and p - r <= 65535 and data[r:r + 4] == data[p:p + 4]]
        pick = held[0] if held else None
        for p in step:
            if pick is None or p <= pick[0]:
                table[slot(p)] = max(table[slot(p)], p + 1)
        if pick is None:
            cur = step[-1] + 1
            continue
        s, r = pick
        length = 4
        while s + length < n - 5 and data[r + length] == data[s + length]:
            length += 1
        out.append(_sequence(data[anchor:s], s - r, length))
        seqs.append((s - anchor, s - r, length))
        anchor = cur = s + length
    out.append(_sequence(data[anchor:]))
    seqs.append((n - anchor, 0, 0))
    return b"".join(out), seqs


# ---- block inputs ---------------------------------------------------------------------------------------------------------------------
def period_bytes(p: int, rng) -> bytes:
    return L._period(p, rng).tobytes()


def block_inputs():
    """[(name, bytes)] in a fixed order"""
    rng = np.random.default_rng(SEED)
    out = []
    for n in BLOCK_SIZES:
        out.append((f"zeros-{n}", bytes(n)))
        out.append((f"random-{n}", rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()))
    for p in L.PERIODS:
        out.append((f"period-{p}", period_bytes(p, rng)))
    out.append(("arange", np.arange(20000, dtype=np.int64).tobytes()))
    half = rng.integers(0, 256, size=72000, dtype=np.uint8).tobytes()
    out.append(("far-repeat", half + half))
    out.append(("alphabet-3", bytes(rng.integers(97, 100, size=6000, dtype=np.uint8))))
    out.append(("rounded-floats", np.round(rng.standard_normal(3000) * 10, 1).tobytes()))
    return out


def literal_run_input(lit: int, seed: int) -> bytes:
    """70 random bytes; their first 8 again (position 70 lies in the second step and finds position 0 in the table: a first match);
    `lit` random literals; bytes 20 .. 28 of the head again (the second match, so the second sequence's literal run is `lit` long);
    a tail that ends the match and keeps it clear of the block's end"""
    rng = np.random.default_rng(SEED + 100 + seed)
    head = rng.integers(0, 256, size=70, dtype=np.uint8).tobytes()
    return head + head[:8] + rng.integers(0, 256, size=lit, dtype=np.uint8).tobytes() + head[20:28] + bytes(range(200, 216))


def match_input(match_len: int, seed: int) -> bytes:
    """a random run of 100 + match_len bytes, one separating byte, the run's first match_len bytes again, then 16 bytes that end the
    match and keep it clear of the block's end"""
    rng = np.random.default_rng(SEED + 200 + seed)
    run = rng.integers(0, 256, size=100 + match_len, dtype=np.uint8).tobytes()
    sep = bytes([run[0] ^ 0x55])
    stop = bytes([run[match_len] ^ 0xFF]) + bytes(range(230, 245))
    return run + sep + run[:match_len] + stop


def seeded(builder, length: int, wanted):
    """the builder's input of the first seed whose sequences -- by the restated rule -- satisfy `wanted` (two random words may share a
    table slot, and the later one then hides the earlier: the seed is chosen, not the rule bent)"""
    for seed in range(50):
        data = builder(length, seed)
        if wanted(encode(data)[1]):
            return data
    raise AssertionError(f"no seed gives the wanted sequences at length {length}")


# ---- files ----------------------------------------------------------------------------------------------------------------------------
def i64_schema(nullable=False):
    return pa.schema([pa.field("k", pa.int64(), nullable=nullable)])


def i64_batch(values, nullable=False, mask=None):
    return pa.RecordBatch.from_arrays([pa.array(np.asarray(values, dtype=np.int64), type=pa.int64(), mask=mask)], schema=i64_schema(nullable))


def shapes():
    """[(name, schema, batch, page_rows, dictionary)]: one column each, page_rows chosen so that the column is one page unless the name
    says otherwise"""
    rng = np.random.default_rng(SEED + 1)
    out = [("zeros", i64_schema(), i64_batch(np.zeros(5000)), 8192, 0)]
    for p in L.PERIODS:
        v = L._period(p, rng)
        out.append((f"period-{p}", i64_schema(), i64_batch(v), 16384 if p > 256 else 1024, 0))
    out.append(("arange", i64_schema(), i64_batch(np.arange(20000)), 32768, 0))
    out.append(("random", i64_schema(), i64_batch(rng.integers(-2**62, 2**62, size=5000)), 8192, 0))
    out.append(("single", i64_schema(), i64_batch([-7]), 64, 0))
    half = rng.integers(-2**62, 2**62, size=9000)
    out.append(("far-repeat", i64_schema(), i64_batch(np.concatenate([half, half])), 32768, 0))
    mask = rng.random(3000) < 0.3
    out.append(("nullable", i64_schema(True), i64_batch(np.arange(3000) % 11, True, mask), 4096, 0))
    bs = pa.schema([pa.field("b", pa.bool_(), nullable=False)])
    out.append(("bool-mod-3", bs, pa.RecordBatch.from_arrays([pa.array(np.arange(5000) % 3 == 0)], schema=bs), 8192, 0))
    words = [f"word-{i % 97:03d}-{'x' * (i % 13)}" for i in range(4000)]
    us = pa.schema([pa.field("s", pa.string(), nullable=False)])
    ub = pa.RecordBatch.from_arrays([pa.array(words, type=pa.string())], schema=us)
    out.append(("utf8-plain", us, ub, 4096, 0))
    out.append(("utf8-dict-pages-of-1024", us, ub, 1024, 1 << 12))
    return out


def fallback_batches():
    """under dictionary = 4: three values, then three new ones (the chunk falls back to PLAIN mid-chunk), then only old ones"""
    import parquet_dict_write_cases as D
    mk = D.decision_batch
    return D.DECISION_SCHEMA, [mk([1, 2, 3] * 30), mk([4, 5, 6] * 30), mk([1, 2, 3] * 30)]


def check_file(path: str, schema: pa.Schema, batches, report: dict, row_group_rows: int = W.DEFAULT_ROW_GROUP_ROWS, page_rows: int = W.DEFAULT_PAGE_ROWS, what=""):
    """a file written under compression = 7 three ways: pyarrow reads back the table that went in, bit for bit; pyarrow's metadata names
    the codec as it does for the files of parquet_lz4_cases.py, both totals with the page headers in them; the program's report (the
    library's reader headers: walk_headers -> inflate_page -> body pass) decoded what went in.  Returns the report's pages, flat."""
    want = pa.Table.from_batches(batches, schema=schema)
    assert report["code"] == 0 and report["reader_code"] == 0 and report["mismatch"] == "", (what, {k: report[k] for k in report if k != "row_groups"})
    assert report["bytes"] == os.path.getsize(path) and report["num_rows"] == want.num_rows, what
    f = pq.ParquetFile(path)
    W.assert_same_table(f.read(), want, what)
    md = f.metadata
    pages = W.expected_pages([b.num_rows for b in batches], row_group_rows, page_rows)
    assert md.num_rows == want.num_rows and md.num_row_groups == len(pages) == len(report["row_groups"]), (what, md.num_row_groups, len(pages))
    flat = []
    for g, group in enumerate(pages):
        mg = md.row_group(g)
        assert mg.num_rows == sum(group), (what, g)
        for c, field in enumerate(schema):
            mc, rc = mg.column(c), report["row_groups"][g]["chunks"][c]
            where = (what, field.name, g)
            assert mc.compression == "LZ4" and rc["codec_id"] == LZ4_RAW, (where, mc.compression)
            data = [p for p in rc["pages"] if p["type"] == 0]
            assert len(data) == len(group) and len(rc["pages"]) == len(data) + (1 if rc["has_dict"] else 0), where
            assert mc.has_dictionary_page == rc["has_dict"], where
            # both totals include the page headers
            assert mc.total_compressed_size == rc["total_compressed_size"] == sum(p["header_len"] + p["compressed"] for p in rc["pages"]), where
            assert mc.total_uncompressed_size == rc["total_uncompressed_size"] == sum(p["header_len"] + p["uncompressed"] for p in rc["pages"]), where
            assert all(p["compressed"] <= bound(p["uncompressed"]) and p["compressed"] >= 1 for p in rc["pages"]), where
            assert mc.num_values == mg.num_rows and mc.physical_type == W.PHYSICAL[W.DTYPES[field.type]], where
            flat += rc["pages"]
    assert report["encoder"]["sequences"] == report["decoder"]["sequences"] == sum(p["sequences"] for p in flat), what
    assert report["encoder"]["lit_extensions"] == report["decoder"]["lit_extensions"], what
    assert report["encoder"]["match_extensions"] == report["decoder"]["match_extensions"], what
    return flat
