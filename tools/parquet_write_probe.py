"""Speed probe of the Parquet writer (deviation D13) over the resident table of tools/csv_write_probe.py: two Float64 columns, one
Int64 column and one Utf8 column of 4-20 bytes, all REQUIRED (a second run: the same columns OPTIONAL with one null row in eight).
Reports bytes of FILE per second
  (a) of the kernels alone (measure + scan + encode, the library's HIP-event profiler: `parquet_write`),
  (b) of the whole dfx_parquet_write call by wall clock (kernels, the page-table read-back, D2H into pinned buffers, fwrite),
  (c) of dfx_csv_write over the same table (bytes of text), and
  (d) of pyarrow.parquet.write_table(compression="NONE", use_dictionary=False) of the same table on the host.
With `--dictionary N` it probes the "dictionary" option instead: the same two tables and a third whose Utf8 column draws from 10^3
distinct strings, each written without the option and with dictionary = N -- file bytes, kernel time, the whole call, and the time the
library's own Parquet source takes to scan each of the two files.
Single runs on a shared machine: no threshold is derived from them and no test times anything.
With `--host-encoder EXE` (beside `--dictionary N`; needs no GPU) it writes the same three seeded tables with the sequential host encoder
instead -- EXE is tests/native/parquet_dict_write_check.cpp built -- and prints the file sizes the device's files must have.
With `--compression 7` it probes the "compression" option: the two tables written without the option and with it (beside
`--dictionary N`: both with the dictionary) -- file bytes, the time of the `parquet_write` kernels and of the `parquet_write_lz4`
kernels, the whole call, the option's counters, and the scan of each file by the library's own Parquet source.
usage: parquet_write_probe.py [rows, default 2^24] [out=<directory>, default /dev/shm or the temp directory] [--dictionary N [--host-encoder EXE]] [--compression 7]"""
import os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
from datafusion_archive_amd import execution as ex
dictionary = 0
if "--dictionary" in sys.argv:
    at = sys.argv.index("--dictionary")
    dictionary = int(sys.argv[at + 1])
    del sys.argv[at:at + 2]
compression = 0
if "--compression" in sys.argv:
    at = sys.argv.index("--compression")
    compression = int(sys.argv[at + 1])
    del sys.argv[at:at + 2]
host_encoder = None
if "--host-encoder" in sys.argv:
    at = sys.argv.index("--host-encoder")
    host_encoder = sys.argv[at + 1]
    del sys.argv[at:at + 2]
rows = int(float(sys.argv[1])) if len(sys.argv) > 1 and "=" not in sys.argv[1] else 1 << 24
out_dir = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else tempfile.gettempdir()
for kv in sys.argv[1:]:
    if kv.startswith("out="): out_dir = kv[4:]
out = os.path.join(out_dir, "dfx_parquet_write_probe.out")
COUNTERS = ["parquet_write_pages", "parquet_write_row_groups", "parquet_write_rle_level_pages", "parquet_write_bitpacked_level_pages"]
if host_encoder is None: ex.init(0)


def table(nullable, distinct=4096):
    rng = np.random.default_rng(17)
    names = np.array(["".join(chr(97 + int(c)) for c in rng.integers(0, 26, int(n))) for n in rng.integers(4, 21, distinct)])
    schema = pa.schema([pa.field("x", pa.float64(), nullable), pa.field("y", pa.float64(), nullable), pa.field("k", pa.int64(), nullable), pa.field("s", pa.string(), nullable)])
    pieces, piece = [], 1 << 22
    name_arr = pa.array(names, pa.string())
    for a in range(0, rows, piece):
        n = min(piece, rows - a)
        cols = [pa.array(rng.normal(0.0, 1e3, n)), pa.array(rng.random(n)), pa.array(rng.integers(-2 ** 40, 2 ** 40, n)),
                name_arr.take(pa.array(rng.integers(0, len(names), n, dtype=np.int32)))]
        if nullable:
            mask = pa.array(rng.integers(0, 8, n) != 0)
            cols = [pa.compute.if_else(mask, c, pa.scalar(None, c.type)) for c in cols]
        pieces.append(pa.RecordBatch.from_arrays(cols, schema=schema))
    return schema, pieces


def timed(run, reps=3):
    run()  # warm: pools, pinned buffers, page cache of the target
    ex.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps): run()
    return (time.perf_counter() - t0) / reps


DICT_COUNTERS = ["parquet_write_dict_pages", "parquet_write_dict_entries", "parquet_write_dict_index_pages", "parquet_write_dict_rle_index_pages",
                 "parquet_write_dict_fallback_chunks"]


DICT_TABLES = (("REQUIRED", False, 4096), ("OPTIONAL, one null in eight", True, 4096), ("REQUIRED, Utf8 of 10^3 distinct strings", False, 1000))


def host_sizes():
    """the three tables through the sequential host encoder, in the batches the resident table hands out (scan(0): one batch per piece)"""
    import json, subprocess
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    import parquet_write_cases as W
    for what, nullable, distinct in DICT_TABLES:
        schema, pieces = table(nullable, distinct)
        desc = out + ".desc"
        with open(desc, "wb") as fh: fh.write(W.describe(schema, pieces))
        print(f"host encoder ({what}): rows={rows}")
        for n in (0, dictionary):
            r = subprocess.run([host_encoder, "write", desc, out, str(n)], capture_output=True, text=True)
            report = json.loads(r.stdout)
            assert r.returncode == 0 and report["code"] == 0 and report["reader_code"] == 0 and report["mismatch"] == "", (r.returncode, r.stderr[-500:])
            print(f"  options { {'dictionary': n} if n else 'none'}: file={report['bytes']} bytes")
        os.remove(desc)


def probe_dictionary():
    for what, nullable, distinct in DICT_TABLES:
        schema, pieces = table(nullable, distinct)
        t = ex.DeviceTable.from_batches(schema, pieces)
        del pieces
        print(f"parquet write dictionary probe ({what}): rows={rows}")
        for options in ({}, {"dictionary": dictionary}):
            run = lambda: ex.write_parquet(t.scan(0), out, options)
            wall = timed(run)
            ex.profile_reset(); ex.profile_enable(True); ex.counter_reset()
            _, nbytes = run()
            ex.profile_enable(False)
            prof = {p["kernel"]: p for p in ex.profile_snapshot()}["parquet_write"]
            counters = {k: ex.counter_get(k) for k in COUNTERS + DICT_COUNTERS}
            def scan():
                for _ in ex.ParquetDataSource(out): pass
            scan_wall = timed(scan)
            print(f"  options {options or 'none'}: file={nbytes} bytes ({nbytes / rows:.1f} per row); kernels ({prof['launches']} tracked launches) {prof['total_ms']:.3f} ms; "
                  f"whole call (mean of 3) {wall * 1e3:.1f} ms; scan of the file by the Parquet source (mean of 3) {scan_wall * 1e3:.1f} ms")
            print(f"    counters: {counters}")
        del t


LZ4_COUNTERS = ["parquet_write_lz4_pages", "parquet_write_lz4_bytes_in", "parquet_write_lz4_bytes_out", "parquet_write_lz4_sequences"]


def probe_compression():
    base = {"dictionary": dictionary} if dictionary > 0 else {}
    for what, nullable, distinct in DICT_TABLES[:2]:
        schema, pieces = table(nullable, distinct)
        t = ex.DeviceTable.from_batches(schema, pieces)
        del pieces
        print(f"parquet write compression probe ({what}): rows={rows}")
        for options in (dict(base), dict(base, compression=compression)):
            run = lambda: ex.write_parquet(t.scan(0), out, options)
            wall = timed(run)
            ex.profile_reset(); ex.profile_enable(True); ex.counter_reset()
            _, nbytes = run()
            ex.profile_enable(False)
            prof = {p["kernel"]: p for p in ex.profile_snapshot()}
            counters = {k: ex.counter_get(k) for k in COUNTERS + LZ4_COUNTERS}
            def scan():
                for _ in ex.ParquetDataSource(out): pass
            scan_wall = timed(scan)
            lz4_ms = prof["parquet_write_lz4"]["total_ms"] if "parquet_write_lz4" in prof else 0.0
            print(f"  options {options or 'none'}: file={nbytes} bytes ({nbytes / rows:.1f} per row); kernels parquet_write {prof['parquet_write']['total_ms']:.3f} ms, "
                  f"parquet_write_lz4 {lz4_ms:.3f} ms; whole call (mean of 3) {wall * 1e3:.1f} ms; scan of the file by the Parquet source (mean of 3) {scan_wall * 1e3:.1f} ms")
            print(f"    counters: {counters}")
        del t


try:
    import pyarrow.compute  # noqa: F401
    if compression > 0:
        probe_compression()
        sys.exit(0)
    if dictionary > 0:
        host_sizes() if host_encoder else probe_dictionary()
        sys.exit(0)
    for nullable in (False, True):
        schema, pieces = table(nullable)
        t = ex.DeviceTable.from_batches(schema, pieces)
        host = pa.Table.from_batches(pieces, schema=schema)
        del pieces
        run = lambda: ex.write_parquet(t.scan(0), out)
        wall = timed(run)
        ex.profile_reset(); ex.profile_enable(True); ex.counter_reset()
        got_rows, nbytes = run()
        ex.profile_enable(False)
        prof = {p["kernel"]: p for p in ex.profile_snapshot()}
        k_ms = prof["parquet_write"]["total_ms"]
        print(f"parquet write probe ({'OPTIONAL, one null in eight' if nullable else 'REQUIRED'}): rows={got_rows} file={nbytes} bytes ({nbytes / got_rows:.1f} per row) -> {out}")
        print(f"  kernels (measure + scan + encode, {prof['parquet_write']['launches']} tracked launches): {k_ms:.3f} ms = {nbytes / (k_ms * 1e-3) / 1e9:.1f} GB/s of file")
        print(f"  whole call (wall clock, mean of 3): {wall * 1e3:.1f} ms = {nbytes / wall / 1e9:.2f} GB/s of file   [PCIe D2H: about 53 GB/s of link]")
        print(f"  counters: { {k: ex.counter_get(k) for k in COUNTERS} }")
        csv_bytes = [0]
        def run_csv(): csv_bytes[0] = ex.write_csv(t.scan(0), out)[1]
        wall = timed(run_csv)
        print(f"  dfx_csv_write of the same table: {csv_bytes[0]} bytes of text, {wall * 1e3:.1f} ms = {csv_bytes[0] / wall / 1e9:.2f} GB/s of text")
        run_pa = lambda: pq.write_table(host, out, compression="NONE", use_dictionary=False)
        wall = timed(run_pa, reps=1)
        print(f"  pyarrow.parquet.write_table(compression='NONE', use_dictionary=False) on the host: {os.path.getsize(out)} bytes, {wall * 1e3:.1f} ms = "
              f"{os.path.getsize(out) / wall / 1e9:.2f} GB/s of file")
        del t, host
finally:
    if os.path.exists(out): os.remove(out)
