"""Speed probe of the Parquet writer (deviation D13) over the resident table of tools/csv_write_probe.py: two Float64 columns, one
Int64 column and one Utf8 column of 4-20 bytes, all REQUIRED (a second run: the same columns OPTIONAL with one null row in eight).
Reports bytes of FILE per second
  (a) of the kernels alone (measure + scan + encode, the library's HIP-event profiler: `parquet_write`),
  (b) of the whole dfx_parquet_write call by wall clock (kernels, the page-table read-back, D2H into pinned buffers, fwrite),
  (c) of dfx_csv_write over the same table (bytes of text), and
  (d) of pyarrow.parquet.write_table(compression="NONE", use_dictionary=False) of the same table on the host.
Single runs on a shared machine: no threshold is derived from them and no test times anything.
usage: parquet_write_probe.py [rows, default 2^24] [out=<directory>, default /dev/shm or the temp directory]"""
import os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
from datafusion_archive_amd import execution as ex
rows = int(float(sys.argv[1])) if len(sys.argv) > 1 and "=" not in sys.argv[1] else 1 << 24
out_dir = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else tempfile.gettempdir()
for kv in sys.argv[1:]:
    if kv.startswith("out="): out_dir = kv[4:]
out = os.path.join(out_dir, "dfx_parquet_write_probe.out")
COUNTERS = ["parquet_write_pages", "parquet_write_row_groups", "parquet_write_rle_level_pages", "parquet_write_bitpacked_level_pages"]
ex.init(0)


def table(nullable):
    rng = np.random.default_rng(17)
    names = np.array(["".join(chr(97 + int(c)) for c in rng.integers(0, 26, int(n))) for n in rng.integers(4, 21, 4096)])
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


try:
    import pyarrow.compute  # noqa: F401
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
