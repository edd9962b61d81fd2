"""Speed probe of the CSV writer (deviation D11) over a resident table: two Float64 columns, one Int64 column and one Utf8 column
of 4-20 bytes.  Reports bytes of TEXT per second
  (a) of the kernels alone (format + assemble, the library's HIP-event profiler: `csv_write`), to be read against the reader's
      850 GB/s of text, its mirror on the device, and
  (b) of the whole dfx_csv_write call by wall clock (kernels, D2H through the pinned staging buffers, fwrite), to be read
      against the PCIe D2H rate of the text (about 53 GB/s of link).
The single-core host rate of the same formatter is what tests/native/numfmt_fuzz.cpp prints.
usage: csv_write_probe.py [rows, default 2^24] [out=<file>, default /dev/shm or the temp directory]"""
import os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import pyarrow as pa
from datafusion_archive_amd import execution as ex
rows = int(float(sys.argv[1])) if len(sys.argv) > 1 and "=" not in sys.argv[1] else 1 << 24
out_dir = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else tempfile.gettempdir()
out = os.path.join(out_dir, "dfx_csv_write_probe.csv")
for kv in sys.argv[1:]:
    if kv.startswith("out="): out = kv[4:]
ex.init(0)
rng = np.random.default_rng(17)
names = np.array(["".join(chr(97 + int(c)) for c in rng.integers(0, 26, int(n))) for n in rng.integers(4, 21, 4096)])
schema = pa.schema([pa.field("x", pa.float64(), False), pa.field("y", pa.float64(), False), pa.field("k", pa.int64(), False), pa.field("s", pa.string(), False)])
pieces, piece = [], 1 << 22
name_arr = pa.array(names, pa.string())
for a in range(0, rows, piece):
    n = min(piece, rows - a)
    pieces.append(pa.RecordBatch.from_arrays([pa.array(rng.normal(0.0, 1e3, n)), pa.array(rng.random(n)), pa.array(rng.integers(-2 ** 40, 2 ** 40, n)),
                                              name_arr.take(pa.array(rng.integers(0, len(names), n, dtype=np.int32)))], schema=schema))
t = ex.DeviceTable.from_batches(schema, pieces)
del pieces
run = lambda: ex.write_csv(t.scan(0), out)
try:
    got_rows, nbytes = run()  # warm: pools, pinned buffers, page cache of the target
    ex.synchronize()
    reps = 3
    t0 = time.perf_counter()
    for _ in range(reps): run()
    wall = (time.perf_counter() - t0) / reps
    ex.profile_reset(); ex.profile_enable(True)
    run()
    ex.profile_enable(False)
    prof = {p["kernel"]: p for p in ex.profile_snapshot()}
    k_ms = prof["csv_write"]["total_ms"]
    print(f"csv write probe: rows={got_rows} text={nbytes} bytes ({nbytes / got_rows:.1f} per row, {4 * got_rows} cells) -> {out}")
    print(f"  kernels (format + assemble, {prof['csv_write']['launches']} launches): {k_ms:.3f} ms = {nbytes / (k_ms * 1e-3) / 1e9:.1f} GB/s of text, "
          f"{4 * got_rows / (k_ms * 1e-3) / 1e9:.2f} G cells/s   [the reader: 850 GB/s of text]")
    print(f"  whole call (wall clock, mean of {reps}): {wall * 1e3:.1f} ms = {nbytes / wall / 1e9:.2f} GB/s of text   [PCIe D2H of the text: about 53 GB/s of link]")
    print(f"  general-path tiles: {ex.counter_get('csv_write_general_tiles')}")
finally:
    if os.path.exists(out): os.remove(out)
