"""Kernel-time probe of Utf8 string terms (deviation D9) over a resident table of short strings: ~1000 city-like names of 4-20
bytes plus an Int32 `code` column holding each name's index.  Timed by the library's HIP-event profiler:
  (a) the term kernel alone (`utf8_pred`) for Eq, Lt, prefix-LIKE and contains-LIKE, as a fraction of the 8 TB/s roofline over
      the bytes the term must read: 4 B per row of offsets + the data bytes of the rows it has to look at (all of them for
      ordered and LIKE terms, only the rows of the literal's length for Eq);
  (b) the whole FilterRelation with the one-term predicate, compacted batches left on the device;
  (c) for scale, WHERE code = k on the Int32 column through the existing path.
usage: utf8_pred_probe.py [rows, default 2^27] [batch=<rows>]"""
import os, random, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import pyarrow as pa
from datafusion_archive_amd import execution as ex
from datafusion_archive_amd.logicalplan import *
rows = int(float(sys.argv[1])) if len(sys.argv) > 1 else 1 << 27
batch = 1 << 27
for kv in sys.argv[2:]:
    k, v = kv.split("=")
    if k == "batch": batch = int(v)
    else: ex.set_option(k, int(v))
ex.init(0)
r = random.Random(9)
names = sorted({"".join(r.choice("abcdefghijklmnopqrstuvwxyz") for _ in range(r.randrange(4, 17))).capitalize() + r.choice(["", ", UK"]) for _ in range(1000)})
lens = np.array([len(s.encode()) for s in names])
schema = pa.schema([pa.field("city", pa.string(), False), pa.field("code", pa.int32(), False)])
rng = np.random.default_rng(9)
pieces, piece = [], 1 << 24
name_arr = pa.array(names, pa.string())
hist = np.zeros(len(names), dtype=np.int64)
for a in range(0, rows, piece):
    codes = rng.integers(0, len(names), min(piece, rows - a), dtype=np.int32)
    hist += np.bincount(codes, minlength=len(names))
    pieces.append(pa.RecordBatch.from_arrays([name_arr.take(pa.array(codes)), pa.array(codes)], schema=schema))
t = ex.DeviceTable.from_batches(schema, pieces)
del pieces
data_bytes = float((hist * lens).sum())
k = len(names) // 2
lit = lambda s: Literal(ScalarValue.Utf8(s))
cases = [("Eq", BinaryExpr(Column(0), Operator.Eq, lit(names[k])), float((hist * lens)[lens == lens[k]].sum())),
         ("Lt", BinaryExpr(Column(0), Operator.Lt, lit(names[k])), data_bytes),
         ("prefix LIKE", BinaryExpr(Column(0), Operator.Like, lit(names[k][:2] + "%")), data_bytes),
         ("contains LIKE", BinaryExpr(Column(0), Operator.Like, lit("%" + names[k][1:4] + "%")), data_bytes),
         ("code = k", BinaryExpr(Column(1), Operator.Eq, Literal(ScalarValue.Int32(k))), None)]
print(f"utf8 term probe: rows={rows} batch={batch} names={len(names)} of {lens.min()}-{lens.max()} bytes, {data_bytes / rows:.2f} data bytes per row")
for what, pred, must_read in cases:
    def run():
        rel = ex.FilterRelation(t.scan(batch), ex.compile_scalar_expr(None, pred, schema), schema)
        return ex.drain_on_device(rel)[0]
    kept = run(); ex.synchronize()
    t0 = time.perf_counter()
    for _ in range(5): run()
    ex.synchronize()
    dt = (time.perf_counter() - t0) / 5
    ex.profile_reset(); ex.profile_enable(True)
    for _ in range(3): run()
    ex.profile_enable(False)
    prof = {p["kernel"]: p for p in ex.profile_snapshot()}
    line = f"  {what:14s} kept={kept} ({kept / rows:.4f}): FilterRelation {dt * 1e3:.3f} ms per pass = {rows / dt / 1e9:.2f} G rows/s"
    if must_read is not None and "utf8_pred" in prof:
        ms = prof["utf8_pred"]["total_ms"] / 3
        b = 4.0 * rows + must_read
        line += f"; utf8_pred {ms:.3f} ms over {b / 1e9:.2f} GB it must read = {b / (ms * 1e-3) / 1e12:.2f} TB/s ({b / (ms * 1e-3) / 8e12:.3f} of 8 TB/s)"
    print(line)
    print("     " + "  ".join(f"{p['kernel']}:{p['launches'] // 3}x{p['total_ms'] / p['launches'] * 1e3:.1f}us" for p in ex.profile_snapshot()))
