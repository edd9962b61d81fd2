"""Speed probe of the Parquet source (deviation D12).  Generates a table on the host -- an Int64 key with 10^6 distinct values, a
Float64 value and an 11-byte Utf8 column of about 10^3 distinct strings --, writes it uncompressed with pyarrow, once
dictionary-encoded and once PLAIN, and reports per file
  (a) the whole scan by wall clock (pread, H2D, page-header walk, kernels; every batch drained on the device), as bytes of FILE
      per second, to be read against the PCIe H2D rate of about 53 GB/s of link and against pyarrow.parquet.read_table on the host,
  (b) the kernels alone (the library's HIP-event profiler: `parquet`, plus the scan and the Utf8 gather of string columns),
  (c) SUM(v) GROUP BY k, which needs 2 of the 3 columns: the chunk bytes copied (projection push-down) and the wall clock,
and the counters that witness the paths.  With --compression LZ4 the files are written LZ4_RAW-compressed and every leg also reports
  (d) the inflate kernel alone (profiler entry `parquet_inflate`): its time and its rate in bytes of inflated IMAGE per second, to
      be read against the same link rate.  One wave inflates one page, so the rate depends on the pages per chunk, which are printed.
usage: parquet_probe.py [rows, default 2^23] [rg=<rows per row group>, default 2^21] [dir=<directory>, default /dev/shm or the temp directory]
                        [--compression {NONE,LZ4}, default NONE]"""
import os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
from datafusion_archive_amd import execution as ex
from datafusion_archive_amd.logicalplan import AggregateFunction, Column, DataType
argv = list(sys.argv)
compression = "NONE"
for i, a in enumerate(argv):
    if a == "--compression" or a.startswith("--compression="):
        compression = a.split("=", 1)[1] if "=" in a else argv[i + 1]
        del argv[i:i + (1 if "=" in a else 2)]
        break
if compression not in ("NONE", "LZ4"):
    sys.exit("--compression takes NONE or LZ4")
sys.argv = argv
rows = int(float(sys.argv[1])) if len(sys.argv) > 1 and "=" not in sys.argv[1] else 1 << 23
rg = 1 << 21
out_dir = "/dev/shm" if os.path.isdir("/dev/shm") and os.access("/dev/shm", os.W_OK) else tempfile.gettempdir()
for kv in sys.argv[1:]:
    if kv.startswith("rg="): rg = int(float(kv[3:]))
    if kv.startswith("dir="): out_dir = kv[4:]
ex.init(0)
rng = np.random.default_rng(23)
names = pa.array([f"name-{i:06d}" for i in rng.choice(10 ** 6, 1000, replace=False)], pa.string())  # 11 bytes each
schema = pa.schema([pa.field("k", pa.int64(), False), pa.field("v", pa.float64(), False), pa.field("s", pa.string(), False)])
table = pa.Table.from_arrays([pa.array(rng.integers(0, 10 ** 6, rows)), pa.array(rng.normal(0.0, 1e3, rows)),
                              names.take(pa.array(rng.integers(0, len(names), rows, dtype=np.int32)))], schema=schema)
COUNTERS = ["parquet_chunk_bytes", "parquet_pages", "parquet_dict_pages", "parquet_plain_pages", "parquet_rle_runs", "parquet_bitpacked_runs",
            "parquet_host_walked_strings"]
if compression == "LZ4":
    COUNTERS += ["parquet_inflated_pages", "parquet_stored_pages", "parquet_inflated_bytes", "parquet_lz4_sequences", "parquet_inflated_bytes_to_host"]


for label, use_dict in (("dictionary", True), ("plain", False)):
    path = os.path.join(out_dir, f"dfx_parquet_probe_{label}_{compression.lower()}.parquet")
    label = label if compression == "NONE" else f"{label}, {compression}"
    try:
        pq.write_table(table, path, compression=compression, use_dictionary=use_dict, row_group_size=rg)
        size = os.path.getsize(path)
        t0 = time.perf_counter()
        pq.read_table(path)
        host = time.perf_counter() - t0
        scan = lambda: ex.drain_on_device(ex.ParquetDataSource(path))
        scan()  # warm: pools, pinned buffers, page cache
        ex.synchronize()
        reps = 3
        t0 = time.perf_counter()
        for _ in range(reps): scan()
        ex.synchronize()
        wall = (time.perf_counter() - t0) / reps
        ex.counter_reset(); ex.profile_reset(); ex.profile_enable(True)
        scan()
        ex.profile_enable(False)
        prof = {p["kernel"]: p for p in ex.profile_snapshot()}
        counters = {k: ex.counter_get(k) for k in COUNTERS}
        k_ms = sum(prof[k]["total_ms"] for k in ("parquet_inflate", "parquet", "scan", "gather_utf8") if k in prof)

        def query():
            src = ex.ParquetDataSource(path)
            s = src.schema()
            agg = ex.AggregateRelation(None, src, [ex.compile_scalar_expr(None, Column(0), s)],
                                       [ex.compile_expr(None, AggregateFunction("SUM", [Column(1)], DataType.Float64), s)])
            return agg.next().num_rows
        query()
        ex.counter_reset()
        t0 = time.perf_counter()
        groups = query()
        q_wall = time.perf_counter() - t0
        q_bytes = ex.counter_get("parquet_chunk_bytes")
        print(f"parquet probe [{label}]: rows={rows} row groups of {rg}, file {size} bytes ({size / rows:.1f} per row)")
        print(f"  whole scan (wall clock, mean of {reps}): {wall * 1e3:.1f} ms = {size / wall / 1e9:.2f} GB/s of file   "
              f"[pyarrow.parquet.read_table on the host: {host * 1e3:.1f} ms; PCIe H2D: about 53 GB/s of link]")
        print(f"  kernels (parquet {prof['parquet']['total_ms']:.3f} ms in {prof['parquet']['launches']} launches, + scan / Utf8 gather): {k_ms:.3f} ms = "
              f"{size / (k_ms * 1e-3) / 1e9:.1f} GB/s of file")
        if compression != "NONE":
            inf = prof["parquet_inflate"]
            image, chunks = counters["parquet_inflated_bytes"], 3 * ((rows + rg - 1) // rg)
            print(f"  inflate kernel alone: {inf['total_ms']:.3f} ms in {inf['launches']} launches = {image / (inf['total_ms'] * 1e-3) / 1e9:.2f} GB/s of inflated image "
                  f"({image} bytes; one wave per page: {counters['parquet_inflated_pages'] + counters['parquet_stored_pages']} pages in {chunks} chunks, "
                  f"{(counters['parquet_inflated_pages'] + counters['parquet_stored_pages']) / chunks:.0f} per chunk)   [PCIe H2D: about 53 GB/s of link]")
        print(f"  SUM(v) GROUP BY k ({groups} groups): {q_wall * 1e3:.1f} ms, {q_bytes} of {size} bytes copied ({100.0 * q_bytes / size:.0f} %)")
        print(f"  counters: {counters}")
    finally:
        if os.path.exists(path): os.remove(path)
