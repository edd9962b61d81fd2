#!/usr/bin/env python3
"""bench.py -- rows/sec of filter + GROUP-BY-SUM over Float64 Arrow on MI355X (BASELINE.json metric).

One "step" = one pass of the hot path over the whole HBM-resident synthetic table:

    SELECT k, SUM(v) FROM t WHERE v > 204.8 AND v < 409.6 GROUP BY k

  t: N rows (default 1e9 on one GPU), k Int64 uniform in [0, 1e6) (1 M groups), v Float64 = m * 2^-10 with
  m uniform in [0, 2^20) ("exact" distribution: every partial sum is representable, so the result is
  order-independent and checked bit-exactly); the predicate keeps 20 % of the rows -- it is BASELINE
  config 2's `lat > 51 AND lat < 53` shape applied to config 3's table.  Algorithmic traffic 16 B/row.
  The operator tree is the reference's: TableScan -> FilterRelation -> AggregateRelation, driven through
  the C ABI; the library fuses Filter into the aggregate kernel.  The timed region starts with the table
  resident in HBM and ends when the result RecordBatch is back on the host.

Multi-GPU (--gpus N, launched by torch.distributed.run): BASELINE config 4 -- 1e10 rows in all, rank g owns rows
[g N/world, (g+1) N/world) (--rows overrides the per-rank count), aggregates locally, exchanges GROUP partials with one
RCCL all-to-all inside the library, merges and emits the groups it owns.  value = rows of all ranks / max-over-ranks time.
The --full line of a multi-rank run also carries config 5 (the TPC-H Q1 shape over the same row ranges) in extra.cfg5_q1_shape.

Timing: one cold step (reported as extra.cold_first_step_ms), W warm-up steps, then EXACTLY K steps between barrier +
synchronize on both sides, un-instrumented -> value / ms_per_step; with --full, K more steps with the library's HIP-event profiler
on -> the per-kernel durations of the `roofline` object (extra.instrumented_ms_per_step is that region's time).  At N=1 the
--full line also carries cpu_baseline (the C restatement of the reference on one host core, 3e8-row sample) and, in `extra`, the
other BASELINE configs that fit one GPU (config 3: no filter; config 2: the FilterRelation as written and fused with
COUNT; config 5: the Q1 shape), each with a `verified_vs_oracle` object: the same query over a 1e8-row slice through the
same product path, compared with the CPU oracle (bit for bit; config 5's uniform doubles within n * eps * sum|v|), and the
north-star size, 1e10 rows on one GPU, as extra.rows_1e10.

A plain run (no --full) does only what the headline needs: it sets up, runs the cold step and the W warm-up steps, times the
K steps, writes the outputs of the last timed step if --dump-outputs DIR is given (DIR/k.npy and DIR/sum_v.npy, float64, sorted
by key) and prints the line; `roofline` and `cpu_baseline` are null there.  --full adds everything else described above: the
plan, the instrumented region and its roofline, the sum-of-sums check, the CPU baseline, the extra legs and their checks.

Prints ONE compact JSON line (< 4 KB) on rank 0 as the last line of stdout: the contract's fields, `roofline`, `cpu_baseline`
and one {frac, ms, ok} per extra leg; the full object (every leg's description and verification record) goes to
gpurun_out/bench_extra.json and to stderr.
"""
import argparse
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_GBPS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured float4 copy)
GROUPS = 1000000
LO, HI = 204.8, 409.6


COMPACT_LINE_LIMIT = 4096  # bytes: the driver keeps the tail of stdout and parses its last line (round 5's 20 KB line came back unparsed)


def _leg_summary(leg):
    """One extra leg -> {"frac": end-to-end fraction of the 8 TB/s roofline, "ok": checked against the oracle?, "ms": step time}."""
    out = {}
    r = leg.get("roofline") if isinstance(leg.get("roofline"), dict) else None
    if r is not None and r.get("frac") is not None:
        out["frac"] = round(float(r["frac"]), 4)
    ms = leg.get("ms_per_step", leg.get("ms"))  # "ms" is the leg's whole timed region, "ms_per_step" (where present) one step of it
    if ms is not None:
        out["ms"] = round(float(ms), 3)
    v = leg.get("verified_vs_oracle")
    if v is not None:
        out["ok"] = bool(v.get("ok")) if isinstance(v, dict) else bool(v)
    if "error" in leg:
        out["error"] = str(leg["error"])[:80]
    return out


def compact_line(full, limit=COMPACT_LINE_LIMIT):
    """The line bench.py prints LAST: the contract's fields, the roofline and cpu_baseline objects without their prose, and
    one {frac, ms, ok} per extra leg.  The full object (every leg's description, its verification record, budgets, plans) goes
    to gpurun_out/bench_extra.json and to stderr.  Always shorter than `limit` bytes: legs are dropped from the end, never
    a contract field (tests/test_bench_line_contract.py)."""
    keep_roofline = ("bound", "achieved", "peak", "unit", "frac", "traffic", "traffic_over_algorithmic", "end_to_end_frac",
                     "launches", "avg_launch_ms", "algo_bytes_per_launch", "cold_first_step_ms", "frac_is", "kernel")
    line = {k: full[k] for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                                 "scaling", "vs_baseline", "dtype", "data") if k in full}
    cfg = dict(full.get("config") or {})
    line["config"] = {k: cfg[k] for k in ("workload", "rows_per_gpu", "rows_total", "batch_rows", "algorithmic_bytes_per_row",
                                          "parallelism", "exchange", "rccl_ranks") if k in cfg}
    r = full.get("roofline")
    if isinstance(r, dict):
        rr = {k: r[k] for k in keep_roofline if k in r}
        if isinstance(rr.get("kernel"), str):
            rr["kernel"] = rr["kernel"][:60]
        if isinstance(rr.get("frac_is"), str):
            rr["frac_is"] = "dominant kernel alone; whole step = end_to_end_frac"
        line["roofline"] = rr
    else:
        line["roofline"] = r
    c = full.get("cpu_baseline")
    if isinstance(c, dict):
        cc = {k: c[k] for k in ("value", "unit", "cores", "kind", "sample") if k in c}
        cc["sample"] = str(cc.get("sample", ""))[:160]
        line["cpu_baseline"] = cc
    else:
        line["cpu_baseline"] = c
    ex_full = full.get("extra") or {}
    ex = {}
    for k in ("verified_sum_of_group_sums_equals_ungrouped_sum", "groups", "selectivity", "cold_first_step_ms", "scaling_anchor_rows_per_s"):
        if k in ex_full:
            v = ex_full[k]
            ex[k] = round(v, 3) if isinstance(v, float) else v
    if isinstance(ex_full.get("verified_vs_oracle"), dict):
        v = ex_full["verified_vs_oracle"]
        ex["verified_vs_oracle"] = {k: v[k] for k in ("rows", "groups", "ok") if k in v}
    if isinstance(ex_full.get("phases_ms"), dict):
        ex["phases_ms"] = ex_full["phases_ms"]
    legs = [(k, v) for k, v in ex_full.items() if isinstance(v, dict) and ("roofline" in v or "error" in v) and k != "verified_vs_oracle"]
    # the legs the review reads first stay when the line has to shrink
    first = ["rows_1e10", "cfg3_groupby_sum_no_filter", "cfg4_as_written", "cfg5_q1_shape", "headline_selectivity_50", "headline_selectivity_80",
             "headline_through_interpreter", "different_operand_sum_min", "cfg2_filter_mask_and_compact", "cfg2_predicate_count"]
    legs.sort(key=lambda kv: first.index(kv[0]) if kv[0] in first else len(first))
    line["extra"] = ex
    line["extra_full"] = "gpurun_out/bench_extra.json"
    ex["legs"] = {}
    for k, v in legs:
        ex["legs"][k] = _leg_summary(v)
        if len(json.dumps(line, separators=(",", ":"))) > limit - 64:
            del ex["legs"][k]
            ex["legs_dropped"] = len(legs) - len(ex["legs"])
            break
    return line


def emit_line(full, full_out=None):
    """Full object -> gpurun_out/bench_extra.json (or --full-out) + stderr; compact object -> the LAST line of stdout."""
    text = json.dumps(full)
    path = full_out or os.path.join(ROOT, "gpurun_out", "bench_extra.json")
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as fh:
            fh.write(text + "\n")
    except OSError:
        pass
    print("bench.py full line: " + text, file=sys.stderr, flush=True)
    out = json.dumps(compact_line(full), separators=(",", ":"))
    assert len(out) < COMPACT_LINE_LIMIT, len(out)
    print(out, flush=True)


def dump_outputs(result, out_dir, suffix=""):
    """The result batch of the timed query -> out_dir/k<suffix>.npy and out_dir/sum_v<suffix>.npy, float64, sorted by key (the
    order the groups leave the device in is unspecified; the keys are < 2^53, so float64 holds them exactly).  10^6 groups = 16 MB."""
    import numpy as np
    k = result.column(0).to_numpy(zero_copy_only=False)
    s = result.column(1).to_numpy(zero_copy_only=False)
    o = np.argsort(k, kind="stable")
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, f"k{suffix}.npy"), k[o].astype(np.float64))
    np.save(os.path.join(out_dir, f"sum_v{suffix}.npy"), s[o].astype(np.float64))


def host_cpu_budget():
    """CPUs this process may actually keep busy: the cgroup's quota when there is one (a box that shows 256 cores to
    os.cpu_count() may grant a container far fewer -- and throttles EVERY thread of the container, the one that drives the GPU
    included, for the rest of the scheduling period once the quota is spent), else the affinity mask."""
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            return max(1, int(int(quota) / int(period)))
    except Exception:
        pass
    try:
        return len(os.sched_getaffinity(0))
    except Exception:
        return os.cpu_count() or 1


class Background:
    """One oracle query on a host thread of its own (the C code holds no global state, ctypes releases the GIL).  At most
    `Background.slots` of them run at a time -- the others wait their turn -- so that the oracle runs beside the timed GPU
    legs never use up the container's CPU quota (round 5: with one thread per query, twenty of them, one or another of the
    host-latency-bound legs came out a third slower in every run, never the same one)."""
    slots = threading.Semaphore(max(2, min(6, host_cpu_budget() - 4)))  # (round 6: six, not ten -- on a box with a slower host ten oracle threads still cost
    # the host-latency-bound legs a third: FilterRelation 0.58 -> 0.39, the 10^10-row leg 0.53 -> 0.48, profiles/r06_bench_line_slow_host_box.json)

    def __init__(self, fn, *args, **kw):
        self.result, self.error = None, None

        def run():
            with Background.slots:
                try:
                    self.result = fn(*args, **kw)
                except Exception as e:  # reported in the line, never fatal
                    self.error = str(e)[:300]
        self.t = threading.Thread(target=run, daemon=True)
        self.t.start()

    def get(self):
        self.t.join()
        if self.error is not None:
            raise RuntimeError(self.error)
        return self.result


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=float, default=0.0, help="rows per GPU (default: 1e9 on one GPU; 1e10 / N on N GPUs -- BASELINE config 4)")
    ap.add_argument("--batch-rows", type=int, default=1 << 27)
    ap.add_argument("--cpu-sample-rows", type=float, default=3e8)
    ap.add_argument("--verify-rows", type=float, default=1e8, help="rows of the slice every extra configuration is checked on against the oracle")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extras", action="store_true")
    ap.add_argument("--full-out", default=None, help="where the full (uncompacted) line object is written; default gpurun_out/bench_extra.json")
    ap.add_argument("--rows-1e10-steps", type=int, default=3, help="timed steps of the north-star size (1e10 rows on one GPU); 0: skip")
    ap.add_argument("--allow-host-exchange", action="store_true",
                    help="multi-rank runs: accept the host-driven exchange (torch.distributed around dfx_aggregate_partial_*) when the library's "
                         "RCCL communicator cannot be created.  Without it such a run exits non-zero: the line of an N-GPU run is about RCCL over xGMI")
    ap.add_argument("--prewarm-steps", type=int, default=0,
                    help="extra untimed steps before the W warmup steps.  Round 1 ran 600 of them (~3.5 s) believing the first seconds of a "
                         "process are slower; round 2 measured the opposite on most boxes -- after seconds of sustained load pass 1 runs "
                         "8-10 %% slower (0.250 ms per launch against 0.229 ms in a short run on the same box, DESIGN.md section 5) -- so the "
                         "default is the contract's: W warm-up steps, then K timed ones.  The process's very first step (pools, calibration) "
                         "is reported as extra.cold_first_step_ms")
    ap.add_argument("--full", action="store_true",
                    help="everything beyond the headline: plan, instrumented region and roofline, sum-of-sums check, CPU baseline, the extra legs "
                         "and their checks against the oracle.  Without it the run times the headline query only")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write the result of the last one as DIR/k.npy and DIR/sum_v.npy (float64, sorted by key; "
                         "a rank's own groups as k_rank<r>.npy / sum_v_rank<r>.npy on N > 1 GPUs)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus and world > 1:
        args.gpus = world

    import torch  # plumbing: device selection, barrier, the all-to-all
    import torch.distributed as dist

    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (torch.cuda.is_available() is False); there is no CPU path")
    # DFX_BENCH_SHARED_GPU=1: dry run of the N-rank code path on a ONE-GPU box (every rank on cuda:0, gloo with
    # host staging instead of RCCL).  Its numbers mean nothing; it exists to test the plumbing.
    shared_gpu = os.environ.get("DFX_BENCH_SHARED_GPU") == "1"
    dev_index = 0 if shared_gpu else local_rank
    torch.cuda.set_device(dev_index)
    device = torch.device("cuda", dev_index)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if shared_gpu:
            dist.init_process_group(backend="gloo")
        else:
            dist.init_process_group(backend="nccl", device_id=device)

    import numpy as np
    import pyarrow as pa
    from datafusion_archive_amd import execution as ex
    from datafusion_archive_amd.distributed import exchange_group_partials
    from datafusion_archive_amd.logicalplan import (AggregateFunction, BinaryExpr, Column, DataType, Literal,
                                                    Operator, ScalarValue)

    ex.init(dev_index)
    for kv in filter(None, os.environ.get("DFX_BENCH_OPTIONS", "").split(",")):  # A/B runs: library options, e.g. agg.early_keys=0
        k_, v_ = kv.split("=")
        ex.set_option(k_.strip(), int(v_))
    coll_device = torch.device("cpu") if shared_gpu else device  # where the tiny bookkeeping collectives run
    info = ex.device_info()
    if args.rows > 0:
        n_rows = int(args.rows)
    else:
        n_rows = 1000000000 if world == 1 else int(10000000000 // world)  # config 4: 1e10 rows over the ranks
    seed = 0xDF02
    syn = [("k", ex.SYNTH_I64_UNIFORM, 0, float(GROUPS), 0.0), ("v", ex.SYNTH_F64_EXACT, 1, 0.0, 0.0)]
    schema = pa.schema([("k", pa.int64()), ("v", pa.float64())])
    table = ex.DeviceTable.synth(syn, seed, rank * n_rows, n_rows)  # resident in HBM before any timing

    f64 = DataType.Float64

    def l64(v):
        return Literal(ScalarValue.Float64(v))

    pred = BinaryExpr(BinaryExpr(Column(1), Operator.Gt, l64(LO)), Operator.And, BinaryExpr(Column(1), Operator.Lt, l64(HI)))
    sum_v = AggregateFunction("SUM", [Column(1)], f64)
    count_v = AggregateFunction("COUNT", [Column(1)], DataType.UInt64)

    def build_on(tbl, sch, filter_expr, group, aggs):
        rel = tbl.scan(args.batch_rows)
        if filter_expr is not None:
            rel = ex.FilterRelation(rel, ex.compile_scalar_expr(None, filter_expr, sch), sch)
        return ex.AggregateRelation(None, rel, [ex.compile_scalar_expr(None, g, sch) for g in group],
                                    [ex.compile_expr(None, a, sch) for a in aggs])

    def build(filter_expr, group, aggs):
        return build_on(table, schema, filter_expr, group, aggs)

    # multi-GPU: the exchange of group partials runs INSIDE the library over RCCL (dfx_aggregate_exchange); torch.distributed
    # only carries the communicator's 128-byte id once.  If RCCL cannot be bound / initialised on some rank, every rank
    # falls back to the host-driven exchange (torch.distributed all_to_all_single around the three device steps).
    comm = None
    exchange_mode = "single GPU"
    if world > 1:
        ok = 1
        try:
            if shared_gpu and not os.environ.get("DFX_RCCL_LIB"):
                # (with DFX_RCCL_LIB = tests/native/librccl_stub.so the library's own exchange runs between the ranks of a
                # one-GPU dry run, host-staged: plumbing only)
                raise RuntimeError("dry run: every rank on one GPU (RCCL needs one device per rank)")
            from datafusion_archive_amd.distributed import library_communicator
            comm = library_communicator(world, rank, dist)
        except Exception as e:
            ok = 0
            comm_error = str(e)[:200]
        t_ok = torch.tensor([ok], dtype=torch.int32, device=coll_device)
        dist.all_reduce(t_ok, op=dist.ReduceOp.MIN)
        if int(t_ok.item()) == 1:
            exchange_mode = "library: dfx_aggregate_exchange (grouped ncclSend/ncclRecv on the library's stream)"
            ranks_seen = comm.ranks()
            if ranks_seen != world:  # (RCCL's own count of the library communicator: anything else is not the job that was asked for)
                raise SystemExit(f"bench.py: the library communicator reports {ranks_seen} ranks, the job has {world}")
        else:
            comm = None
            exchange_mode = "host: torch.distributed all_to_all_single around dfx_aggregate_partial_* (library communicator unavailable" + \
                            (": " + comm_error if not ok else " on another rank") + ")"
            if not args.allow_host_exchange:
                if rank == 0:
                    print("bench.py: " + exchange_mode + " -- refusing to report a multi-GPU line without RCCL (--allow-host-exchange overrides)", file=sys.stderr, flush=True)
                dist.destroy_process_group()
                raise SystemExit(3)

    emit_s = [0.0, 0.0]  # [wall seconds of agg.next() after an exchange, seconds in the host-driven exchange]

    def finish(agg):
        """exchange (multi-GPU) + the single result batch"""
        if world > 1 and comm is not None:
            comm.exchange(agg)
        elif world > 1:
            t_x = time.perf_counter()
            exchange_group_partials(agg, world, device, dist, torch)
            emit_s[1] += time.perf_counter() - t_x
        t_e = time.perf_counter()
        out = agg.next()
        emit_s[0] += time.perf_counter() - t_e
        assert agg.next() is None
        return out

    def phases_begin():
        ex.counter_reset()
        emit_s[0] = emit_s[1] = 0.0

    def phases_end(steps):
        """per-rank phase times of the steps since phases_begin(), reduced to min / max over the ranks (ms per step):
        local scan + aggregation | wait for the slowest rank | dfx_aggregate_exchange proper (counts, payload, merge) | emit + download"""
        if world <= 1:
            return None
        mine = [ex.counter_get("xchg_local_us") / 1e3 / steps, ex.counter_get("xchg_wait_peers_us") / 1e3 / steps,
                ex.counter_get("xchg_exchange_us") / 1e3 / steps, emit_s[0] * 1e3 / steps, emit_s[1] * 1e3 / steps]
        t = torch.tensor(mine, dtype=torch.float64, device=coll_device)
        lo, hi = t.clone(), t.clone()
        dist.all_reduce(lo, op=dist.ReduceOp.MIN)
        dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        names = ["local_scan_and_aggregate", "wait_for_slowest_rank", "exchange_and_merge", "emit_and_download", "host_driven_exchange"]
        out = {n_: {"min_over_ranks": round(float(lo[i].item()), 3), "max_over_ranks": round(float(hi[i].item()), 3)} for i, n_ in enumerate(names)
               if i < 4 or float(hi[i].item()) > 0.0}
        # what the library's exchange cost in protocol terms (rank 0's counters; grouped queries): collective rounds and host
        # synchronisations per query -- round 6: 2 and 2 (the all-gather of states + counts, the buckets)
        calls = max(1, ex.counter_get("xchg_calls"))
        out["collective_rounds"] = round(ex.counter_get("xchg_rounds") / calls, 2)
        out["host_syncs"] = round(ex.counter_get("xchg_host_syncs") / calls, 2)
        return out

    def step(filter_expr=pred, group=(Column(0),), aggs=(sum_v,)):
        return finish(build(filter_expr, list(group), list(aggs)))

    def sync():
        ex.synchronize()
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()

    def timed(fn, steps, warmup):
        for _ in range(warmup):
            fn()
        sync()
        t0 = time.perf_counter()
        last = None
        for _ in range(steps):
            last = fn()
        sync()
        dt = time.perf_counter() - t0
        if world > 1:
            t = torch.tensor([dt], dtype=torch.float64, device=coll_device)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        return dt, last

    # ---- the headline measurement ---------------------------------------------------------------
    # Two timed regions of exactly K steps each, same work:
    #   1. un-instrumented -> `value` / `ms_per_step` (what a caller of the library gets);
    #   2. with the library's HIP-event profiler on (two events around every tracked launch, on the launch stream)
    #      -> the per-kernel durations the roofline is computed from.  The events serialise the kernel chain
    #      (~10 us of idle device per launch, rocprofv3 timeline), so region 2 is ~8 % slower; its time is
    #      reported as extra.instrumented_ms_per_step.
    sync()
    t_cold = time.perf_counter()
    step()  # the process's very first query: calibration slice, first use of every pool, idle-box clocks
    sync()
    cold_first_step_ms = (time.perf_counter() - t_cold) * 1e3
    for _ in range(args.prewarm_steps):
        step()
    for _ in range(args.warmup):
        step()
    phases_begin()
    dt, result = timed(step, args.steps, 0)
    phases_headline = phases_end(args.steps)
    if args.dump_outputs:
        dump_outputs(result, args.dump_outputs, "" if world == 1 else f"_rank{rank}")
    plan_text = "n/a"
    if world == 1 and args.full:  # physical plan of the timed query after one more (untimed) run: fusion, kernel family, strategy, groups
        try:
            plan_agg = build(pred, [Column(0)], [sum_v])
            plan_agg.next()
            plan_text = ex.explain(plan_agg)
            del plan_agg
        except Exception as e:  # never lose the measurement over a description
            plan_text = f"unavailable: {e}"
    total_rows = n_rows * world
    value = total_rows * args.steps / dt
    ms_per_step = dt / args.steps * 1e3
    dt_instr, prof = None, {}
    if args.full:
        sync()
        ex.profile_reset()
        ex.profile_enable(True)
        dt_instr, _ = timed(step, args.steps, 0)
        ex.profile_enable(False)
        prof = {p["kernel"]: p for p in ex.profile_snapshot()}

    # the oracle's side of the per-configuration checks below: started now, on host threads of their own, so that they run
    # beside the remaining GPU measurements (the headline regions above are not disturbed) and are joined when needed
    verify_rows = int(min(args.verify_rows, n_rows))
    want_extras = args.full and (not args.no_extras) and world == 1
    want_oracle = want_extras and rank == 0 and not args.no_cpu_baseline
    seed2 = 0xDF01
    syn_lat = [("lat", ex.SYNTH_F64_UNIFORM, 0, 49.0, 10.0)]  # lat = 49 + 10 u, seed 0xDF01
    schema2 = pa.schema([("lat", pa.float64())])
    pred2 = BinaryExpr(BinaryExpr(Column(0), Operator.Gt, l64(51.0)), Operator.And, BinaryExpr(Column(0), Operator.Lt, l64(53.0)))
    # BASELINE config 5's shape (TPC-H Q1: 7 columns = 56 B/row, 2 predicates, 2 keys, 4 SUMs, <= 6 groups)
    syn5 = [("rf", ex.SYNTH_I64_UNIFORM, 0, 3.0, 0.0), ("ls", ex.SYNTH_I64_UNIFORM, 1, 2.0, 0.0),
            ("qty", ex.SYNTH_F64_UNIFORM, 2, 1.0, 49.0), ("price", ex.SYNTH_F64_UNIFORM, 3, 900.0, 104100.0),
            ("disc", ex.SYNTH_F64_UNIFORM, 4, 0.0, 0.10), ("tax", ex.SYNTH_F64_UNIFORM, 5, 0.0, 0.08),
            ("ship", ex.SYNTH_F64_UNIFORM, 6, 0.0, 2526.0)]
    schema5 = pa.schema([(nm, pa.int64() if i < 2 else pa.float64()) for i, (nm, *_r) in enumerate(syn5)])
    dp = BinaryExpr(Column(3), Operator.Multiply, BinaryExpr(l64(1.0), Operator.Minus, Column(4)))
    aggs5 = [AggregateFunction("sum", [Column(2)], f64), AggregateFunction("sum", [Column(3)], f64),
             AggregateFunction("sum", [dp], f64),
             AggregateFunction("sum", [BinaryExpr(dp, Operator.Multiply, BinaryExpr(l64(1.0), Operator.Plus, Column(5)))], f64)]
    pred5 = BinaryExpr(BinaryExpr(Column(6), Operator.LtEq, l64(2436.0)), Operator.And, BinaryExpr(Column(4), Operator.GtEq, l64(0.0)))
    count_qty = AggregateFunction("COUNT", [Column(2)], DataType.UInt64)
    # the neighbours of the headline query measured as extras (defined here: their oracle runs start before any timing)
    pred_n = BinaryExpr(BinaryExpr(Column(1), Operator.GtEq, l64(LO)), Operator.And, BinaryExpr(Column(1), Operator.Lt, l64(HI)))
    min_v = AggregateFunction("MIN", [Column(1)], f64)
    pred_1 = BinaryExpr(Column(1), Operator.Lt, l64(LO))
    sum_2v = AggregateFunction("SUM", [BinaryExpr(Column(1), Operator.Multiply, l64(2.0))], f64)
    pred_3 = BinaryExpr(pred, Operator.And, BinaryExpr(Column(0), Operator.GtEq, Literal(ScalarValue.Int64(0))))
    syn_w = syn + [("w", ex.SYNTH_F64_EXACT, 2, 0.0, 0.0)]
    schema_w = pa.schema([("k", pa.int64()), ("v", pa.float64()), ("w", pa.float64())])
    min_w = AggregateFunction("MIN", [Column(2)], f64)
    max_w = AggregateFunction("MAX", [Column(2)], f64)
    avg_v = AggregateFunction("AVG", [Column(1)], f64)
    syn_z = [("k", ex.SYNTH_I64_ZIPF, 0, float(GROUPS), 1.0), ("v", ex.SYNTH_F64_EXACT, 1, 0.0, 0.0)]
    # name -> (generator columns, schema, predicate, aggregates): every one checked on the first verify_rows rows
    neighbours = {"headline_through_interpreter": (syn, schema, pred, [sum_v]),
                  "neighbour_query_sum_min": (syn, schema, pred_n, [sum_v, min_v]),
                  "one_term_predicate_query": (syn, schema, pred_1, [sum_v]),
                  "product_argument_query": (syn, schema, pred, [sum_2v]),
                  "three_term_predicate_query": (syn, schema, pred_3, [sum_v]),
                  "different_operand_sum_min": (syn_w, schema_w, pred, [sum_v, min_w]),
                  "avg_v_max_w_two_columns": (syn_w, schema_w, pred, [avg_v, max_w]),
                  "zipf_keys": (syn_z, schema, pred, [sum_v])}
    # round 4: the run-time shape FAMILY (scan plans: the query is data, csrc/dfx_device.hpp DevScanPlan) -- what round 3 ran through
    # FastPolicy (0.29) or the interpreter (0.16)
    i64lit = lambda v: Literal(ScalarValue.Int64(v))
    pred_k = BinaryExpr(BinaryExpr(Column(0), Operator.GtEq, i64lit(200000)), Operator.And, BinaryExpr(Column(0), Operator.Lt, i64lit(400000)))
    syn_nv = [syn[0], ("v", ex.synth_nulls(ex.SYNTH_F64_EXACT, 100), 1, 0.0, 0.0)]
    syn_k32 = [("k", ex.SYNTH_I32_UNIFORM, 0, float(GROUPS), 0.0), syn[1]]
    schema_k32 = pa.schema([("k", pa.int32()), ("v", pa.float64())])
    family = {"min_only": (syn, schema, pred, [min_v], 16, "SELECT k, MIN(v) WHERE v > lo AND v < hi GROUP BY k (the headline's scan, another accumulator: pass 1 routes the ordered image)"),
              "int64_predicate": (syn, schema, pred_k, [sum_v], 16, "SELECT k, SUM(v) WHERE k >= 200000 AND k < 400000 GROUP BY k (a two-term range on the Int64 key column, 20 % of the rows)"),
              "nullable_v_10pct": (syn_nv, schema, pred, [sum_v], 16.125, "the headline query over a v column with a validity bitmap, 10 % nulls (16 B + 1 validity bit per row; round 3: a "
                                   "materialised FilterRelation + the interpreter)"),
              "int32_key": (syn_k32, schema_k32, pred, [sum_v], 12, "the headline query with an Int32 key column (12 B/row: the reference's own fixtures group by Int32, aggregate.rs:1033-1127)"),
              "headline_through_scan_plan": (syn, schema, pred, [sum_v], 16, "the headline query with scan.plan = 2: the plan kernels INSTEAD of its compile-time signature (what the signature still buys)")}
    # round 5: what the headline's numbers do NOT say by themselves -- keys that are not small integers, and other selectivities
    syn_wide = [("k", ex.SYNTH_I64_WIDE, 0, float(GROUPS), 0.0), syn[1]]
    pred_s50 = BinaryExpr(BinaryExpr(Column(1), Operator.Gt, l64(LO)), Operator.And, BinaryExpr(Column(1), Operator.Lt, l64(716.8)))
    pred_s80 = BinaryExpr(BinaryExpr(Column(1), Operator.Gt, l64(LO)), Operator.And, BinaryExpr(Column(1), Operator.Lt, l64(1024.0)))
    family["wide_int64_keys"] = (syn_wide, schema, pred, [sum_v], 16, "the headline query over 10^6 distinct keys (u + 1) * 0x9E3779B97F4A7C15 mod 2^64: every key >= 2^32, half of them negative "
                                 "(hashed ids; the reference takes any Int64 key, aggregate.rs:807-852) -- 16-byte routed rows {key, operand}, 64-bit key compares in pass 2")
    family["wide_int64_keys_no_filter"] = (syn_wide, schema, None, [sum_v], 16, "config 3 as written (no filter, every row routed) over the same wide keys")
    family["headline_selectivity_50"] = (syn, schema, pred_s50, [sum_v], 16, "the headline query with WHERE v > 204.8 AND v < 716.8: half of the rows pass (the headline keeps a fifth)")
    family["headline_selectivity_80"] = (syn, schema, pred_s80, [sum_v], 16, "the headline query with WHERE v > 204.8 AND v < 1024.0: 80 % of the rows pass")
    for name_, (cols_, sch_, filt_, aggs_, _b, _w) in family.items():
        neighbours[name_] = (cols_, sch_, filt_, aggs_)
    bg = {}
    tail_rows = int(min(verify_rows, 100000000))
    truth_rows = int(min(verify_rows, 1 << 24))
    tail_row0 = (10000000000 - tail_rows) // 64 * 64
    if want_oracle:
        import oracle  # tests/oracle.py: the CPU restatement -- the reported baseline AND the checker of the GPU results
        # (started in the order their results are wanted: at most Background.slots of them run at a time)
        bg["cfg2"] = Background(oracle.run_synth_filter, syn_lat, seed2, 0, verify_rows, 1024, pred2)
        bg["cfg3"] = Background(oracle.run_synth_query, syn, seed, 0, verify_rows, 1024, None, [Column(0)], [sum_v])
        for name, (cols_, _sch, filt_, aggs_) in neighbours.items():
            bg[name] = Background(oracle.run_synth_query, cols_, seed, 0, verify_rows, 1024, filt_, [Column(0)], list(aggs_))
        bg["cfg5"] = Background(oracle.run_synth_query, syn5, seed, 0, verify_rows, 1024, pred5, [Column(0), Column(1)], aggs5 + [count_qty])
        # (the EXACT sums of its first truth_rows rows -- integer arithmetic, tests/oracle.py: exact_sums_q1 -- are numpy code that holds
        # the interpreter lock: computed where they are used, not on a thread beside the timed legs)
        if args.rows_1e10_steps > 0 and n_rows < 10000000000:
            # the LAST verify_rows rows of the 10^10-row table (row indices beyond 2^32: rows 9.9e9 ...): the same generator, seed and rows
            bg["rows_1e10_tail"] = Background(oracle.run_synth_query, syn, seed, tail_row0, 10000000000 - tail_row0, 1024, pred, [Column(0)], [sum_v])

    # dominant kernel = the scan kernel (the one that reads the table) with the largest total time:
    # "partition" (pass 1 of the partitioned strategy: predicate + key/arg evaluation + routing) or
    # "hash_agg" (fused K7) when the table strategy is used
    roofline = None
    scans = [k for k in ("partition", "hash_agg", "reduce_all") if k in prof and prof[k]["algo_bytes"] > 0]
    if scans:
        dom = max(scans, key=lambda k: prof[k]["total_ms"])
        p = prof[dom]
        avg_ms = p["total_ms"] / p["launches"]
        achieved = p["algo_bytes"] / p["total_ms"] * 1e-6  # GB/s
        pipeline_ms = sum(prof[k]["total_ms"] for k in ("partition", "partition_agg", "hash_agg") if k in prof)
        e2e_gbps = value / world * 16 * 1e-9  # per GPU: the metric's own rate x algorithmic bytes per row
        roofline = {"bound": "hbm", "kernel": {"partition": "k_partition pass 1 (K7: fused predicate + key/arg evaluation + LDS "
                                               "write-combined routing to table blocks)",
                                               "hash_agg": "k_hash_agg (fused predicate + group-by, K7)",
                                               "reduce_all": "k_reduce (K5)"}[dom],
                    "achieved": round(achieved, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                    "frac": round(achieved / HBM_PEAK_GBPS, 4), "traffic": None,
                    "launches": p["launches"], "avg_launch_ms": round(avg_ms, 4),
                    "algo_bytes_per_launch": p["algo_bytes"] / p["launches"],
                    "frac_of_measured_copy_6290": round(achieved / 6290.0, 4),
                    "all_aggregation_kernels_GBps": round(n_rows * args.steps * 16 / pipeline_ms * 1e-6, 1)
                    if pipeline_ms > 0 else None,
                    # the whole step (every kernel, the host side, the result on the host) against the same peak
                    "end_to_end_GBps": round(e2e_gbps, 1), "end_to_end_frac": round(e2e_gbps / HBM_PEAK_GBPS, 4)}

    # HBM traffic of the dominant kernel: rocprofv3 PMC passes over the same query (tools/gpu_round.sh profile ->
    # profiles/r06_partition_counters.json; FETCH_SIZE and WRITE_SIZE collected in SEPARATE passes; FETCH_SIZE doubled as
    # MI355X_MICROARCH.md prescribes for gfx950 -- doubled it equals the table bytes read, the calibration point).  It is a
    # committed measurement of this kernel, not something this run collected; null if the file is absent.
    if roofline is not None:
        for fname in ("r06_partition_counters.json", "r05_partition_counters.json", "r04_partition_counters.json", "r03_partition_counters.json", "r02_partition_counters.json"):
            try:
                with open(os.path.join(ROOT, "profiles", fname)) as f:
                    ctr = json.load(f)
                want = "headline | pass1" if dom == "partition" else None
                key = [k for k in ctr if want and k.startswith(want)]
                if key:
                    c = ctr[key[0]]
                    measured = (2.0 * c["FETCH_SIZE_per_dispatch"] + c["WRITE_SIZE_per_dispatch"]) * 1024.0
                    # per launch of THIS run: the profiled dispatches scanned rows_per_dispatch rows each (2^26 if the file predates the field)
                    per_row = measured / float(c.get("rows_per_dispatch", 1 << 26))
                    roofline["traffic"] = per_row * roofline["algo_bytes_per_launch"] / 16.0
                    roofline["traffic_over_algorithmic"] = round(per_row / 16.0, 3)
                    roofline["traffic_source"] = (f"profiles/{fname} (rocprofv3 --pmc in separate passes over tools/prof_query.py headline, "
                                                  "2*FETCH_SIZE + WRITE_SIZE per dispatch of the pass-1 kernel; committed, not collected by this run): "
                                                  + key[0][:120])
                    break
            except Exception:
                pass

    # ---- correctness of the timed result (not timed) --------------------------------------------
    def sum_of_sums_check(tbl, res, rows_total_here):
        """sum over groups of SUM(v) == the ungrouped fused SUM over the same rows, bit for bit (exact data); every group present"""
        local_sum = float(np.sum(res.column(1).to_numpy())) if res.num_rows else 0.0
        local_groups = res.num_rows
        if world > 1:
            t = torch.tensor([local_sum, float(local_groups)], dtype=torch.float64, device=coll_device)
            dist.all_reduce(t)
            local_sum, local_groups = float(t[0].item()), int(t[1].item())
        tot = build_on(tbl, schema, pred, [], [sum_v, count_v]).next()
        ts, tc = tot.column(0)[0].as_py() or 0.0, tot.column(1)[0].as_py() or 0
        if world > 1:
            t = torch.tensor([ts, float(tc)], dtype=torch.float64, device=coll_device)
            dist.all_reduce(t)
            ts, tc = float(t[0].item()), int(t[1].item())
        return bool(local_sum == ts and local_groups == GROUPS and abs(tc / rows_total_here - 0.2) < 1e-3)

    if args.full:
        verified = sum_of_sums_check(table, result, total_rows)
        extra = {"plan": plan_text.strip().split("\n"),
                 "kernels": {k: {"launches": v["launches"], "total_ms": round(v["total_ms"], 3)} for k, v in prof.items()},
                 "verified_sum_of_group_sums_equals_ungrouped_sum": verified, "device": info["name"],
                 "groups": GROUPS, "selectivity": 0.2, "instrumented_ms_per_step": dt_instr / args.steps * 1e3}
    else:
        extra = {"device": info["name"], "groups": GROUPS, "selectivity": 0.2}

    def csv_leg(megabytes=1024, batch_rows=1 << 22):
        import tempfile
        rng_c = np.random.default_rng(1)
        nb = 20000
        cols_c = (rng_c.integers(0, 10**6, nb), rng_c.random(nb) * 100, rng_c.standard_normal(nb), rng_c.integers(-10**9, 10**9, nb))
        block = "\n".join(f"{int(a)},{float(b)!r},{float(c)!r},{int(d)}" for a, b, c, d in zip(*cols_c)) + "\n"
        reps = max(1, megabytes * 1000000 // len(block))
        schema_c = pa.schema([("k", pa.int64()), ("lat", pa.float64()), ("lng", pa.float64()), ("w", pa.int64())])
        aggs_c = [AggregateFunction("SUM", [Column(1)], DataType.Float64), AggregateFunction("COUNT", [Column(0)], DataType.UInt64),
                  AggregateFunction("SUM", [Column(3)], DataType.Int64)]
        with tempfile.NamedTemporaryFile("w", suffix=".csv", dir="/tmp", delete=False) as fh:
            path = fh.name
            fh.write("k,lat,lng,w\n")
            for _ in range(reps):
                fh.write(block)
        try:
            size, records = os.path.getsize(path), reps * nb
            # the checker: the oracle's own CSV reader (oracle/dfx_oracle.c: orc_csv_*, datasource.rs:33-58 restated) over the WHOLE
            # file, on a host thread beside the timed GPU passes
            bg_csv = Background(__import__("oracle").read_csv, path, schema_c, 1 << 20) if want_oracle else None
            best = None
            for _ in range(3):
                ex.profile_reset()
                ex.profile_enable(True)
                t0 = time.perf_counter()
                src = ex.CsvDataSource(path, schema_c, batch_rows)
                t1 = time.perf_counter()
                out = ex.AggregateRelation(None, src, [], [ex.compile_expr(None, a, schema_c) for a in aggs_c]).next()
                ex.synchronize()
                t2 = time.perf_counter()
                ex.profile_enable(False)
                k_ms = {p_["kernel"]: p_ for p_ in ex.profile_snapshot()}.get("csv", {"total_ms": 0.0})["total_ms"]
                if best is None or k_ms < best[0]:
                    best = (k_ms, (t1 - t0) * 1e3, (t2 - t1) * 1e3)
            first = ex.CsvDataSource(path, schema_c, nb).next()
            exact = (np.array_equal(first.column(0).to_numpy(), cols_c[0].astype(np.int64)) and
                     np.array_equal(first.column(1).to_numpy().view(np.uint64), np.array([float(repr(float(b))) for b in cols_c[1]]).view(np.uint64)) and
                     np.array_equal(first.column(2).to_numpy().view(np.uint64), np.array([float(repr(float(c))) for c in cols_c[2]]).view(np.uint64)) and
                     np.array_equal(first.column(3).to_numpy(), cols_c[3].astype(np.int64)))
            ok = bool(exact) and out.column(1)[0].as_py() == records and out.column(2)[0].as_py() == int(np.sum(cols_c[3])) * reps
            every = None
            if bg_csv is not None:
                # EVERY record of the file: the product's batches against the oracle reader's, column by column, bit for bit; the
                # Float64 SUM against the reference-shaped sum of the oracle's batches by check_float_sums (and against the exact sum)
                import math
                import oracle as orc
                ref_batches = bg_csv.get()
                ref_cols = [np.concatenate([b.column(i).to_numpy(zero_copy_only=False) for b in ref_batches]) for i in range(4)]
                src_all = ex.CsvDataSource(path, schema_c, batch_rows)
                got_parts = [[] for _ in range(4)]
                while True:
                    b_ = src_all.next()
                    if b_ is None:
                        break
                    for i in range(4):
                        got_parts[i].append(b_.column(i).to_numpy(zero_copy_only=False))
                got_cols = [np.concatenate(x) for x in got_parts]
                same = all(len(g_) == len(r_) == records and np.array_equal(g_.view(np.uint64), r_.view(np.uint64)) for g_, r_ in zip(got_cols, ref_cols))
                ref_out = orc.aggregate([], aggs_c, ref_batches)
                sums = orc.check_float_sums(np.array([out.column(0)[0].as_py()]), np.array([ref_out.column(0)[0].as_py()]), np.array([records]),
                                            np.array([float(np.sum(np.abs(ref_cols[1])))]), truth=np.array([math.fsum(ref_cols[1])]), what="csv SUM(lat)")
                every = {"records_compared": int(len(ref_cols[0])), "columns_bit_exact": bool(same), "float_sum": sums}
                ok = ok and bool(same) and ref_out.column(1)[0].as_py() == records
                del ref_batches, ref_cols, got_cols, got_parts
            else:
                want_sum = float(np.sum(cols_c[1])) * reps
                ok = ok and abs(out.column(0)[0].as_py() - want_sum) <= 1e-9 * abs(want_sum)
            algo = size + 32.0 * records  # the text once in, four 8-byte columns out
            gbps = algo / (best[0] * 1e-3) * 1e-9
            return {"what": "CsvDataSource over 1 GB of numeric text (4 columns; tools/csv_bench.py's file): record boundaries, cell conversion "
                            "(Rust str::parse semantics, bit-exact doubles), SUM / COUNT over the columns; all device kernels of the source",
                    "file_bytes": size, "records": records, "csv_kernels_ms": round(best[0], 3), "text_GBps": round(size / (best[0] * 1e-3) * 1e-9, 1),
                    "open_read_and_h2d_ms": round(best[1], 1), "index_parse_aggregate_ms": round(best[2], 2),
                    "csv_tiles": ex.counter_get("csv_tiles"), "csv_general_tiles": ex.counter_get("csv_general_tiles"),
                    "algorithmic_bytes": "text once + 32 bytes of columns per record",
                    "roofline": {"bound": "hbm", "achieved": round(gbps, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s", "frac": round(gbps / HBM_PEAK_GBPS, 4)},
                    "verified_vs_oracle": {"ok": bool(ok), "every_record": every,
                                           "what": "EVERY record of the file: the four columns bit for bit against the oracle's CSV reader (orc_csv_*); COUNT and the "
                                                   "Int64 SUM exact; the Float64 SUM against the oracle's reference-shaped sum by check_float_sums (8 sqrt(n) ULP, "
                                                   "and (sqrt(n) + 8) ULP of the exact sum); the first 20 000 records also against Python's float() / int()"}}
        finally:
            os.remove(path)

    def rate(rows, secs, bytes_per_row, what):
        """One extra measurement with its own roofline: algorithmic bytes per row x rows/s against the 8 TB/s HBM peak."""
        gbps = rows * bytes_per_row / secs * 1e-9
        return {"rows_per_s": rows / secs, "ms": secs * 1e3, "algorithmic_bytes_per_row": bytes_per_row, "what": what,
                "roofline": {"bound": "hbm", "achieved": round(gbps, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                             "frac": round(gbps / HBM_PEAK_GBPS, 4)}}

    def by_key(b, n_keys=1):
        """columns sorted by the (combined) key"""
        k = b.column(0).to_numpy()
        for i in range(1, n_keys):
            k = k * 1000003 + b.column(i).to_numpy()
        o = np.argsort(k, kind="stable")
        return [k[o]] + [b.column(i).to_numpy()[o] for i in range(n_keys, b.num_columns)]

    def checked(name, fn):
        """a verification must show up in the line, never kill the measurement"""
        if not want_oracle:
            return None
        try:
            return fn()
        except Exception as e:
            return {"rows": verify_rows, "ok": False, "error": f"{name}: {str(e)[:300]}"}

    def verify_neighbour(name, options=()):
        """the extra `name` over the first verify_rows rows of its table, every group and every aggregate against the CPU
        oracle bit for bit (exact data: SUMs, MINs and doubled terms have one representable answer)"""
        def run():
            cols_, sch_, filt_, aggs_ = neighbours[name]
            t_s = ex.DeviceTable.synth(cols_, seed, 0, verify_rows)
            for k_, v_ in options:
                ex.set_option(k_, v_)
            try:
                got = build_on(t_s, sch_, filt_, [Column(0)], list(aggs_)).next()
            finally:
                for k_, _v in options:
                    ex.set_option(k_, 1)
            _secs, kept, want = bg[name].get()
            g, w = by_key(got), by_key(want)
            ok = len(g) == len(w) and len(g[0]) == len(w[0]) and np.array_equal(g[0], w[0])
            for a_, b_ in zip(g[1:], w[1:]):
                ok = ok and np.array_equal(np.ascontiguousarray(a_).view(np.uint64), np.ascontiguousarray(b_).view(np.uint64))
            return {"rows": verify_rows, "groups": int(len(w[0])), "rows_passing": int(kept), "ok": bool(ok),
                    "what": "every group, every aggregate bit-exact, GPU (same options, same batch width) vs CPU oracle over the same rows"}
        return checked(name, run)

    extra["prewarm_steps"] = args.prewarm_steps
    extra["cold_first_step_ms"] = cold_first_step_ms
    if roofline is not None:
        # `frac` is the DOMINANT KERNEL's (SURVEY.md section 8(d) asks for that); the query's own number is end_to_end_frac, and the first
        # query of a shape on a table pays the calibration slice on top (cold_first_step_ms, this process's very first step)
        roofline["frac_is"] = "the dominant kernel alone (pass 1); the whole step: end_to_end_frac"
        roofline["cold_first_step_ms"] = round(cold_first_step_ms, 3)
        roofline["ms_per_step"] = round(ms_per_step, 4)
    if phases_headline is not None:
        extra["phases_ms"] = phases_headline
    if want_extras:
        k3 = max(2, args.steps // 2)
        # BASELINE config 3 as written: SELECT k, SUM(v) GROUP BY k -- no filter, every row is routed
        d3, _ = timed(lambda: step(None), k3, 1)
        extra["cfg3_groupby_sum_no_filter"] = rate(n_rows * k3, d3, 16, "SELECT k, SUM(v) GROUP BY k (10^6 keys), no filter")
        extra["cfg3_groupby_sum_no_filter_rows_per_s"] = n_rows * k3 / d3

        def verify_cfg3():
            t_s = table if verify_rows == n_rows else ex.DeviceTable.synth(syn, seed, 0, verify_rows)
            got = build_on(t_s, schema, None, [Column(0)], [sum_v]).next()
            _secs, kept, want = bg["cfg3"].get()
            gk, gs = by_key(got)
            wk, ws = by_key(want)
            ok = bool(kept == verify_rows and len(gk) == len(wk) and np.array_equal(gk, wk) and np.array_equal(gs.view(np.uint64), ws.view(np.uint64)))
            return {"rows": verify_rows, "groups": int(len(wk)), "ok": ok,
                    "what": f"SUM bit-exact for every group, GPU ({args.batch_rows}-row batches, automatic strategy) vs CPU oracle over the same rows"}

        # BASELINE config 2, fused form: predicate + COUNT (K5, one pass over the column); BASELINE.md's column: lat = 49 + 10 u
        t2 = ex.DeviceTable.synth(syn_lat, seed2, 0, n_rows)
        count_lat = AggregateFunction("COUNT", [Column(0)], DataType.UInt64)

        def mask_only():
            return build_on(t2, schema2, pred2, [], [count_lat]).next()
        d2, r2 = timed(mask_only, k3, 1)
        extra["cfg2_predicate_count"] = rate(n_rows * k3, d2, 8, "SELECT COUNT(lat) WHERE lat > 51 AND lat < 53 (fused predicate + reduce)")
        extra["cfg2_predicate_count_rows_per_s"] = n_rows * k3 / d2

        # BASELINE config 2 as written: the FilterRelation itself over the one Float64 column -- single pass: predicate, LSB
        # bitmap, decoupled look-back over the tiles' kept counts and the compaction in ONE kernel (filter.single_pass),
        # compacted batches left on the device (dfx_relation_drain_device: no D2H)
        kept2 = [0]

        def filter_as_written():
            rel = ex.FilterRelation(t2.scan(args.batch_rows), ex.compile_scalar_expr(None, pred2, schema2), schema2)
            kept2[0] = ex.drain_on_device(rel)[0]
        dfw, _ = timed(filter_as_written, k3, 1)
        sel2 = kept2[0] / n_rows
        extra["cfg2_filter_mask_and_compact"] = rate(n_rows * k3, dfw, 8.125 + 8 * sel2,
                                                     f"FilterRelation as written over lat = 49 + 10 u: bitmap + compacted output on the device, selectivity {sel2:.3f} "
                                                     "(8.125 + 8 sel B/row: the column is read once)")
        extra["cfg2_filter_kept_equals_count"] = bool(kept2[0] == (r2.column(0)[0].as_py() or 0))
        ex.set_option("filter.single_pass", 0)
        try:
            dfw2, _ = timed(filter_as_written, k3, 1)
        finally:
            ex.set_option("filter.single_pass", 1)
        extra["cfg2_filter_two_pass"] = rate(n_rows * k3, dfw2, 8.125 + 8 * sel2, "the same with filter.single_pass = 0 (k_predicate_mask -> scan -> k_compact: "
                                             "round 2's path, the column is read twice)")

        # ... and when the filter is NOT selective: a wave parks at most a quarter of its 4096-row tile in LDS, denser tiles re-read
        # their passing rows after the look-back (two reads of those tiles) -- what that costs, at selectivity 0.5 and 0.9
        dense_preds = {"cfg2_filter_dense_sel50": (51.0, 56.0), "cfg2_filter_dense_sel90": (49.5, 58.5)}
        for name_, (lo_, hi_) in dense_preds.items():
            pd_ = BinaryExpr(BinaryExpr(Column(0), Operator.Gt, l64(lo_)), Operator.And, BinaryExpr(Column(0), Operator.Lt, l64(hi_)))
            keptd = [0]

            def filter_dense():
                rel = ex.FilterRelation(t2.scan(args.batch_rows), ex.compile_scalar_expr(None, pd_, schema2), schema2)
                keptd[0] = ex.drain_on_device(rel)[0]
            try:
                dfd, _ = timed(filter_dense, k3, 1)
                seld = keptd[0] / n_rows
                extra[name_] = rate(n_rows * k3, dfd, 8.125 + 8 * seld, f"FilterRelation over lat = 49 + 10 u WHERE lat > {lo_} AND lat < {hi_}: selectivity {seld:.3f} "
                                    "(8.125 + 8 sel B/row), bitmap + compacted output on the device")
                if want_oracle:
                    bg[name_] = Background(oracle.run_synth_filter, syn_lat, seed2, 0, min(verify_rows, 30000000), 1024, pd_)
            except Exception as e:
                extra[name_] = {"error": str(e)[:200]}

        def verify_dense(name_):
            lo_, hi_ = dense_preds[name_]
            pd_ = BinaryExpr(BinaryExpr(Column(0), Operator.Gt, l64(lo_)), Operator.And, BinaryExpr(Column(0), Operator.Lt, l64(hi_)))
            rows_ = min(verify_rows, 30000000)
            t_s = ex.DeviceTable.synth(syn_lat, seed2, 0, rows_)
            rel = ex.FilterRelation(t_s.scan(args.batch_rows), ex.compile_scalar_expr(None, pd_, schema2), schema2)
            _secs, kept, want_cols, _m = bg[name_].get()
            parts = []
            while True:
                b = rel.next()
                if b is None:
                    break
                parts.append(b.column(0).to_numpy())
            got = np.concatenate(parts) if parts else np.empty(0)
            ok = bool(len(got) == kept and np.array_equal(got.view(np.uint64), want_cols[0][:kept].view(np.uint64)))
            return {"rows": rows_, "rows_passing": int(kept), "ok": ok, "what": "the compacted column, GPU vs CPU oracle (orc_filter_next, 1024-row batches), bit for bit"}

        def verify_cfg2():
            t_s = t2 if verify_rows == n_rows else ex.DeviceTable.synth(syn_lat, seed2, 0, verify_rows)
            rel = ex.FilterRelation(t_s.scan(args.batch_rows), ex.compile_scalar_expr(None, pred2, schema2), schema2)
            rel.keep_mask()
            _secs, kept, want_cols, want_mask = bg["cfg2"].get()
            want = want_cols[0]
            at, row0, ok = 0, 0, True
            while True:
                b = rel.next()
                if b is None:
                    break
                bits, rows = rel.last_mask(args.batch_rows)
                got = b.column(0).to_numpy()
                ok = ok and np.array_equal(bits, want_mask[row0 // 8:(row0 + rows + 7) // 8]) and \
                    np.array_equal(got.view(np.uint64), want[at:at + len(got)].view(np.uint64))
                at += len(got)
                row0 += rows
            ok = bool(ok and row0 == verify_rows and at == kept)
            return {"rows": verify_rows, "rows_passing": int(kept), "ok": ok,
                    "what": "the Arrow bitmap of every batch and the compacted column, GPU vs CPU oracle (orc_filter_next, 1024-row batches), bit for bit"}
        extra["cfg2_filter_mask_and_compact"]["verified_vs_oracle"] = checked("cfg2", verify_cfg2)
        for name_ in dense_preds:
            if "roofline" in extra.get(name_, {}):
                extra[name_]["verified_vs_oracle"] = checked(name_, lambda n_=name_: verify_dense(n_))

        def verify_cfg2_count():
            t_s = t2 if verify_rows == n_rows else ex.DeviceTable.synth(syn_lat, seed2, 0, verify_rows)
            got = build_on(t_s, schema2, pred2, [], [count_lat]).next().column(0)[0].as_py() or 0
            _secs, kept, _c, _m = bg["cfg2"].get()
            return {"rows": verify_rows, "rows_passing": int(kept), "ok": bool(int(got) == int(kept)),
                    "what": "COUNT of the fused predicate + reduce, GPU vs the rows the CPU oracle's FilterRelation kept over the same slice"}
        extra["cfg2_predicate_count"]["verified_vs_oracle"] = checked("cfg2_count", verify_cfg2_count)
        del t2
        extra["cfg3_groupby_sum_no_filter"]["verified_vs_oracle"] = checked("cfg3", verify_cfg3)

        # generic paths of the headline query: the SSA interpreter (scan.fast = 0) and a neighbour query no compile-time
        # signature covers (>= / <, SUM + MIN: run-time decoded shape, generic row width)
        ex.set_option("scan.fast", 0)
        try:
            dgi, _ = timed(step, k3, 1)
        finally:
            ex.set_option("scan.fast", 1)
        extra["headline_through_interpreter"] = rate(n_rows * k3, dgi, 16, "the headline query with scan.fast = 0 (generic SSA interpreter in every kernel)")
        extra["headline_through_interpreter"]["verified_vs_oracle"] = verify_neighbour("headline_through_interpreter", (("scan.fast", 0),))
        dgn, _ = timed(lambda: step(pred_n, (Column(0),), (sum_v, min_v)), k3, 1)
        extra["neighbour_query_sum_min"] = rate(n_rows * k3, dgn, 16, "SELECT k, SUM(v), MIN(v) WHERE v >= lo AND v < hi GROUP BY k "
                                                "(two aggregates of one operand: 12-byte routed rows {image, raw operand})")
        extra["neighbour_query_sum_min"]["verified_vs_oracle"] = verify_neighbour("neighbour_query_sum_min")
        # shapes without a compile-time signature (FastPolicy: run-time decoded column-op-literal terms)
        dg1, _ = timed(lambda: step(pred_1, (Column(0),), (sum_v,)), k3, 1)
        extra["one_term_predicate_query"] = rate(n_rows * k3, dg1, 16, "SELECT k, SUM(v) WHERE v < lo GROUP BY k (one ordered Float64 comparison runs as the "
                                                 "two-sided range v >= -inf AND v < lo: the headline's compile-time signature; FastPolicy until round 3)")
        extra["one_term_predicate_query"]["verified_vs_oracle"] = verify_neighbour("one_term_predicate_query")
        dg2, _ = timed(lambda: step(pred, (Column(0),), (sum_2v,)), k3, 1)
        extra["product_argument_query"] = rate(n_rows * k3, dg2, 16, "SELECT k, SUM(v * 2.0) WHERE v > lo AND v < hi GROUP BY k (signature KeyAffSumPred2F64 in pass 1: "
                                               "argument = column <op> literal, the op read at run time; FastPolicy until round 3)")

        extra["product_argument_query"]["verified_vs_oracle"] = verify_neighbour("product_argument_query")
        # a shape NO compile-time signature covers (three terms, one of them on the Int64 key): FastPolicy, decoded at run time
        dg3, _ = timed(lambda: step(pred_3, (Column(0),), (sum_v,)), k3, 1)
        extra["three_term_predicate_query"] = rate(n_rows * k3, dg3, 16, "SELECT k, SUM(v) WHERE v > lo AND v < hi AND k >= 0 GROUP BY k (no compile-time signature: a scan plan; FastPolicy until round 4)")
        extra["three_term_predicate_query"]["verified_vs_oracle"] = verify_neighbour("three_term_predicate_query")

        # the shape family (scan plans): one more accumulator kind, an Int64 predicate column, a validity bitmap, a 4-byte key,
        # and the headline itself through the plan kernels
        for name_, (cols_, sch_, filt_, aggs_, bytes_, what_) in family.items():
            opts_ = (("scan.plan", 2),) if name_ == "headline_through_scan_plan" else ()
            try:
                tf = table if cols_ is syn else ex.DeviceTable.synth(cols_, seed, 0, n_rows)
                for k_, v_ in opts_:
                    ex.set_option(k_, v_)
                try:
                    dfm, _ = timed(lambda: build_on(tf, sch_, filt_, [Column(0)], list(aggs_)).next(), k3, 1)
                finally:
                    for k_, _v in opts_:
                        ex.set_option(k_, 1)
                del tf
                extra[name_] = rate(n_rows * k3, dfm, bytes_, what_)
                extra[name_]["verified_vs_oracle"] = verify_neighbour(name_, opts_)
            except Exception as e:  # a measurement, not a gate
                extra[name_] = {"error": str(e)[:200]}

        # two aggregates of DIFFERENT operands over 10^6 groups (generic 24-byte routed rows: no shared operand, no narrow form)
        try:
            tw = ex.DeviceTable.synth(syn_w, seed, 0, n_rows)
            dgw, _ = timed(lambda: build_on(tw, schema_w, pred, [Column(0)], [sum_v, min_w]).next(), k3, 1)
            extra["different_operand_sum_min"] = rate(n_rows * k3, dgw, 24, "SELECT k, SUM(v), MIN(w) WHERE v > lo AND v < hi GROUP BY k (two aggregates of "
                                                      "different operands over 10^6 groups: the pair scan -- one pass 1 routes 20-byte rows {v, hash image, w}, a pass 2 per "
                                                      "accumulator plane, agg.pair_scan; rounds 4-6: one scan per aggregate, 0.29-0.30); 24 B/row of algorithmic bytes")
            extra["different_operand_sum_min"]["verified_vs_oracle"] = verify_neighbour("different_operand_sum_min")
            # three accumulators over the two columns: the operands travel raw in the pair row, every accumulator has its own pass 2
            dga, _ = timed(lambda: build_on(tw, schema_w, pred, [Column(0)], [avg_v, max_w]).next(), k3, 1)
            extra["avg_v_max_w_two_columns"] = rate(n_rows * k3, dga, 24, "SELECT k, AVG(v), MAX(w) WHERE v > lo AND v < hi GROUP BY k (AVG = SUM + COUNT: three accumulators over two "
                                                    "columns, one scan; a scan per aggregate: 14.3 ms per 10^9 rows = 0.21); 24 B/row of algorithmic bytes")
            extra["avg_v_max_w_two_columns"]["verified_vs_oracle"] = verify_neighbour("avg_v_max_w_two_columns")
            del tw
        except Exception as e:  # a measurement, not a gate
            extra.setdefault("different_operand_sum_min", {"error": str(e)[:200]})
            extra.setdefault("avg_v_max_w_two_columns", {"error": str(e)[:200]})

        # skewed keys (Zipf s = 1.0; the generator is log-uniform, p(k) ~ 1/k), same query
        tz = ex.DeviceTable.synth(syn_z, seed, 0, n_rows)
        dz, _ = timed(lambda: build_on(tz, schema, pred, [Column(0)], [sum_v]).next(), k3, 1)
        extra["zipf_keys"] = rate(n_rows * k3, dz, 16, "the headline query over Zipf(1.0)-distributed keys (10^6 keys)")
        extra["zipf_rows_per_s"] = n_rows * k3 / dz
        del tz
        extra["zipf_keys"]["verified_vs_oracle"] = verify_neighbour("zipf_keys")

        # PCIe-inclusive rate: the same query over HOST Arrow batches (HostStreamRelation uploads every batch); never `value`
        try:
            hb_rows = 1 << 24
            rng = np.random.default_rng(7)
            hb = [pa.RecordBatch.from_arrays([pa.array(rng.integers(0, GROUPS, hb_rows).astype(np.int64)),
                                              pa.array(rng.integers(0, 1 << 20, hb_rows).astype(np.float64) / 1024.0)], names=["k", "v"])
                  for _ in range(4)]

            def host_step():
                rel = ex.FilterRelation(ex.DataSourceRelation(schema, hb), ex.compile_scalar_expr(None, pred, schema), schema)
                return ex.AggregateRelation(None, rel, [ex.compile_scalar_expr(None, Column(0), schema)], [ex.compile_expr(None, sum_v, schema)]).next()
            # This leg copies on the HOST (library threads fill the pinned staging ring): nothing else may be running on the host
            # cores -- every oracle run started above is waited for first (their results are kept for the checks that want them).
            for b_ in bg.values():
                b_.t.join()
            dh, _ = timed(host_step, 4, 1)
            e = rate(4 * hb_rows * 4, dh, 16, "the headline query over host Arrow batches (4 x 2^24 rows), H2D inside the timed region: pageable copies in order "
                     "on the library's stream (host.stream = 0, the default: the fastest of the four forms measured, profiles/r04_host_stream_matrix.txt)")
            e["roofline"] = {"bound": "pcie", "achieved": e["roofline"]["achieved"], "peak": 63.0, "unit": "GB/s",
                             "frac": round(e["roofline"]["achieved"] / 63.0, 4)}
            extra["host_streamed_pcie_inclusive"] = e
            ex.set_option("host.stream", 1)  # round 4's pinned staging ring (8 library threads, 6 x 16 MB slots)
            try:
                dh1, _ = timed(host_step, 2, 1)
            finally:
                ex.set_option("host.stream", 0)
            e1 = rate(4 * hb_rows * 2, dh1, 16, "the same with host.stream = 1: a ring of pinned slots filled by 8 library threads, DMA on a copy stream (slower: the staging "
                      "copy triples the host-memory traffic per byte moved)")
            e1["roofline"] = {"bound": "pcie", "achieved": e1["roofline"]["achieved"], "peak": 63.0, "unit": "GB/s", "frac": round(e1["roofline"]["achieved"] / 63.0, 4)}
            extra["host_streamed_staged_ring"] = e1

            def verify_host():
                got = host_step()
                want = oracle.aggregate([Column(0)], [sum_v], [oracle.filter_next(pred, b) for b in hb])
                g, w = by_key(got), by_key(want)
                ok = len(g[0]) == len(w[0]) and np.array_equal(g[0], w[0]) and np.array_equal(g[1].view(np.uint64), w[1].view(np.uint64))
                return {"rows": 4 * hb_rows, "groups": int(len(w[0])), "ok": bool(ok),
                        "what": "SUM bit-exact for every group, GPU over the host batches vs the CPU oracle's FilterRelation + AggregateRelation over the same batches"}
            extra["host_streamed_pcie_inclusive"]["verified_vs_oracle"] = checked("host_streamed", verify_host)
            del hb
        except Exception as e:  # a measurement, not a gate
            extra["host_streamed_pcie_inclusive"] = {"error": str(e)[:200]}

    # ---- config 4 AS WRITTEN on N GPUs: config 3's query -- no filter, every row routed -- over the ranks' row ranges -----
    # (the headline above keeps its 20 %-selective predicate at every N, so that the N = 1, 2, 4, 8 values are one curve; the
    # unfiltered query is 2.3 x slower per row on one GPU, and BASELINE.json's config 4 names it)
    if world > 1 and args.full and not args.no_extras:
        k4 = max(2, args.steps // 2)
        step(None)
        phases_begin()
        d4, r4 = timed(lambda: step(None), k4, 0)
        e4 = rate(total_rows * k4, d4, 16, f"BASELINE config 4 as written: SELECT k, SUM(v) GROUP BY k (no filter) over {total_rows} rows on {world} GPUs, "
                  "group partials exchanged inside the library")
        e4["roofline"]["achieved"] = round(e4["roofline"]["achieved"] / world, 1)  # per GPU against the per-GPU peak
        e4["roofline"]["frac"] = round(e4["roofline"]["achieved"] / HBM_PEAK_GBPS, 4)
        e4["roofline"]["per"] = "GPU"
        e4["phases_ms"] = phases_end(k4)
        g4 = torch.tensor([float(r4.num_rows)], dtype=torch.float64, device=coll_device)
        dist.all_reduce(g4)
        e4["groups_over_all_ranks"] = int(g4.item())
        e4["every_group_emitted_once"] = bool(int(g4.item()) == GROUPS)
        extra["cfg4_as_written"] = e4

    # ---- config 5 (TPC-H Q1 shape): one GPU as an extra, N GPUs over the ranks' row ranges -----------------
    if (want_extras or world > 1) and args.full and not args.no_extras:
        k3 = max(2, args.steps // 2)
        n5 = n_rows if world == 1 else int(min(n_rows, 2500000000))  # 56 B/row: at most 140 GB per rank
        if world > 1:
            del table  # 16 B/row of HBM back before 56 B/row arrive
            table = None
        t5 = ex.DeviceTable.synth(syn5, seed, rank * n5, n5)

        def q1():
            return finish(build_on(t5, schema5, pred5, [Column(0), Column(1)], aggs5))
        q1()
        phases_begin()
        d5, r5 = timed(q1, k3, 0)
        phases5 = phases_end(k3)
        extra["cfg5_q1_shape"] = rate(n5 * world * k3, d5, 56, "TPC-H Q1 shape: 7 columns, 2 predicates, 2 keys, 4 SUMs of expressions, 6 groups" +
                                      (f"; {n5} rows per rank x {world} ranks, group partials exchanged" if world > 1 else ""))
        if world > 1:  # per GPU against the per-GPU peak
            g = extra["cfg5_q1_shape"]["roofline"]
            g["achieved"] = round(g["achieved"] / world, 1)
            g["frac"] = round(g["achieved"] / HBM_PEAK_GBPS, 4)
            g["per"] = "GPU"
            extra["cfg5_q1_shape"]["phases_ms"] = phases5
        extra["cfg5_q1_shape_rows_per_s"] = n5 * world * k3 / d5
        extra["cfg5_q1_shape_GBps_at_56B_per_row"] = n5 * world * k3 * 56 / d5 * 1e-9
        g5 = r5.num_rows
        if world > 1:
            t = torch.tensor([float(g5)], dtype=torch.float64, device=coll_device)
            dist.all_reduce(t)
            g5 = int(t.item())
        extra["cfg5_groups"] = g5

        def verify_cfg5():
            t_s = t5 if verify_rows == n5 else ex.DeviceTable.synth(syn5, seed, 0, verify_rows)
            got = build_on(t_s, schema5, pred5, [Column(0), Column(1)], aggs5).next()
            _secs, kept, want = bg["cfg5"].get()
            g, w = by_key(got, 2), by_key(want, 2)
            ok = len(g[0]) == len(w[0]) and np.array_equal(g[0], w[0]) and int(w[5].sum()) == kept
            worst, worst_sqrt = 0.0, 0.0
            for i in range(1, 5):  # uniform doubles: a parallel sum cannot reproduce the sequential rounding; every term is positive
                try:  # n * eps * sum|v| (proven) AND 8 sqrt(n) ULP of the reference's sum (working bound): tests/oracle.py, BASELINE.md section 3
                    st_ = oracle.check_float_sums(g[i], w[i], w[5], w[i], what=f"cfg5 SUM #{i}")
                    worst, worst_sqrt = max(worst, st_["max_ulp_vs_reference"]), max(worst_sqrt, st_["max_over_sqrt_n"])
                except AssertionError as e:
                    return {"rows": verify_rows, "ok": False, "error": str(e)[:300]}
            # the truth column: the same query over the first truth_rows rows against the EXACT sums of those rows
            worst_exact, ref_exact = 0.0, 0.0
            try:
                truth, tcount = oracle.exact_sums_q1(syn5, seed, 0, truth_rows)
                t_t = ex.DeviceTable.synth(syn5, seed, 0, truth_rows)
                got_t = build_on(t_t, schema5, pred5, [Column(0), Column(1)], aggs5).next()
                gt = by_key(got_t, 2)
                gid = (got_t.column(0).to_numpy() * 2 + got_t.column(1).to_numpy())[np.argsort(got_t.column(0).to_numpy() * 1000003 + got_t.column(1).to_numpy(), kind="stable")]
                n_t = tcount[gid].astype(np.float64)
                for i in range(1, 5):
                    tv = truth[i - 1][gid]
                    st_ = oracle.check_float_sums(gt[i], tv, n_t, tv, truth=tv, what=f"cfg5 SUM #{i} vs the exact sums of the first {truth_rows} rows")
                    worst_exact = max(worst_exact, st_["max_ulp_vs_exact"])
            except AssertionError as e:
                return {"rows": verify_rows, "ok": False, "error": str(e)[:300]}
            return {"rows": verify_rows, "groups": int(len(w[0])), "rows_passing": int(kept), "ok": bool(ok), "max_ulp_of_reference_sum": worst,
                    "max_ulp_over_sqrt_rows_of_the_group": worst_sqrt, "truth_rows": truth_rows, "max_ulp_of_exact_sum": worst_exact,
                    "what": "keys exact; the four SUMs per group within n * eps * sum|v| AND within 8 sqrt(n) ULP of the CPU oracle's sequential sums "
                            "(n = rows of the group, eps = 2^-52); and, over the first truth_rows rows, within (sqrt(n) + 8) ULP of the EXACT sums "
                            "(integer arithmetic, tests/oracle.py: exact_sums_q1)"}
        if world == 1:
            extra["cfg5_q1_shape"]["verified_vs_oracle"] = checked("cfg5", verify_cfg5)
        del t5

        # ---- CSV text -> Arrow columns on the device (CsvDataSource, datasource.rs:33-58): 1 GB of numeric
        # text -- the file of tools/csv_bench.py -- indexed, converted and summed; the first records bit-exact against Python's
        # float() / int() (correctly rounded, like Rust's parse)
        if world == 1:
            try:
                extra["csv_ingest_1gb"] = csv_leg()
            except Exception as e:  # noqa: BLE001
                extra["csv_ingest_1gb"] = {"error": str(e)[:300]}

    # ---- the north-star size: 1e10 rows (160 GB) on ONE GPU, same query, same code path ------------------------------
    if want_extras and args.rows_1e10_steps > 0 and n_rows < 10000000000:
        try:
            del table
            table = None
            ex.set_option("pool.trim", 1)
            big_rows = 10000000000
            tb = ex.DeviceTable.synth(syn, seed, 0, big_rows)

            def big_step():
                return build_on(tb, schema, pred, [Column(0)], [sum_v]).next()
            # TWO warm-up steps: the first query over a new table runs the calibration slice; the SECOND is the first to take the
            # remembered strategy from its first row on and allocates the full-size routing scratch, GROUP BY table and result
            # buffers (hipMalloc of ~3 GB: +120 ms once per process, tools/stall_probe.py / profiles/r06_stall_probe.txt -- with one
            # warm-up step that allocation fell into the three timed steps on two boxes of three: 48 and 54 ms per step instead of 37-38)
            # Every step is timed on its own and the leg's rate is the MEDIAN step's: a process's first queries over a new table still
            # allocate now and then (the third one pins the buffers of the key column's early copy: one 159-ms leg of three steps in six
            # runs of the final tree, 110-115 in the others); the steps are all in `step_ms`.
            for _ in range(3):
                big_step()
            sync()
            step_ms, rb = [], None
            for _ in range(args.rows_1e10_steps):
                t0s = time.perf_counter()
                rb = big_step()
                sync()
                step_ms.append((time.perf_counter() - t0s) * 1e3)
            med = sorted(step_ms)[len(step_ms) // 2]
            db = med * 1e-3 * args.rows_1e10_steps
            e = rate(big_rows * args.rows_1e10_steps, db, 16, f"the headline query over 1e10 rows resident on one GPU (160 GB): the median of {args.rows_1e10_steps} steps, each timed on "
                                                                 "its own (launch to synchronisation), after 3 warm-up steps; `ms` = that median x the step count")
            e["ms_per_step"] = med
            e["step_ms"] = [round(x, 3) for x in step_ms]
            e["roofline"]["end_to_end_frac"] = e["roofline"]["frac"]
            e["verified_sum_of_group_sums_equals_ungrouped_sum"] = sum_of_sums_check(tb, rb, big_rows)
            # where the step goes: one more step with the library's HIP-event profiler on (the events serialise the kernel chain: the
            # instrumented step is a few per cent slower than the timed ones; the budget is scaled to the timed step)
            try:
                sync()
                ex.profile_reset()
                ex.profile_enable(True)
                t0b = time.perf_counter()
                big_step()
                sync()
                instr_ms = (time.perf_counter() - t0b) * 1e3
                ex.profile_enable(False)
                pb = {p_["kernel"]: p_ for p_ in ex.profile_snapshot()}
                k_ms = {k_: round(v_["total_ms"], 3) for k_, v_ in pb.items()}
                known = sum(k_ms.values())
                e["budget_of_one_instrumented_step_ms"] = {
                    "pass1_partition": k_ms.get("partition", 0.0), "pass2_partition_agg": k_ms.get("partition_agg", 0.0),
                    "other_kernels": round(known - k_ms.get("partition", 0.0) - k_ms.get("partition_agg", 0.0), 3),
                    "launch_gaps_host_and_result_download": round(instr_ms - known, 3), "instrumented_step_total": round(instr_ms, 3),
                    "launches": {k_: v_["launches"] for k_, v_ in pb.items() if k_ in ("partition", "partition_agg")},
                    "pass1_avg_launch_ms": round(pb["partition"]["total_ms"] / pb["partition"]["launches"], 4) if "partition" in pb else None,
                    "pass1_roofline_frac": round(pb["partition"]["algo_bytes"] / pb["partition"]["total_ms"] * 1e-6 / HBM_PEAK_GBPS, 4) if "partition" in pb else None}
            except Exception as be:
                e["budget_of_one_instrumented_step_ms"] = {"error": str(be)[:200]}
            e["verified_vs_oracle_first_rows"] = "see extra.verified_vs_oracle: the first rows of this table ARE the headline table's (same generator, seed, row 0), same batch width and strategy"

            def verify_tail():
                # the query over a row-range scan of THIS table (dfx_table_scan_range_new: zero-copy slices that start 158 GB into the columns)
                rel = tb.scan(args.batch_rows, tail_row0, big_rows - tail_row0)
                rel = ex.FilterRelation(rel, ex.compile_scalar_expr(None, pred, schema), schema)
                got = ex.AggregateRelation(None, rel, [ex.compile_scalar_expr(None, Column(0), schema)], [ex.compile_expr(None, sum_v, schema)]).next()
                _secs, kept, want = bg["rows_1e10_tail"].get()
                g, w = by_key(got), by_key(want)
                ok = len(g[0]) == len(w[0]) and np.array_equal(g[0], w[0]) and np.array_equal(g[1].view(np.uint64), w[1].view(np.uint64))
                return {"rows": int(big_rows - tail_row0), "first_row": int(tail_row0), "groups": int(len(w[0])), "rows_passing": int(kept), "ok": bool(ok),
                        "what": "the headline query over the LAST rows of the 10^10-row table (row indices > 2^32), scanned in place, every group's SUM bit-exact "
                                "vs the CPU oracle over the same row range of the same generator"}
            e["verified_vs_oracle"] = checked("rows_1e10_tail", verify_tail)
            extra["rows_1e10"] = e
            # the N = 1 anchor of the multi-GPU curve: N > 1 ranks share config 4's 10^10 rows, so their line divides by THIS rate
            # (one GPU over the same 10^10 rows), not by the 10^9-row headline above
            if e.get("rows_per_s"):
                extra["scaling_anchor_rows_per_s"] = e["rows_per_s"]
            del tb
            ex.set_option("pool.trim", 1)
        except Exception as e:  # e.g. a box with less free HBM: a measurement, not a gate
            extra["rows_1e10"] = {"error": str(e)[:300]}

    cpu_baseline = None
    verified_vs_oracle = None
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        import oracle
        for b in bg.values():  # the timed baseline below runs alone on the host
            b.t.join()
        sample = min(int(args.cpu_sample_rows), n_rows)
        secs, kept, want = oracle.run_synth_query(syn, seed, 0, sample, 1024, pred, [Column(0)], [sum_v, count_v], want_result=True)
        cpu_baseline = {"value": sample / secs, "unit": "rows/s", "cores": 1, "kind": "port",
                        "sample": f"first {sample} rows of the same table, same query (+ COUNT), 1024-row batches "
                                  f"(reference-shaped C restatement, oracle/dfx_oracle.c), {secs:.2f} s",
                        "host_cores_available": os.cpu_count(), "host_cpu_budget_of_this_container": host_cpu_budget()}
        # per-group parity at the benchmark's size: the same row slice through the product path (same batch width, same
        # automatic strategy => partitioned), every group compared with the oracle bit for bit (exact distribution)
        try:
            t_s = table if (table is not None and sample == n_rows) else ex.DeviceTable.synth(syn, seed, 0, sample)
            got = build_on(t_s, schema, pred, [Column(0)], [sum_v]).next()             # the timed query itself (static signature, narrow rows, lean pass 2)
            got2 = build_on(t_s, schema, pred, [Column(0)], [sum_v, count_v]).next()   # SUM + COUNT (generic row width)
            gk, gs = by_key(got)
            g2k, g2s, g2c = by_key(got2)
            wk, ws, wc = by_key(want)
            ok = bool(len(gk) == len(wk) and np.array_equal(gk, wk) and np.array_equal(gs.view(np.uint64), ws.view(np.uint64))
                      and np.array_equal(g2k, wk) and np.array_equal(g2s.view(np.uint64), ws.view(np.uint64))
                      and np.array_equal(g2c, wc) and int(g2c.sum()) == kept)
            verified_vs_oracle = {"rows": sample, "groups": int(len(wk)), "rows_passing": int(kept), "ok": ok,
                                  "what": "SUM bit-exact for every group of the timed query, and SUM + COUNT of its two-aggregate "
                                          f"variant, GPU (partitioned strategy, {args.batch_rows}-row batches) vs CPU oracle over the same rows"}
            del t_s, got, got2
        except Exception as e:  # a failed check must show up in the line, not kill the measurement
            verified_vs_oracle = {"rows": sample, "ok": False, "error": str(e)[:300]}
        extra["verified_vs_oracle"] = verified_vs_oracle

    if rank == 0:
        line = {
            "metric": "rows/sec filter+GROUP-BY-SUM over Float64 Arrow",
            "value": value, "unit": "rows/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms_per_step, "higher_is_better": True,
            # one GPU runs config 3's size (1e9 rows); N > 1 GPUs share config 4's 1e10 rows (total work fixed)
            "scaling": "weak" if (world == 1 or args.rows > 0) else "strong", "vs_baseline": None,
            "dtype": "f64", "data": "synthetic",
            "config": {"workload": "SELECT k, SUM(v) FROM t WHERE v > 204.8 AND v < 409.6 GROUP BY k; "
                                   f"{n_rows} rows/GPU, k Int64 uniform 1e6 keys, v Float64 exact (m*2^-10)"
                                   + ("" if world == 1 else f" (BASELINE config 4: {total_rows} rows over {world} GPUs)"),
                       "rows_per_gpu": n_rows, "rows_total": total_rows, "batch_rows": args.batch_rows,
                       "algorithmic_bytes_per_row": 16, "parallelism": f"rows range-partitioned x{world}, "
                       "group partials all-to-all" if world > 1 else "single GPU", "exchange": exchange_mode,
                       # the ranks RCCL itself reports for the library's communicator (ncclCommCount): N means the exchange ran
                       # over RCCL between N ranks; null: no library communicator (one GPU, or the host-driven fallback)
                       "rccl_ranks": (comm.ranks() if comm is not None else None)},
            "roofline": roofline, "cpu_baseline": cpu_baseline, "extra": extra,
        }
        emit_line(line, args.full_out)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
