// dfx_k_partition.hip -- partitioned GROUP BY: the pass-1 dispatcher (select_pass1, launch_partition), the probe for wide keys
// (k_probe_wide_keys).  The pass-1 kernels and the description of the strategy are in dfx_k_partition_inl.hpp; their
// instantiations are in dfx_k_partition_<unit>.hip, one file per unit of dfx_pass1_units.hpp; the kernels' LDS bytes and what
// launch_partition accepts (partition_launchable) are in dfx_pass1_layout.hpp; pass 2 is dfx_k_pass2.hip.
#include "dfx_k_partition_ws_inl.hpp"

namespace dfx {

// does the (single-word-key) table hold a key that has no 32-bit image?  Run once, after the calibration slice.
__global__ __launch_bounds__(256) void k_probe_wide_keys(const DevTable T) {
  const uint64_t n = T.mask + 1;
  bool wide = false;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) {
    const uint64_t k = T.keys[i];
    if (k != kEmptyKey) {
      uint64_t key1[1] = {k};
      wide = wide || (k >> 32) != 0 || (uint32_t)(hash_keys<1>(key1) >> 32) >= kTagForeign;
    }
  }
  if (__ballot(wide) != 0 && lane_id() == 0) __hip_atomic_store(&T.ctrl[CTRL_WIDE_KEYS], 1u, RLX_AGENT);
  if (blockIdx.x == 0 && threadIdx.x == 0 && __hip_atomic_load(&T.ctrl[CTRL_SENTINEL], RLX_AGENT) != 0u)
    __hip_atomic_store(&T.ctrl[CTRL_WIDE_KEYS], 1u, RLX_AGENT);  // the key i64::MIN lives outside the slots
}
hipError_t launch_probe_wide_keys(const DevTable& T, hipStream_t s) {
  if (T.kw != 1) return hipSuccess;
  hipLaunchKernelGGL(k_probe_wide_keys, dim3(1024), dim3(256), 0, s, T);
  return hipGetLastError();
}

// the pass-1 units (dfx_pass1_units.hpp; dfx_k_partition_<unit>.hip defines launch_pass1_<unit>)
#define X(name) void launch_pass1_##name(DFX_PASS1_ARGS);
DFX_PASS1_UNITS(X)
#undef X
typedef void (*Pass1Launch)(DFX_PASS1_ARGS);
#define X(name) launch_pass1_##name,
static const Pass1Launch kPass1Launch[kPass1Units] = {DFX_PASS1_UNITS(X)};
#undef X

// What select_pass1 decides: the unit that takes a launch and what it is launched with.
struct Pass1Choice {
  Pass1Unit unit = Pass1Unit::none;  // none: no pass-1 kernel takes this launch
  bool bound = false;                // the scan plan bound the batch: the launch takes fp / cp in place of the caller's fast plan and columns
  DevFastPlan fp;
  DevColumns cp;
  DevPartition PT;       // the launch's: the pair scan's slot and transform filled in, PTF_WS stripped for fast_* / interp_*
  size_t lds_bytes = 0;  // of that PT
};

// The compile-time signature this program matches, as its static_* unit.  raw (PTF_SHARED): pass 1 routes the aggregates' common
// RAW operand -- the shape of a one-aggregate query whose operand is that column (what the accumulators do with it is pass 2's
// business).
static Pass1Unit signature_unit(const DevProgram& P, const DevFastPlan& fast, const DevTable& T, bool raw) {
  static_assert(SigKeySumPred2F64::acc(0) == ACC_ADD_F64 && SigKeySum::acc(0) == ACC_ADD_F64 && SigKeyAffSumPred2F64::acc(0) == ACC_ADD_F64 &&
                    SigKeySumPred2F64::xf(0) == VT_RAW && SigKeySum::xf(0) == VT_RAW && SigKeyAffSumPred2F64::xf(0) == VT_RAW,
                "the one-aggregate signatures add the raw operand");
  const uint8_t raw_kind[1] = {ACC_ADD_F64}, raw_xf[1] = {VT_RAW};
  const int na = raw ? 1 : T.na;
  const uint8_t* kind = raw ? raw_kind : T.acc_kind;
  const uint8_t* xf = raw ? raw_xf : T.val_xform;
  if (sig_matches<SigKeySumPred2F64>(P, fast, 1, na, kind, xf)) return Pass1Unit::static_key_sum_pred2;
  if (sig_matches<SigKeySum>(P, fast, 1, na, kind, xf)) return Pass1Unit::static_key_sum;
  if (sig_matches<SigKeyAffSumPred2F64>(P, fast, 1, na, kind, xf)) return Pass1Unit::static_key_aff_sum_pred2;
  return Pass1Unit::none;
}

// The scan plan (DevScanPlan): run-time shapes as data.  Which binding a launch needs follows from the kernel flavour that
// will run: the one-value flavours (narrow rows, the wave-specialised kernel) find the key in slot 0 and the routed value in
// slot 1 (PlanPolicy1), the others look their slots up.  false: the plan does not take this launch (c->unit stays none).
static bool select_plan_unit(const DevProgram& P, const DevFastPlan& fast, const DevColumns& C, const DevTable& T, const DevPartition& PT, Pass1Choice* c) {
  const bool shared = (PT.flags & PTF_SHARED) != 0;
  const bool pair = (PT.flags & PTF_PAIR) != 0;  // two operands per routed row: the multi-value binding (slot look-ups) in the wave-specialised kernel
  const bool key4 = (PT.flags & PTF_KEY4) != 0;
  const bool one_value = !pair && ((PT.flags & PTF_WS) || ((PT.mode & 15u) == 2 && (PT.flags & PTF_NARROW)));
  if (one_value && !shared && T.na != 1) return false;
  if (pair && (T.na < 2 || T.kw != 1 || !(PT.flags & PTF_WS))) return false;
  const uint8_t raw_xf[kMaxAggs] = {VT_RAW};
  // (a pair scan whose key is the only 4-byte column -- the Int32 shadow -- has kernels of its own: asked for under PTF_KEY4 alone)
  if (!bind_scan_plan(P, fast, C, 1, shared ? 1 : T.na, shared ? raw_xf : T.val_xform, one_value, &c->fp, &c->cp, pair && key4)) return false;
  const Pass1Unit unit = plan_unit(c->fp.scan.n_cols, c->fp.scan.gen, pair, one_value, key4);
  if (unit == Pass1Unit::none) return false;
  c->unit = unit;
  c->bound = true;
  if (pair) {  // operand 1: the plan slot and the transform of its first accumulator
    const uint32_t a1 = PT.pair_arg1 < (uint32_t)kMaxAggs ? PT.pair_arg1 : 1u;
    c->PT.pair_slot1 = c->fp.scan.argslot[a1];
    c->PT.pair_xf1 = T.val_xform[a1];
  }
  return true;
}

// Which pass-1 unit takes this launch, and with what?  Host only, no launch: launch_partition runs the answer, the
// partition_*_supported queries below predict it from the same code.  P, fast, C: the batch as the launch binds it -- under
// PTF_KEY4 the key column is its Int32 shadow (T_U32).
static Pass1Choice select_pass1(const DevProgram& P, const DevFastPlan& fast, const DevColumns& C, const DevTable& T, const DevPartition& PT) {
  Pass1Choice c;
  c.PT = PT;
  c.lds_bytes = partition_stage_bytes(PT);
  const bool shared = (PT.flags & PTF_SHARED) != 0;
  const bool plan_first = (fast.plan_mode & 3) == 2;  // (A/B: scan.plan = 2)
  // regions of 8-byte rows (PTF_ROW8) take the launches that bind both shadows and no other: not the caller's word for it
  if (!partition_row8_consistent(PT.flags)) return c;
  if (PT.flags & PTF_KEY4) {
    // The two signatures that have a two-keys-per-lane kernel (StaticKey4Policy: the wave-specialised kernel alone) describe the
    // 8-byte binding; whatever else the scan plan binds with the key as an unsigned 4-byte column: its one-value kernels
    // (plan_c2_g4, plan_c4_g4) and the pair kernels (pair_key4_*), one 4-byte load per lane.
    if ((PT.flags & PTF_WS) && !(PT.flags & PTF_PAIR) && (PT.flags & PTF_NARROW) && !plan_first && T.kw == 1) {
      DevProgram P8 = P;
      if (fast.valid && fast.keycol[0] < kMaxCols) P8.col_dtype[fast.keycol[0]] = T_I64;
      // PTF_VAL4: ... and the operand -- the other of the two columns -- its Float32 shadow (T_F32), which the same two units
      // widen back to the column's own values (StaticKey4Val4Policy)
      if ((PT.flags & PTF_VAL4) && fast.valid && P.n_cols == 2 && fast.keycol[0] < 2 && P.col_dtype[1 - fast.keycol[0]] == T_F32)
        P8.col_dtype[1 - fast.keycol[0]] = T_F64;
      const Pass1Unit sig = signature_unit(P8, fast, T, shared);
      if (sig == Pass1Unit::static_key_sum_pred2) c.unit = Pass1Unit::key4_static_key_sum_pred2;
      if (sig == Pass1Unit::static_key_sum) c.unit = Pass1Unit::key4_static_key_sum;
      if (c.unit != Pass1Unit::none) return c;
    }
    if (PT.flags & PTF_VAL4) return c;  // (no other kernel reads an operand's shadow: partition_value_shadow_supported said so)
    select_plan_unit(P, fast, C, T, PT, &c);
    return c;
  }
  if (PT.flags & PTF_PAIR) {  // (the host asked partition_pair_supported first: a batch the plan cannot bind is its error to handle)
    select_plan_unit(P, fast, C, T, PT, &c);
    return c;
  }
  if (plan_first && select_plan_unit(P, fast, C, T, PT, &c)) return c;
  c.unit = signature_unit(P, fast, T, shared);
  if (c.unit != Pass1Unit::none) return c;
  // everything else the plan covers: any single MIN / MAX / COUNT / SUM, one to four terms over Int32 ... Float64 columns,
  // nullable columns -- same kernels, the query is data (the wave-specialised flavour included: its scan loop stays short)
  if (!plan_first && select_plan_unit(P, fast, C, T, PT, &c)) return c;
  if (PT.flags & PTF_PLANES) return c;  // (the host asked partition_planes_supported first; the ring kernels below write another geometry)
  if (fast.plan_mode & 4) return c;     // (the host fused a predicate over nulls counting on a plan)
  // The wave-specialised flavour pays when the scan loop is short (compile-time signatures).  The run-time decoded shapes and
  // the interpreter spend several times as many instructions per row group: eight scanner waves cannot keep up, sixteen
  // symmetric ones can (measured with PTF_WS on every policy: FastPolicy queries -25 %, the interpreter -28 %).  Same regions,
  // counts and padding either way, so the choice is made per launch.
  c.PT.flags &= ~PTF_WS;
  c.lds_bytes = partition_stage_bytes(c.PT);
  switch (choose_row_source(ScanKernel::pass1_generic, P, fast, T.kw, T.na, T.acc_kind, T.val_xform, false, 0)) {
    case RowSource::fast_c2: c.unit = Pass1Unit::fast_c2; break;
    case RowSource::fast_c4: c.unit = Pass1Unit::fast_c4; break;
    case RowSource::fast_c8: c.unit = Pass1Unit::fast_c8; break;
    case RowSource::interp_c2: c.unit = Pass1Unit::interp_c2; break;
    case RowSource::interp_c4: c.unit = Pass1Unit::interp_c4; break;
    case RowSource::interp_c8: c.unit = Pass1Unit::interp_c8; break;
    default: break;  // (no other source in this ladder)
  }
  return c;
}

// PTF_PAIR: can THIS bound batch go through the pair kernels?  (the plan binds it, three or four plan columns)
bool partition_pair_supported(const DevProgram& P, const DevFastPlan& fast, const DevColumns& C, const DevTable& T) {
  if (!kNarrowLine || T.na < 2 || T.kw != 1) return false;
  if (T.na > 2 && P.has_nulls && fast.np == 0) return false;  // (three and more aggregates: the operands travel raw -- see partition_planes_supported)
  DevPartition PTq = {};
  PTq.flags = PTF_WS | PTF_PAIR;
  Pass1Choice c;
  return select_plan_unit(P, fast, C, T, PTq, &c) && !(c.fp.scan.gen & 4);
}

// PTF_KEY4: does a pass-1 kernel read this program's key from 4-byte words?  P, fast, C: the batch as the operator bound it, the
// key (slot ks) an 8-byte integer column without nulls; PT: the launch's flags.  The plan refuses what it cannot widen -- an
// aggregate over the key itself, a product --: those launches keep the 8-byte column.
bool partition_key_shadow_supported(const DevProgram& P, const DevFastPlan& fast, const DevColumns& C, const DevTable& T, const DevPartition& PT) {
  if (!(PT.flags & PTF_WS) || T.kw != 1 || !fast.valid) return false;
  const int ks = fast.keycol[0];
  if (ks >= kMaxCols) return false;
  DevProgram P4 = P;
  P4.col_dtype[ks] = T_U32;  // (C's own 8-byte aligned base stands in for the shadow's)
  DevPartition PT4 = PT;
  PT4.flags = (PT4.flags & ~PTF_ROW8) | PTF_KEY4;  // (the question is about the shape; the row form follows from the answers)
  return select_pass1(P4, fast, C, T, PT4).unit != Pass1Unit::none;
}

// PTF_VAL4: does a pass-1 kernel read this launch's operand from 4-byte floats as well?  P, PT: the launch with the key shadow bound
// (the key T_U32, PTF_KEY4).  Only the two signatures' kernels do: two columns, the operand a plain Float64 column that every
// predicate term is on (sig_matches), SUM of it -- or, under PTF_SHARED, the raw operand of two or three aggregates of it.
// *operand_col: its slot.
bool partition_value_shadow_supported(const DevProgram& P, const DevFastPlan& fast, const DevColumns& C, const DevTable& T, const DevPartition& PT, int* operand_col) {
  if (!(PT.flags & PTF_KEY4) || !fast.valid || P.n_cols != 2 || fast.keycol[0] >= 2) return false;
  const int vc = 1 - fast.keycol[0];
  if (P.col_dtype[vc] != T_F64) return false;
  DevProgram P4 = P;
  P4.col_dtype[vc] = T_F32;
  DevPartition PT4 = PT;
  PT4.flags = (PT4.flags & ~PTF_ROW8) | PTF_VAL4;
  const Pass1Unit unit = select_pass1(P4, fast, C, T, PT4).unit;
  *operand_col = vc;
  return unit == Pass1Unit::key4_static_key_sum_pred2 || unit == Pass1Unit::key4_static_key_sum;
}

// PTF_PLANES: does THIS bound batch take the wave-specialised one-value pass 1 with the aggregates' common raw operand?
// (a compile-time signature of the raw shape, or the scan plan's fixed-slot binding)
bool partition_planes_supported(const DevProgram& P, const DevFastPlan& fast, const DevColumns& C, const DevTable& T) {
  // (nulls: a raw operand carries no validity.  Under an absorbed predicate nobody asks for it -- every surviving slot is valid,
  // filter.rs:83-92, DevScanPlan::count_valid --; without one COUNT would)
  if (!kNarrowLine || T.na < 2 || T.na > kMaxAggs || T.kw != 1 || (P.has_nulls && fast.np == 0)) return false;
  if ((fast.plan_mode & 3) != 2 && signature_unit(P, fast, T, true) != Pass1Unit::none) return true;
  DevPartition PTq = {};
  PTq.flags = PTF_WS | PTF_SHARED;
  Pass1Choice c;
  return select_plan_unit(P, fast, C, T, PTq, &c);
}

hipError_t launch_partition(const DevProgram& P, const DevFastPlan& fast, const DevColumns& C, const DevAggPlan& plan,
                            const DevTable& T, const DevPartition& PT, const DevRows& spill, int64_t n,
                            double algo_bytes, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  Scope sc(KID_PARTITION, s, algo_bytes);
  if (!partition_launchable(PT) || !partition_row8_consistent(PT.flags)) return hipErrorInvalidValue;
  const Pass1Choice c = select_pass1(P, fast, C, T, PT);
  if (c.unit == Pass1Unit::none) return hipErrorNotSupported;
  kPass1Launch[(int)c.unit](P, c.bound ? c.fp : fast, c.bound ? c.cp : C, plan, T, c.PT, spill, n, c.lds_bytes, s);
  return hipGetLastError();
}

}  // namespace dfx
