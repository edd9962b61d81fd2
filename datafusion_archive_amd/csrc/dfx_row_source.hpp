// dfx_row_source.hpp -- how a lane gets its row in the kernels that scan rows through a fused program: THE ladder, once.
// A launch tries, in this order: a compile-time signature (StaticPolicy, dfx_sigs.hpp), the scan plan (PlanPolicyN: the batch
// has nulls or 4-byte columns, or scan.plan = 2), a refusal (the host relies on a plan that did not bind), the run-time decoded
// shape (FastPolicy), the SSA interpreter (InterpPolicy) -- the last three by column class (<= 2 / <= 4 / <= 8 referenced
// columns).  The eight kernels differ in which rungs they have; kScanLadder holds those differences as data, every launcher
// (dfx_k_filter.hip, dfx_k_core.hip, dfx_k_reduce.hip, dfx_k_table_inl.hpp, dfx_k_fewgroup.hip, dfx_k_distinct_inl.hpp, the tail
// of select_pass1) switches on the answer, and fewgroup_supported and the explain() texts ask the same code.
// Host only and free of HIP: tests/native/row_source_check.cpp holds the choice against a table written out by hand.
#pragma once
#include "dfx_device.hpp"
#include "dfx_sigs.hpp"

namespace dfx {

#define DFX_SCAN_KERNELS(X) \
  X(predicate_mask) X(filter_fused) X(project) X(reduce) X(hash_agg) X(fewgroup) X(distinct_insert) X(pass1_generic)

// sig_*: a compile-time signature.  plan_c<C>: the scan plan bound to <= 2 / <= 4 plan columns.  fast_c<C> / interp_c<C>: the
// decoded shape / the interpreter over <= 2 / <= 4 / <= 8 program columns.
#define DFX_ROW_SOURCES(X)                                                                                              \
  X(sig_pred2_f64) X(sig_count_pred2_f64) X(sig_sum_count_pred2_f64) X(sig_key_sum_pred2_f64) X(sig_key_sum) X(sig_q1) \
  X(plan_c2) X(plan_c4) X(fast_c2) X(fast_c4) X(fast_c8) X(interp_c2) X(interp_c4) X(interp_c8)

enum class ScanKernel : int {
#define X(name) name,
  DFX_SCAN_KERNELS(X)
#undef X
};
enum class RowSource : int {
  none = -1,  // no kernel of this launcher takes the launch: it returns its error
#define X(name) name,
  DFX_ROW_SOURCES(X)
#undef X
};
#define X(name) +1
constexpr int kScanKernels = 0 DFX_SCAN_KERNELS(X);
constexpr int kRowSources = 0 DFX_ROW_SOURCES(X);
#undef X
#define X(name) #name,
constexpr const char* kScanKernelName[kScanKernels] = {DFX_SCAN_KERNELS(X)};
constexpr const char* kRowSourceName[kRowSources] = {DFX_ROW_SOURCES(X)};
#undef X

// a plan_* launch reads the plan's own fast plan and columns (what bind_scan_plan filled), every other the caller's
constexpr bool is_plan(RowSource r) { return r == RowSource::plan_c2 || r == RowSource::plan_c4; }

typedef bool (*SigMatch)(const DevProgram&, const DevFastPlan&, int, int, const uint8_t*, const uint8_t*);
struct SigRung {
  RowSource source;
  int kw;            // the key words the launcher tries it at
  SigMatch matches;  // nullptr: no rung
};
constexpr SigRung kNoSig = {RowSource::none, 0, nullptr};

enum class PlanWhen : uint8_t {
  never,
  batch_needs_it,  // validity bitmaps, 4-byte columns, or scan.plan = 2
  fast_valid       // scan.plan != 0 and a decoded shape: plain columns, whatever the batch
};
enum class Refusal : uint8_t {
  never,
  plan_relied_on,         // plan_mode bit 2 and no bound plan, asked for or not
  plan_asked_and_needed   // a plan was asked for and did not bind, and the batch has nulls or plan_mode bit 2
};

struct ScanLadder {
  ScanKernel kernel;
  int max_kw, max_na;  // 0: any; else the launcher takes 1..max_kw key words and 1..max_na aggregates only
  SigRung sig[3];
  PlanWhen plan;
  Refusal refuse;
  bool fast, interp;
  bool c2;  // the <= 2 column class exists (<= 4 and <= 8 always do)
};

constexpr ScanLadder kScanLadder[kScanKernels] = {
    // the common ladder of the kernels without keys or aggregates: one signature, no plan (intended: their null rule is the interpreter's)
    {ScanKernel::predicate_mask, 0, 0, {{RowSource::sig_pred2_f64, 0, &sig_matches<SigPred2F64>}, kNoSig, kNoSig},
     PlanWhen::never, Refusal::never, true, true, true},
    {ScanKernel::filter_fused, 0, 0, {{RowSource::sig_pred2_f64, 0, &sig_matches<SigPred2F64>}, kNoSig, kNoSig},
     PlanWhen::never, Refusal::never, true, true, true},
    // interpreter only (intended: a projection computes values, the decoded shapes and the plan are predicates and plain operands)
    {ScanKernel::project, 0, 0, {kNoSig, kNoSig, kNoSig}, PlanWhen::never, Refusal::never, false, true, true},
    // the full ladder
    {ScanKernel::reduce, 0, 0,
     {{RowSource::sig_count_pred2_f64, 0, &sig_matches<SigCountPred2F64>}, {RowSource::sig_sum_count_pred2_f64, 0, &sig_matches<SigSumCountPred2F64>}, kNoSig},
     PlanWhen::batch_needs_it, Refusal::plan_relied_on, true, true, true},
    {ScanKernel::hash_agg, 0, 0,
     {{RowSource::sig_key_sum_pred2_f64, 1, &sig_matches<SigKeySumPred2F64>}, {RowSource::sig_key_sum, 1, &sig_matches<SigKeySum>}, {RowSource::sig_q1, 2, &sig_matches<SigQ1>}},
     PlanWhen::batch_needs_it, Refusal::plan_relied_on, true, true, true},
    // one or two key words, up to four aggregates (intended: the accumulators live in registers).  No interpreter (intended: its
    // registers are the accumulators').  The refusal sits inside the plan branch and adds has_nulls, so plan_mode bit 2 alone
    // does not refuse a batch that never asked for a plan: kept as found.
    {ScanKernel::fewgroup, 2, 4, {{RowSource::sig_q1, 2, &sig_matches<SigQ1>}, kNoSig, kNoSig},
     PlanWhen::batch_needs_it, Refusal::plan_asked_and_needed, true, false, true},
    // the plan for every decoded shape, not only where the batch needs it (intended: the tuple's columns are plain columns, the
    // plan's loads are the fastest there are); no signature, no FastPolicy, no <= 2 column class: kept as found.
    {ScanKernel::distinct_insert, 0, 0, {kNoSig, kNoSig, kNoSig}, PlanWhen::fast_valid, Refusal::never, false, true, false},
    // what select_pass1 (dfx_k_partition.hip) has left when neither a signature nor the plan took the launch: it tried both, and
    // refused, before it asks
    {ScanKernel::pass1_generic, 0, 0, {kNoSig, kNoSig, kNoSig}, PlanWhen::never, Refusal::never, true, true, true},
};
#define X(name) && kScanLadder[(int)ScanKernel::name].kernel == ScanKernel::name
static_assert(true DFX_SCAN_KERNELS(X), "kScanLadder is indexed by ScanKernel");
#undef X

// Step 1: does this launch try the scan plan?  (Asked before the signatures: under scan.plan = 2 a launch that a signature takes
// binds a plan it does not run -- host work of an A/B setting, no kernel sees it.)
inline bool wants_scan_plan(ScanKernel kernel, const DevProgram& P, const DevFastPlan& fast) {
  switch (kScanLadder[(int)kernel].plan) {
    case PlanWhen::batch_needs_it: return P.has_nulls || !P.wide8 || (fast.plan_mode & 3) == 2;
    case PlanWhen::fast_valid: return (fast.plan_mode & 3) != 0 && fast.valid;
    default: return false;
  }
}

// Step 2.  plan_bound / plan_cols: whether bind_scan_plan bound the batch (asked only where wants_scan_plan said so) and its
// DevScanPlan::n_cols.  kw, na, acc_kind, val_xform: the table's, as sig_matches takes them (kernels without: 0 and zeroes).
inline RowSource choose_row_source(ScanKernel kernel, const DevProgram& P, const DevFastPlan& fast, int kw, int na, const uint8_t* acc_kind,
                                   const uint8_t* val_xform, bool plan_bound, int plan_cols) {
  const ScanLadder& L = kScanLadder[(int)kernel];
  if (L.max_kw != 0 && !(kw >= 1 && kw <= L.max_kw && na >= 1 && na <= L.max_na)) return RowSource::none;
  for (const SigRung& s : L.sig)
    if (s.matches != nullptr && kw == s.kw && s.matches(P, fast, kw, na, acc_kind, val_xform)) return s.source;
  const bool asked = wants_scan_plan(kernel, P, fast);
  if (asked && plan_bound) return plan_cols <= 2 ? RowSource::plan_c2 : RowSource::plan_c4;
  if (L.refuse == Refusal::plan_relied_on && (fast.plan_mode & 4)) return RowSource::none;
  if (L.refuse == Refusal::plan_asked_and_needed && asked && (P.has_nulls || (fast.plan_mode & 4))) return RowSource::none;
  const int cls = P.n_cols <= 2 && L.c2 ? 0 : P.n_cols <= 4 ? 1 : 2;
  constexpr RowSource kFast[3] = {RowSource::fast_c2, RowSource::fast_c4, RowSource::fast_c8};
  constexpr RowSource kInterp[3] = {RowSource::interp_c2, RowSource::interp_c4, RowSource::interp_c8};
  if (L.fast && fast.valid && !P.has_nulls) return kFast[cls];
  return L.interp ? kInterp[cls] : RowSource::none;
}

// The answer where there are no bound columns to try a plan on (fewgroup_supported, explain()): the plan counts as bound where
// scan_plan_shape_ok (plan_shape_ok: the caller's, dfx_scan_plan.hpp) says it can be built; it then has one slot per program column.
inline RowSource row_source_without_batch(ScanKernel kernel, const DevProgram& P, const DevFastPlan& fast, int kw, int na,
                                          const uint8_t* acc_kind, const uint8_t* val_xform, bool plan_shape_ok) {
  const bool bound = wants_scan_plan(kernel, P, fast) && (fast.plan_mode & 3) != 0 && plan_shape_ok;
  return choose_row_source(kernel, P, fast, kw, na, acc_kind, val_xform, bound, P.n_cols);
}

// explain(): the row source in words.  r: row_source_without_batch of the operator's program as built -- no batch bound, so the
// plan where one can be built, which is what the texts say.
inline const char* row_source_prose(ScanKernel kernel, RowSource r, int kw) {
  const bool filter = kernel == ScanKernel::predicate_mask || kernel == ScanKernel::filter_fused;
  switch (r) {
    case RowSource::sig_pred2_f64: return "static shape Pred2F64";
    case RowSource::sig_count_pred2_f64: return "static shape CountPred2F64";
    case RowSource::sig_sum_count_pred2_f64: return "static shape SumCountPred2F64";
    case RowSource::sig_key_sum_pred2_f64: return "static shape KeySumPred2F64";
    case RowSource::sig_key_sum: return "static shape KeySum";
    case RowSource::sig_q1: return "static shape Q1";
    case RowSource::plan_c2:
    case RowSource::plan_c4:
      return kw == 0   ? "scan plan where a batch has nulls or 4-byte columns (PlanPolicy: range tests on value images), else column-op-literal shape (FastPolicy)"
             : kw == 1 ? "scan plan (PlanPolicy: range tests on value images, 4-byte columns widened, nulls by arrow's rule; every kernel of the partitioned strategy, the other strategies where a batch has nulls or 4-byte columns)"
                       : "scan plan where a batch has nulls or 4-byte columns (PlanPolicy), else column-op-literal shape (FastPolicy)";
    case RowSource::fast_c2:
    case RowSource::fast_c4:
    case RowSource::fast_c8:
      return filter ? "column-op-literal conjunction (FastPolicy; interpreter when a batch has nulls)"
                    : "column-op-literal shape (FastPolicy; interpreter when a batch has nulls)";
    default: return "SSA interpreter";
  }
}

}  // namespace dfx
