// dfx_k_distinct1.hip -- COUNT(DISTINCT) set kernels for 1-word tuples (ungrouped), and the dispatch over the tuple width
// (see dfx_k_distinct_inl.hpp; the other widths are instantiated in dfx_k_distinct{2,3,4,8}.hip).
#include "dfx_k_distinct_inl.hpp"

namespace dfx {
DFX_INSTANTIATE_DISTINCT_KW(1)

#define DFX_DECLARE_DISTINCT_KW(KW)                                                                                          \
  extern template hipError_t distinct_insert<KW>(const DevProgram&, const DevFastPlan&, const DevColumns&, const DevAggPlan&, \
                                                 int, const DevTable&, const DevRows&, int64_t, bool*, hipStream_t);          \
  extern template hipError_t distinct_count<KW>(const DevTable&, const DevTable&, uint64_t*, hipStream_t);                    \
  extern template hipError_t distinct_lookup<KW>(const DevTable&, const DevDistinctKeys&, int, int64_t, uint64_t*, hipStream_t);
DFX_DECLARE_DISTINCT_KW(2)
DFX_DECLARE_DISTINCT_KW(3)
DFX_DECLARE_DISTINCT_KW(4)
DFX_DECLARE_DISTINCT_KW(8)

#define DFX_DISTINCT_DISPATCH(kw, CALL) \
  switch (kw) {                         \
    case 1: return CALL(1);             \
    case 2: return CALL(2);             \
    case 3: return CALL(3);             \
    case 4: return CALL(4);             \
    case 8: return CALL(8);             \
    default: return hipErrorInvalidValue; \
  }

hipError_t launch_distinct_insert(const DevProgram& P, const DevFastPlan& fast, const DevColumns& C, const DevAggPlan& plan, int kw_out,
                                  const DevTable& T, const DevRows& spill, int64_t n, bool* plan_kernel, hipStream_t s) {
  *plan_kernel = false;
  if (n <= 0) return hipSuccess;
  Scope sc(KID_DISTINCT_INSERT, s, 0);
#define CALL(K) distinct_insert<K>(P, fast, C, plan, kw_out, T, spill, n, plan_kernel, s)
  DFX_DISTINCT_DISPATCH(T.kw, CALL)
#undef CALL
}

hipError_t launch_distinct_count(const DevTable& S, const DevTable& Cnt, uint64_t* total, hipStream_t s) {
  Scope sc(KID_DISTINCT_COUNT, s, 0);
#define CALL(K) distinct_count<K>(S, Cnt, total, s)
  DFX_DISTINCT_DISPATCH(S.kw, CALL)
#undef CALL
}

hipError_t launch_distinct_lookup(const DevTable& Cnt, const DevDistinctKeys& K, int kw_out, int64_t n, uint64_t* out, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  Scope sc(KID_DISTINCT_COUNT, s, 0);
#define CALL(K_) distinct_lookup<K_>(Cnt, K, kw_out, n, out, s)
  DFX_DISTINCT_DISPATCH(Cnt.kw, CALL)
#undef CALL
}
}  // namespace dfx
