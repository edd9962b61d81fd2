// dfx_k_distinct3.hip -- COUNT(DISTINCT) set kernels for 3-word tuples (see dfx_k_distinct_inl.hpp).
#include "dfx_k_distinct_inl.hpp"

namespace dfx {
DFX_INSTANTIATE_DISTINCT_KW(3)
}  // namespace dfx
