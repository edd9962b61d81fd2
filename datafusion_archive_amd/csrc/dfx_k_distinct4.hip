// dfx_k_distinct4.hip -- COUNT(DISTINCT) set kernels for 4-word tuples (see dfx_k_distinct_inl.hpp).
#include "dfx_k_distinct_inl.hpp"

namespace dfx {
DFX_INSTANTIATE_DISTINCT_KW(4)
}  // namespace dfx
