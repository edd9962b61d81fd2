// dfx_k_distinct8.hip -- COUNT(DISTINCT) set kernels for 8-word tuples (see dfx_k_distinct_inl.hpp).
#include "dfx_k_distinct_inl.hpp"

namespace dfx {
DFX_INSTANTIATE_DISTINCT_KW(8)
}  // namespace dfx
