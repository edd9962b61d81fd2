// dfx_k_distinct2.hip -- COUNT(DISTINCT) set kernels for 2-word tuples (see dfx_k_distinct_inl.hpp).
#include "dfx_k_distinct_inl.hpp"

namespace dfx {
DFX_INSTANTIATE_DISTINCT_KW(2)
}  // namespace dfx
