// dfx_k_partition_v26.hip -- pass 1 of the partitioned GROUP BY over the Int32 shadow of the key column (PTF_KEY4: two keys per lane, StaticKey4Policy): Static SigKeySum (key + SUM, no predicate).
#include "dfx_k_partition_ws_inl.hpp"
namespace dfx {
DFX_PARTITION_VARIANT_WS_ONLY(26, DFX_ARG(StaticKey4Policy<4, SigKeySum>), DFX_ARG(StaticKey4Policy<8, SigKeySum>))
}  // namespace dfx
