// dfx_k_partition_v25.hip -- pass 1 of the partitioned GROUP BY over the Int32 shadow of the key column (PTF_KEY4: two keys per lane, StaticKey4Policy): Static SigKeySumPred2F64 (key + SUM under a two-sided f64 predicate: the headline query).
#include "dfx_k_partition_ws_inl.hpp"
namespace dfx {
DFX_PARTITION_VARIANT_WS_ONLY(25, DFX_ARG(StaticKey4Policy<4, SigKeySumPred2F64>), DFX_ARG(StaticKey4Policy<8, SigKeySumPred2F64>))
}  // namespace dfx
