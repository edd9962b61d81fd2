// dfx_k_partition_key4_static_key_sum_pred2.hip -- pass 1 of the partitioned GROUP BY, unit key4_static_key_sum_pred2 (dfx_pass1_units.hpp): the headline's signature over the key column's Int32 shadow.
#include "dfx_k_partition_ws_inl.hpp"
DFX_PASS1_UNIT(key4_static_key_sum_pred2, StaticKey4Unit<SigKeySumPred2F64>)
