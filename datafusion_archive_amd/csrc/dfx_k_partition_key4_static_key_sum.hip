// dfx_k_partition_key4_static_key_sum.hip -- pass 1 of the partitioned GROUP BY, unit key4_static_key_sum (dfx_pass1_units.hpp): key + SUM without a predicate over the key column's Int32 shadow.
#include "dfx_k_partition_ws_inl.hpp"
DFX_PASS1_UNIT(key4_static_key_sum, StaticKey4Unit<SigKeySum>)
