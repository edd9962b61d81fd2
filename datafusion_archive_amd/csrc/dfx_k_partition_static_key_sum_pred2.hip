// dfx_k_partition_static_key_sum_pred2.hip -- pass 1 of the partitioned GROUP BY, unit static_key_sum_pred2 (dfx_pass1_units.hpp): key + SUM under a two-sided f64 predicate: the headline query.
#include "dfx_k_partition_ws_inl.hpp"
DFX_PASS1_UNIT(static_key_sum_pred2, StaticUnit<SigKeySumPred2F64>)
