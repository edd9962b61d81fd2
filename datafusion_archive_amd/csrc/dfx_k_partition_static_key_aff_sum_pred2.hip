// dfx_k_partition_static_key_aff_sum_pred2.hip -- pass 1 of the partitioned GROUP BY, unit static_key_aff_sum_pred2 (dfx_pass1_units.hpp): the headline's shape with SUM(v <+ - *> literal) as the argument.
#include "dfx_k_partition_ws_inl.hpp"
DFX_PASS1_UNIT(static_key_aff_sum_pred2, StaticUnit<SigKeyAffSumPred2F64>)
