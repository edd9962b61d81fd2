// dfx_k_partition_static_key_sum.hip -- pass 1 of the partitioned GROUP BY, unit static_key_sum (dfx_pass1_units.hpp): key + SUM, no predicate: BASELINE config 3.
#include "dfx_k_partition_ws_inl.hpp"
DFX_PASS1_UNIT(static_key_sum, StaticUnit<SigKeySum>)
