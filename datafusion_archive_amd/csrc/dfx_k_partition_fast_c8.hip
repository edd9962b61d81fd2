// dfx_k_partition_fast_c8.hip -- pass 1 of the partitioned GROUP BY, unit fast_c8 (dfx_pass1_units.hpp): FastPolicy, <= 8 columns.
#include "dfx_k_partition_ws_inl.hpp"
DFX_PASS1_UNIT(fast_c8, Pass1Policies<FastPolicy<8, 2>, FastPolicy<8, 1>, FastPolicy1<8, 1>>)
