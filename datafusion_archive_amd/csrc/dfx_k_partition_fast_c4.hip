// dfx_k_partition_fast_c4.hip -- pass 1 of the partitioned GROUP BY, unit fast_c4 (dfx_pass1_units.hpp): FastPolicy, <= 4 columns.
#include "dfx_k_partition_ws_inl.hpp"
DFX_PASS1_UNIT(fast_c4, Pass1Policies<FastPolicy<4, 2>, FastPolicy<4, 2>, FastPolicy1<4, 2>>)
