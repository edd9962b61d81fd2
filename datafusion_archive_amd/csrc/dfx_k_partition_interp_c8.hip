// dfx_k_partition_interp_c8.hip -- pass 1 of the partitioned GROUP BY, unit interp_c8 (dfx_pass1_units.hpp): InterpPolicy, <= 8 columns.
#include "dfx_k_partition_ws_inl.hpp"
DFX_PASS1_UNIT(interp_c8, Pass1Policies<InterpPolicy<8, 1>, InterpPolicy<8, 1>, InterpPolicy1<8, 1>>)
