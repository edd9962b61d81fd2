// dfx_k_partition_interp_c4.hip -- pass 1 of the partitioned GROUP BY, unit interp_c4 (dfx_pass1_units.hpp): InterpPolicy, <= 4 columns.
#include "dfx_k_partition_ws_inl.hpp"
DFX_PASS1_UNIT(interp_c4, Pass1Policies<InterpPolicy<4, 2>, InterpPolicy<4, 1>, InterpPolicy1<4, 1>>)
