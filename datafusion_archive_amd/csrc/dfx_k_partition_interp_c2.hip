// dfx_k_partition_interp_c2.hip -- pass 1 of the partitioned GROUP BY, unit interp_c2 (dfx_pass1_units.hpp): InterpPolicy, <= 2 columns.
#include "dfx_k_partition_ws_inl.hpp"
DFX_PASS1_UNIT(interp_c2, Pass1Policies<InterpPolicy<2, 2>, InterpPolicy<2, 1>, InterpPolicy1<2, 1>>)
