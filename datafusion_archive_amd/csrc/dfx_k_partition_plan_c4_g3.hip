// dfx_k_partition_plan_c4_g3.hip -- pass 1 of the partitioned GROUP BY, unit plan_c4_g3 (dfx_pass1_units.hpp): the scan plan, column class 4, GENK = 3.
#include "dfx_k_partition_ws_inl.hpp"
DFX_PASS1_UNIT(plan_c4_g3, PlanUnit<4, 3>)
