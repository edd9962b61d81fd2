// dfx_k_partition_plan_c3_g0.hip -- pass 1 of the partitioned GROUP BY, unit plan_c3_g0 (dfx_pass1_units.hpp): the scan plan, column class 3, GENK = 0.
#include "dfx_k_partition_ws_inl.hpp"
DFX_PASS1_UNIT(plan_c3_g0, PlanUnit<3, 0>)
