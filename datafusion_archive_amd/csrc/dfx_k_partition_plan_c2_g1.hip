// dfx_k_partition_plan_c2_g1.hip -- pass 1 of the partitioned GROUP BY, unit plan_c2_g1 (dfx_pass1_units.hpp): the scan plan, column class 2, GENK = 1.
#include "dfx_k_partition_ws_inl.hpp"
DFX_PASS1_UNIT(plan_c2_g1, PlanUnit<2, 1>)
