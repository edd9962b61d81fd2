// dfx_k_partition_fast_c2.hip -- pass 1 of the partitioned GROUP BY, unit fast_c2 (dfx_pass1_units.hpp): FastPolicy, <= 2 columns.
#include "dfx_k_partition_ws_inl.hpp"
#ifndef DFX_V2_UN
#define DFX_V2_UN 4  // row groups per trip of the one-value flavour (A/B: tools/build_variant.py)
#endif
DFX_PASS1_UNIT(fast_c2, Pass1Policies<FastPolicy<2, 4>, FastPolicy<2, 2>, FastPolicy1<2, DFX_V2_UN>>)
