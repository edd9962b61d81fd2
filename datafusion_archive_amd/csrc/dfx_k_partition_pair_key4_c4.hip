// dfx_k_partition_pair_key4_c4.hip -- pass 1 of the partitioned GROUP BY, unit pair_key4_c4 (dfx_pass1_units.hpp): the pair scan over a 4-byte key, 4 columns.
#include "dfx_k_partition_ws_inl.hpp"
DFX_PASS1_UNIT(pair_key4_c4, PairKey4Unit<4>)
