// dfx_k_partition_v29.hip -- pass 1 of the partitioned GROUP BY, the PAIR flavour (two aggregates of different operands) over a 4-byte key:
// PlanPolicy with slot look-ups, 3 columns, GENK = 4 (the key in slot 0 is the only 4-byte column: the Int32 shadow of a resident Int64
// key column, read with one 4-byte load per lane).  Trips as in the 8-byte unit of the same width.
#include "dfx_k_partition_ws_inl.hpp"
namespace dfx {
DFX_PARTITION_VARIANT_WS_PAIR_ONLY(29, DFX_ARG(PlanPolicyN<3, 3, 4>))
}  // namespace dfx
