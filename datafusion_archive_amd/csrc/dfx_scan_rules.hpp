// dfx_scan_rules.hpp -- what the hosts of an exclusive scan (launch_scan_u32 / launch_scan_i32, dfx_k_core.hip) must agree on with its
// launcher, and the rule a Utf8 column's byte total is judged by.  Free of HIP (tests/native/utf8_total_rule_check.cpp).
#pragma once
#include <stdint.h>

namespace dfx {

constexpr int kScanChunk = 4096;  // elements per block of the scan kernels (256 threads x 16)

// Blocks a scan of n elements launches.  Its `tmp` holds one 64-bit sum per block and, in slot scan_blocks(n), the 64-bit grand
// total (k_scan_sums) -- the untruncated value of what launch_scan_i32 stores as int32 in out[n].  Callers allocate
// n / 4096 + 4 words of tmp, which always holds that slot.
inline int64_t scan_blocks(int64_t n) { return n > 0 ? (n + kScanChunk - 1) / kScanChunk : 1; }

// Arrow Utf8 offsets are int32: a column's bytes must sum to at most 2^31 - 1.  Asked of a 64-BIT sum: an int32 read-back of the
// scan's last offset shows a sum in [2^31, 2^32) as negative and one of 2^32 or more as a small positive number again.
inline bool utf8_total_exceeds_offsets(uint64_t total_bytes) { return total_bytes > (uint64_t)INT32_MAX; }

}  // namespace dfx
