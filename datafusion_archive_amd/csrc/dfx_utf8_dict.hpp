// dfx_utf8_dict.hpp -- Utf8Dict: the host side of dfx_k_dict.hip.  A Utf8 column's strings become stable UInt64 ids on the device
// (the GROUP BY's Utf8 keys, the distinct sets' Utf8 keys and arguments); ids become an Arrow Utf8 column again at emit.
#pragma once
#include <string.h>

#include <memory>
#include <vector>

#include "dfx_host.hpp"
#include "dfx_kernels.hpp"

namespace dfx {

struct Utf8Dict {
  explicit Utf8Dict(const char* noun_) : noun(noun_) { memset(&D, 0, sizeof(D)); }
  const char* noun;  // what the error messages call this dictionary
  DevDict D;
  std::shared_ptr<void> state, hash, sid, str_off, str_len, pool, cursors;
  uint64_t ids_used = 0, pool_used = 0;  // as of the last completed batch
  bool allocated = false;

  // (re)allocate with 2^slots_log2 slots (ids capacity = half of that) and `pool_cap` pool bytes; keep == true carries the
  // strings of completed batches over and rebuilds the slot table from them
  Status alloc(int slots_log2, uint64_t pool_cap, bool keep);
  // ids of one batch's strings: a bare UInt64 column (no validity).  Grows the dictionary (ids stay stable) and re-encodes when it
  // overflows; capacity_log2: the first allocation's slots (0: 2^16)
  Status encode(const DeviceColumn& src, int64_t n, int capacity_log2, DeviceColumn* ids_col);
  // g ids -> an Arrow Utf8 column on the device (lengths, scan, gather), nullable when null_count != 0; `what` names the
  // strings in the error of a column past 2 GB
  Status to_utf8(const uint64_t* ids, int64_t g, const std::shared_ptr<void>& validity, int64_t null_count, const char* what, DeviceColumn* out) const;
  // the strings in id order (lengths + bytes back to back), to the host and from it; install replaces the dictionary
  Status download(std::vector<uint32_t>* lens, std::vector<uint8_t>* strings) const;
  Status install(const std::vector<uint32_t>& lens, const std::vector<uint8_t>& strings);
};

}  // namespace dfx
