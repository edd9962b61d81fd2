// dfx_gather.hpp -- rows of several device batches gathered into one column, addressed once: what ORDER BY does with its sorted
// permutation (dfx_sort.cpp) and a resident table with the identity over the batches it concatenates (dfx_table.cpp).  Also the one
// place where the lengths of a Utf8 column become its offsets and its data buffer (utf8_layout_from_lens).
#pragma once
#include "dfx_host.hpp"

namespace dfx {

// lens (device, n entries) -> offs (n + 1 int32 offsets), data (max(bytes, 8) bytes, not yet filled) and bytes, the column's total.
// The total is the scan's own 64-bit sum, so a column beyond Arrow's 32-bit offsets is refused however far beyond
// (utf8_total_exceeds_offsets, dfx_scan_rules.hpp): DFX_EXECUTION_ERROR "<what> exceeds 2 GB (Arrow Utf8 offsets are 32-bit)".
// One scan, one 8-byte read-back, one synchronisation.
Status utf8_layout_from_lens(const int32_t* lens, int64_t n, const char* what, std::shared_ptr<void>* offs, std::shared_ptr<void>* data,
                             int64_t* bytes);

class BatchGather {
 public:
  // the identity: every row of every batch, in order.  too_many_rows: the NOT_IMPLEMENTED text for 2^32 or more rows, given when
  // a column first needs the location array (fixed-width values of the identity never do)
  BatchGather(const std::vector<DeviceBatch>& batches, const char* too_many_rows);
  // the n rows idx[0..n) (device) of the batches' concatenation; the caller has refused 2^32 or more rows
  BatchGather(const std::vector<DeviceBatch>& batches, const uint32_t* idx, int64_t n);

  // column c's validity bits and how many of them are zero; *bitmap stays null (nothing is launched) when no batch has
  // `validity && null_count != 0`.  Whether a bitmap without zeros is attached is the caller's rule.
  Status validity(int c, std::shared_ptr<void>* bitmap, int64_t* zeros);
  // the values of column c into *col (values / offsets / data / data_bytes, owners); dtype, length and validity are the caller's
  Status utf8(int c, const char* what, DeviceColumn* col);
  Status bits(int c, DeviceColumn* col);   // Boolean values
  Status fixed(int c, DeviceColumn* col);  // identity: one D2D copy per batch; permutation: launch_gather_fixed
  Status values(int c, const char* utf8_what, DeviceColumn* col) {  // ... whichever of the three col->dtype asks for
    return col->dtype == DFX_UTF8 ? utf8(c, utf8_what, col) : col->dtype == DFX_BOOLEAN ? bits(c, col) : fixed(c, col);
  }

 private:
  Status locate();  // builds loc_ on first need
  // one pointer per batch, taken from its column c, as a device table
  template <typename F>
  Status pointer_table(int c, F&& of, std::shared_ptr<void>* dev) const {
    std::vector<const void*> v;
    for (const DeviceBatch& b : batches_) v.push_back(of(b.columns[(size_t)c]));
    return upload_vec(v, dev);
  }
  // bit (base[batch], bit_offset[batch] + row) of every output row; *zeros (may be null): how many are 0
  Status gather_bitmap(int c, const std::shared_ptr<void>& bases, std::shared_ptr<void>* out, int64_t* zeros);

  const std::vector<DeviceBatch>& batches_;
  const uint32_t* idx_;  // null: the identity
  int64_t n_ = 0;
  const char* too_many_rows_ = nullptr;
  std::shared_ptr<void> loc_;  // (batch << 32 | row) of every output row
};

}  // namespace dfx
