// dfx_gather.cpp -- BatchGather and utf8_layout_from_lens (dfx_gather.hpp): the multi-batch gathers of dfx_k_sort.hip driven by a
// (batch << 32 | row) location per output row.  Per column the launches, copies and synchronisations are those ORDER BY and the
// resident table each had when they carried this code themselves.
#include "dfx_gather.hpp"

#include <algorithm>

#include "dfx_kernels.hpp"

namespace dfx {

Status utf8_layout_from_lens(const int32_t* lens, int64_t n, const char* what, std::shared_ptr<void>* offs, std::shared_ptr<void>* data,
                             int64_t* bytes) {
  hipStream_t s = ctx().stream;
  Status st;
  *offs = device_alloc(sizeof(int32_t) * (size_t)(n + 1), &st);
  if (!*offs) return st;
  auto tmp = device_alloc(sizeof(uint64_t) * (size_t)(n / 4096 + 4), &st);
  if (!tmp) return st;
  DFX_HIP(launch_scan_i32(lens, (int32_t*)offs->get(), n, (uint64_t*)tmp.get(), s));
  uint64_t total = 0;  // the scan's 64-bit sum: offs[n] is this value cut to int32
  DFX_HIP(hipMemcpyAsync(&total, (const uint64_t*)tmp.get() + scan_blocks(n), sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  DFX_HIP(hipStreamSynchronize(s));
  if (utf8_total_exceeds_offsets(total))
    return Status::Err(DFX_EXECUTION_ERROR, std::string(what) + " exceeds 2 GB (Arrow Utf8 offsets are 32-bit)");
  *bytes = (int64_t)total;
  *data = device_alloc((size_t)std::max<int64_t>(*bytes, 8), &st);
  return *data ? Status::OK() : st;
}

BatchGather::BatchGather(const std::vector<DeviceBatch>& batches, const char* too_many_rows)
    : batches_(batches), idx_(nullptr), too_many_rows_(too_many_rows) {
  for (const DeviceBatch& b : batches_) n_ += b.num_rows;
}

BatchGather::BatchGather(const std::vector<DeviceBatch>& batches, const uint32_t* idx, int64_t n) : batches_(batches), idx_(idx), n_(n) {}

Status BatchGather::locate() {
  if (loc_) return Status::OK();
  if (!idx_ && n_ >= (1ll << 32)) return Status::Err(DFX_NOT_IMPLEMENTED, too_many_rows_);
  hipStream_t s = ctx().stream;
  Status st;
  std::vector<uint64_t> starts(batches_.size() + 1, 0);
  for (size_t b = 0; b < batches_.size(); ++b) starts[b + 1] = starts[b] + (uint64_t)batches_[b].num_rows;
  auto dstarts = device_alloc(sizeof(uint64_t) * starts.size(), &st);
  if (!dstarts) return st;
  DFX_HIP(hipMemcpyAsync(dstarts.get(), starts.data(), sizeof(uint64_t) * starts.size(), hipMemcpyHostToDevice, s));
  const size_t slots = (size_t)std::max<int64_t>(n_, 1);
  std::shared_ptr<void> iota;
  if (!idx_) {
    iota = device_alloc(sizeof(uint32_t) * slots, &st);
    if (!iota) return st;
    DFX_HIP(launch_sort_iota((uint32_t*)iota.get(), n_, s));
  }
  auto loc = device_alloc(sizeof(uint64_t) * slots, &st);
  if (!loc) return st;
  DFX_HIP(launch_sort_locate(idx_ ? idx_ : (const uint32_t*)iota.get(), n_, (const uint64_t*)dstarts.get(), (int)batches_.size(),
                             (uint64_t*)loc.get(), s));
  DFX_HIP(hipStreamSynchronize(s));  // `starts` is a stack vector
  loc_ = loc;
  return Status::OK();
}

Status BatchGather::gather_bitmap(int c, const std::shared_ptr<void>& bases, std::shared_ptr<void>* out, int64_t* zeros) {
  hipStream_t s = ctx().stream;
  Status st;
  std::vector<int64_t> bit_offsets;
  for (const DeviceBatch& b : batches_) bit_offsets.push_back(b.columns[(size_t)c].bit_offset);
  std::shared_ptr<void> dbo;
  DFX_RETURN_IF_ERROR(upload_vec(bit_offsets, &dbo));
  *out = device_alloc(((size_t)(n_ + 63) / 64 + 1) * 8, &st);  // (one word of slack behind the bitmap)
  if (!*out) return st;
  std::shared_ptr<void> count;
  if (zeros) {
    count = device_alloc(sizeof(uint64_t), &st);
    if (!count) return st;
    DFX_HIP(hipMemsetAsync(count.get(), 0, sizeof(uint64_t), s));
  }
  DFX_HIP(launch_gather_bits((const uint8_t* const*)bases.get(), (const int64_t*)dbo.get(), (const uint64_t*)loc_.get(), n_,
                             (uint64_t*)out->get(), (uint64_t*)count.get(), s));
  if (zeros) {
    uint64_t nz = 0;
    DFX_HIP(hipMemcpyAsync(&nz, count.get(), sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    DFX_HIP(hipStreamSynchronize(s));
    *zeros = (int64_t)nz;
  }
  return Status::OK();
}

Status BatchGather::validity(int c, std::shared_ptr<void>* bitmap, int64_t* zeros) {
  bitmap->reset();
  *zeros = 0;
  auto has_nulls = [](const DeviceColumn& col) { return col.validity && col.null_count != 0; };
  bool any_nulls = false;
  for (const DeviceBatch& b : batches_) any_nulls = any_nulls || has_nulls(b.columns[(size_t)c]);
  if (!any_nulls) return Status::OK();
  DFX_RETURN_IF_ERROR(locate());
  std::shared_ptr<void> bases;  // (a batch without nulls: a null pointer, every bit reads as 1)
  DFX_RETURN_IF_ERROR(pointer_table(c, [&](const DeviceColumn& col) -> const void* { return has_nulls(col) ? col.validity : nullptr; }, &bases));
  return gather_bitmap(c, bases, bitmap, zeros);
}

Status BatchGather::utf8(int c, const char* what, DeviceColumn* col) {
  DFX_RETURN_IF_ERROR(locate());
  hipStream_t s = ctx().stream;
  Status st;
  std::shared_ptr<void> doffs, ddata;
  DFX_RETURN_IF_ERROR(pointer_table(c, [](const DeviceColumn& ic) -> const void* { return ic.offsets; }, &doffs));
  DFX_RETURN_IF_ERROR(pointer_table(c, [](const DeviceColumn& ic) -> const void* { return ic.data; }, &ddata));
  auto lens = device_alloc(sizeof(int32_t) * (size_t)(n_ + 1), &st);
  if (!lens) return st;
  DFX_HIP(launch_gather_utf8_lens((const int32_t* const*)doffs.get(), (const uint64_t*)loc_.get(), n_, (int32_t*)lens.get(), s));
  std::shared_ptr<void> offs, data;
  DFX_RETURN_IF_ERROR(utf8_layout_from_lens((const int32_t*)lens.get(), n_, what, &offs, &data, &col->data_bytes));
  DFX_HIP(launch_gather_utf8_copy((const int32_t* const*)doffs.get(), (const uint8_t* const*)ddata.get(), (const uint64_t*)loc_.get(), n_,
                                  (const int32_t*)offs.get(), (uint8_t*)data.get(), s));
  col->offsets = (const int32_t*)offs.get();
  col->data = (const uint8_t*)data.get();
  col->owners.push_back(offs);
  col->owners.push_back(data);
  return Status::OK();
}

Status BatchGather::bits(int c, DeviceColumn* col) {
  DFX_RETURN_IF_ERROR(locate());
  std::shared_ptr<void> bases, vals;
  DFX_RETURN_IF_ERROR(pointer_table(c, [](const DeviceColumn& ic) { return ic.values; }, &bases));
  DFX_RETURN_IF_ERROR(gather_bitmap(c, bases, &vals, nullptr));
  col->values = vals.get();
  col->owners.push_back(vals);
  return Status::OK();
}

Status BatchGather::fixed(int c, DeviceColumn* col) {
  hipStream_t s = ctx().stream;
  Status st;
  const int w = dtype_width(col->dtype);
  auto vals = device_alloc((size_t)std::max<int64_t>(n_, 1) * (size_t)w, &st);
  if (!vals) return st;
  if (idx_) {
    DFX_RETURN_IF_ERROR(locate());
    std::shared_ptr<void> bases;
    DFX_RETURN_IF_ERROR(pointer_table(c, [](const DeviceColumn& ic) { return ic.values; }, &bases));
    DFX_HIP(launch_gather_fixed((const void* const*)bases.get(), (const uint64_t*)loc_.get(), n_, w, vals.get(), s));
  } else {  // the batches one behind the other: no location array, no pointer table
    int64_t pos = 0;
    for (const DeviceBatch& b : batches_) {
      const DeviceColumn& ic = b.columns[(size_t)c];
      if (ic.length) DFX_HIP(hipMemcpyAsync((uint8_t*)vals.get() + (size_t)pos * w, ic.values, (size_t)ic.length * w, hipMemcpyDeviceToDevice, s));
      pos += ic.length;
    }
  }
  col->values = vals.get();
  col->owners.push_back(vals);
  return Status::OK();
}

}  // namespace dfx
