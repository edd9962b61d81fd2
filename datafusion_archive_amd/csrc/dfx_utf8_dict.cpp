// dfx_utf8_dict.cpp -- Utf8Dict (dfx_utf8_dict.hpp): the only host code that binds buffers to the kernels of dfx_k_dict.hip.
#include "dfx_utf8_dict.hpp"

#include <algorithm>

namespace dfx {

Status Utf8Dict::alloc(int slots_log2, uint64_t pool_cap, bool keep) {
  hipStream_t s = ctx().stream;
  const uint64_t slots = 1ull << slots_log2, id_cap = slots / 2;
  Status st;
  auto dstate = device_alloc(sizeof(uint32_t) * slots, &st);
  if (!dstate) return st;
  auto h = device_alloc(sizeof(uint64_t) * slots, &st);
  if (!h) return st;
  auto sd = device_alloc(sizeof(uint64_t) * slots, &st);
  if (!sd) return st;
  auto so = device_alloc(sizeof(uint64_t) * id_cap, &st);
  if (!so) return st;
  auto sl = device_alloc(sizeof(uint32_t) * id_cap, &st);
  if (!sl) return st;
  auto pl = device_alloc(std::max<uint64_t>(pool_cap, 64), &st);
  if (!pl) return st;
  auto cur = device_alloc(sizeof(uint64_t) * DICT_WORDS, &st);
  if (!cur) return st;
  DFX_HIP(hipMemsetAsync(dstate.get(), 0, sizeof(uint32_t) * slots, s));
  if (keep && allocated) {
    if (pool_used) DFX_HIP(hipMemcpyAsync(pl.get(), pool.get(), pool_used, hipMemcpyDeviceToDevice, s));
    if (ids_used) {
      DFX_HIP(hipMemcpyAsync(so.get(), str_off.get(), sizeof(uint64_t) * ids_used, hipMemcpyDeviceToDevice, s));
      DFX_HIP(hipMemcpyAsync(sl.get(), str_len.get(), sizeof(uint32_t) * ids_used, hipMemcpyDeviceToDevice, s));
    }
  } else {
    ids_used = pool_used = 0;
  }
  const uint64_t hc[DICT_WORDS] = {pool_used, ids_used, 0, 0};
  DFX_HIP(hipMemcpyAsync(cur.get(), hc, sizeof(hc), hipMemcpyHostToDevice, s));
  DFX_HIP(hipStreamSynchronize(s));  // hc is a stack buffer; the old arrays are released below
  state = dstate; hash = h; sid = sd; str_off = so; str_len = sl; pool = pl; cursors = cur;
  D.state = (uint32_t*)dstate.get();
  D.hash = (uint64_t*)h.get();
  D.sid = (uint64_t*)sd.get();
  D.str_off = (uint64_t*)so.get();
  D.str_len = (uint32_t*)sl.get();
  D.pool = (uint8_t*)pl.get();
  D.cursors = (uint64_t*)cur.get();
  D.mask = slots - 1;
  D.shift = 64 - slots_log2;
  D.id_cap = id_cap;
  D.pool_cap = std::max<uint64_t>(pool_cap, 64);
  allocated = true;
  if (ids_used) DFX_HIP(launch_dict_rebuild(D, ids_used, s));
  return Status::OK();
}

Status Utf8Dict::encode(const DeviceColumn& src, int64_t n, int capacity_log2, DeviceColumn* ids_col) {
  hipStream_t s = ctx().stream;
  Status st;
  auto ids = device_alloc(sizeof(uint64_t) * (size_t)std::max<int64_t>(n, 1), &st);
  if (!ids) return st;
  if (!allocated) {
    int lg = capacity_log2 > 0 ? capacity_log2 : 16;
    lg = std::max(4, std::min(lg, 30));
    DFX_RETURN_IF_ERROR(alloc(lg, std::max<uint64_t>((uint64_t)src.data_bytes * 2, 1u << 16), false));
  }
  for (int attempt = 0; n > 0; ++attempt) {
    if (attempt > 16) return Status::Err(DFX_INTERNAL_ERROR, strfmt("%s does not converge", noun));
    DFX_HIP(launch_dict_encode(src.offsets, src.data, n, D, ids_used, (uint64_t*)ids.get(), s));
    uint64_t hc[DICT_WORDS];
    DFX_HIP(hipMemcpyAsync(hc, D.cursors, sizeof(hc), hipMemcpyDeviceToHost, s));
    DFX_HIP(hipStreamSynchronize(s));
    if (hc[DICT_OVERFLOW] == 2) return Status::Err(DFX_INTERNAL_ERROR, strfmt("%s: slot claim timed out", noun));
    if (hc[DICT_OVERFLOW] == 0) {
      ids_used = hc[DICT_IDS];
      pool_used = hc[DICT_POOL];
      break;
    }
    // overflow: forget this attempt (its ids were not used yet), grow x4 (slots / ids) and to fit the batch (pool)
    int lg = 64 - D.shift;
    const uint64_t want_ids = std::max<uint64_t>(hc[DICT_IDS], ids_used + 1);
    while ((1ull << lg) / 2 < want_ids * 2 && lg < 31) ++lg;
    lg = std::min(31, std::max(lg, 64 - D.shift + 2));
    const uint64_t want_pool = std::max<uint64_t>(hc[DICT_POOL], pool_used + (uint64_t)src.data_bytes) * 2;
    DFX_RETURN_IF_ERROR(alloc(lg, std::max<uint64_t>(want_pool, D.pool_cap), true));
  }
  ids_col->dtype = DFX_UINT64;
  ids_col->length = n;
  ids_col->null_count = 0;
  ids_col->values = ids.get();
  ids_col->validity = nullptr;
  ids_col->bit_offset = 0;
  ids_col->offsets = nullptr;
  ids_col->data = nullptr;
  ids_col->owners.clear();
  ids_col->owners.push_back(ids);
  return Status::OK();
}

// A null row carries the id of some string of length 0 (the empty string's): nothing is gathered for it.
Status Utf8Dict::to_utf8(const uint64_t* ids, int64_t g, const std::shared_ptr<void>& validity, int64_t null_count, const char* what,
                         DeviceColumn* out) const {
  hipStream_t s = ctx().stream;
  Status st;
  auto lens = device_alloc(sizeof(uint32_t) * (size_t)std::max<int64_t>(g, 1), &st);
  if (!lens) return st;
  auto starts = device_alloc(sizeof(uint64_t) * (size_t)(g + 1), &st);
  if (!starts) return st;
  auto tmp = device_alloc(sizeof(uint64_t) * (size_t)(g / 4096 + 4), &st);
  if (!tmp) return st;
  auto offs = device_alloc(sizeof(int32_t) * (size_t)(g + 1), &st);
  if (!offs) return st;
  uint64_t total = 0;
  if (g > 0) {
    DFX_HIP(launch_dict_lengths(ids, g, D, (uint32_t*)lens.get(), s));
    DFX_HIP(launch_scan_u32((const uint32_t*)lens.get(), (uint64_t*)starts.get(), g, (uint64_t*)tmp.get(), s));
    DFX_HIP(hipMemcpyAsync(&total, (uint64_t*)starts.get() + g, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    DFX_HIP(hipStreamSynchronize(s));
  } else {
    DFX_HIP(hipMemsetAsync(starts.get(), 0, sizeof(uint64_t), s));
  }
  if (total > 0x7FFFFFFFull) return Status::Err(DFX_EXECUTION_ERROR, strfmt("%s exceed 2 GB (Arrow Utf8 offsets are 32-bit)", what));
  auto data = device_alloc((size_t)std::max<uint64_t>(total, 8), &st);
  if (!data) return st;
  DFX_HIP(launch_dict_gather(ids, g, D, (const uint64_t*)starts.get(), (int32_t*)offs.get(), (uint8_t*)data.get(), s));
  out->dtype = DFX_UTF8;
  out->length = g;
  out->null_count = null_count;
  out->validity = null_count ? (const uint8_t*)validity.get() : nullptr;
  out->bit_offset = 0;
  out->values = nullptr;
  out->offsets = (const int32_t*)offs.get();
  out->data = (const uint8_t*)data.get();
  out->data_bytes = (int64_t)total;
  out->owners.clear();
  out->owners.push_back(offs);
  out->owners.push_back(data);
  if (null_count) out->owners.push_back(validity);
  return Status::OK();
}

Status Utf8Dict::download(std::vector<uint32_t>* lens, std::vector<uint8_t>* strings) const {
  lens->assign((size_t)ids_used, 0);
  strings->clear();
  if (!allocated || ids_used == 0) return Status::OK();
  std::vector<uint64_t> offs((size_t)ids_used);
  std::vector<uint8_t> raw((size_t)pool_used);
  DFX_HIP(hipStreamSynchronize(ctx().stream));
  DFX_HIP(hipMemcpy(lens->data(), D.str_len, sizeof(uint32_t) * lens->size(), hipMemcpyDeviceToHost));
  DFX_HIP(hipMemcpy(offs.data(), D.str_off, sizeof(uint64_t) * offs.size(), hipMemcpyDeviceToHost));
  if (!raw.empty()) DFX_HIP(hipMemcpy(raw.data(), D.pool, raw.size(), hipMemcpyDeviceToHost));
  size_t total = 0;
  for (uint32_t l : *lens) total += l;
  strings->reserve(total);
  for (size_t i = 0; i < lens->size(); ++i) {  // the pool is filled by atomics: put the strings in id order
    if (offs[i] + (*lens)[i] > raw.size()) return Status::Err(DFX_INTERNAL_ERROR, strfmt("%s: string outside the pool", noun));
    strings->insert(strings->end(), raw.begin() + (ptrdiff_t)offs[i], raw.begin() + (ptrdiff_t)(offs[i] + (*lens)[i]));
  }
  return Status::OK();
}

Status Utf8Dict::install(const std::vector<uint32_t>& lens, const std::vector<uint8_t>& strings) {
  const uint64_t g = lens.size();
  int lg = 4;
  while ((1ull << lg) / 2 < std::max<uint64_t>(g, 1) && lg < 31) ++lg;
  ids_used = pool_used = 0;
  DFX_RETURN_IF_ERROR(alloc(lg, std::max<uint64_t>(strings.size(), 64), false));
  std::vector<uint64_t> offs((size_t)g);
  uint64_t at = 0;
  for (size_t i = 0; i < (size_t)g; ++i) {
    offs[i] = at;
    at += lens[i];
  }
  if (g) {
    DFX_HIP(hipMemcpy(D.str_len, lens.data(), sizeof(uint32_t) * (size_t)g, hipMemcpyHostToDevice));
    DFX_HIP(hipMemcpy(D.str_off, offs.data(), sizeof(uint64_t) * (size_t)g, hipMemcpyHostToDevice));
    if (!strings.empty()) DFX_HIP(hipMemcpy(D.pool, strings.data(), strings.size(), hipMemcpyHostToDevice));
  }
  ids_used = g;
  pool_used = strings.size();
  const uint64_t hc[DICT_WORDS] = {pool_used, ids_used, 0, 0};
  DFX_HIP(hipMemcpy(D.cursors, hc, sizeof(hc), hipMemcpyHostToDevice));
  return Status::OK();
}

}  // namespace dfx
