// dfx_distinct_emit.cpp -- the distinct sets at emit: every set's tuples counted (COUNT_DISTINCT) or folded (Utf8 MIN / MAX) per key
// prefix into an emit table, each group the inner aggregate emits looked up there, and the columns spliced into the result (next).
#include "dfx_distinct_impl.hpp"

namespace dfx {
namespace {

// an EmitTable for a set of `kw`-word tuples of which `occupied` are taken, zeroed on the library's stream
Status alloc_emit_table(int kw, uint64_t occupied, int planes, EmitTable* E) {
  hipStream_t s = ctx().stream;
  Status st;
  DevTable& T = E->T;
  memset(&T, 0, sizeof(T));
  int lg = 10;
  while ((1ull << lg) < occupied * 2 + 2 && lg < 34) ++lg;
  const uint64_t cap = 1ull << lg;
  T.kw = kw;
  T.na = planes;
  T.stride = kw == 1 ? 1 : cap + 64;
  if (kw > 1) {
    T.mask = cap - 1;
    T.shift = 64 - lg;
    T.load_limit = cap;
    T.max_probe = (int)std::min<uint64_t>(cap, 1u << 30);
    T.block_mask = (uint32_t)(cap - 1);
    auto keys = device_alloc(sizeof(uint64_t) * T.stride * (size_t)kw, &st);
    if (!keys) return st;
    auto state = device_alloc(sizeof(uint32_t) * T.stride, &st);
    if (!state) return st;
    T.keys = (uint64_t*)keys.get();
    T.state = (uint32_t*)state.get();
    E->owners.push_back(keys);
    E->owners.push_back(state);
    DFX_HIP(hipMemsetAsync(T.state, 0, sizeof(uint32_t) * T.stride, s));
  }
  auto accs = device_alloc(sizeof(uint64_t) * T.stride * (size_t)planes, &st);
  if (!accs) return st;
  auto ctrl = device_alloc(sizeof(uint32_t) * CTRL_WORDS, &st);
  if (!ctrl) return st;
  T.accs = (uint64_t*)accs.get();
  T.ctrl = (uint32_t*)ctrl.get();
  E->owners.push_back(accs);
  E->owners.push_back(ctrl);
  for (int a = 0; a < planes; ++a) {
    T.acc_kind[a] = ACC_ADD_U64;
    T.val_xform[a] = VT_RAW;
  }
  DFX_HIP(hipMemsetAsync(T.accs, 0, sizeof(uint64_t) * T.stride * (size_t)planes, s));
  DFX_HIP(hipMemsetAsync(T.ctrl, 0, sizeof(uint32_t) * CTRL_WORDS, s));
  return Status::OK();
}

// g rows of NULL: what a set that no tuple reached gives every group
Status utf8_null_column(int64_t g, DeviceColumn* out) {
  hipStream_t s = ctx().stream;
  Status st;
  auto offs = device_alloc(sizeof(int32_t) * (size_t)(g + 1), &st);
  if (!offs) return st;
  const size_t vbytes = sizeof(uint64_t) * (size_t)std::max<int64_t>((g + 63) / 64, 1);
  auto validity = device_alloc(vbytes, &st);
  if (!validity) return st;
  auto data = device_alloc(8, &st);
  if (!data) return st;
  DFX_HIP(hipMemsetAsync(offs.get(), 0, sizeof(int32_t) * (size_t)(g + 1), s));
  DFX_HIP(hipMemsetAsync(validity.get(), 0, vbytes, s));
  out->dtype = DFX_UTF8;
  out->length = g;
  out->null_count = g;
  out->validity = g ? (const uint8_t*)validity.get() : nullptr;
  out->bit_offset = 0;
  out->values = nullptr;
  out->offsets = (const int32_t*)offs.get();
  out->data = (const uint8_t*)data.get();
  out->data_bytes = 0;
  out->owners = {offs, data, validity};
  return Status::OK();
}

// g zeroes: the counts of a set that no batch reached
Status zero_count_column(int64_t g, DeviceColumn* col) {
  Status st;
  const size_t bytes = sizeof(uint64_t) * (size_t)std::max<int64_t>(g, 1);
  auto vals = device_alloc(bytes, &st);
  if (!vals) return st;
  DFX_HIP(hipMemsetAsync(vals.get(), 0, bytes, ctx().stream));
  col->dtype = DFX_UINT64;
  col->length = g;
  col->values = vals.get();
  col->owners.push_back(vals);
  return Status::OK();
}

// the ungrouped result's one row: the set's tuple count, NULL (over a 0) where COUNT(x) of the same rows is
Status ungrouped_count_row(uint64_t total, bool valid, DeviceColumn* col) {
  const uint64_t v = valid ? total : 0;
  col->dtype = DFX_UINT64;
  col->length = 1;
  std::shared_ptr<void> dv;
  DFX_RETURN_IF_ERROR(upload_small(&v, 8, &dv));
  col->values = dv.get();
  col->owners.push_back(dv);
  if (!valid) {
    const uint8_t vb[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::shared_ptr<void> dn;
    DFX_RETURN_IF_ERROR(upload_small(vb, 8, &dn));
    col->validity = (const uint8_t*)dn.get();
    col->null_count = 1;
    col->owners.push_back(dn);
  }
  return Status::OK();
}

}  // namespace

// the emitted keys as the sets' programs saw them (Utf8: through this side's dictionary); *ids keeps the id columns alive
Status DistinctAggregateRelation::emitted_keys(const DeviceBatch& inner_out, DevDistinctKeys* K, std::vector<DeviceColumn>* ids) {
  memset(K, 0, sizeof(*K));
  ids->assign(dicts_.size(), DeviceColumn());
  for (int k = 0; k < kw_out_; ++k) {
    const DeviceColumn& kc = inner_out.columns[(size_t)k];
    if (key_dict_[(size_t)k] >= 0) {
      DistinctDict& d = dicts_[(size_t)key_dict_[(size_t)k]];
      DFX_RETURN_IF_ERROR(encode_with_validity(d, kc, inner_out.num_rows, &(*ids)[(size_t)key_dict_[(size_t)k]]));
      K->values[k] = (*ids)[(size_t)key_dict_[(size_t)k]].values;
      K->dtype[k] = T_U64;
    } else {
      K->values[k] = kc.values;
      K->dtype[k] = (uint8_t)kc.dtype;
    }
  }
  return Status::OK();
}

// MIN / MAX of the set's Utf8 argument per emitted group (ungrouped: of the one row): fold the set into the extrema table, look
// every group up, ids -> strings.  A group without a non-null argument has no entry, or an empty word: NULL.
Status DistinctAggregateRelation::emit_extrema(DistinctSet& S, const DeviceBatch& inner_out, DeviceColumn* min_col, DeviceColumn* max_col) {
  hipStream_t s = ctx().stream;
  Status st;
  const int64_t g = inner_out.num_rows;
  DeviceColumn* cols[2] = {S.want_min ? min_col : nullptr, S.want_max ? max_col : nullptr};
  if (!S.T.keys || g == 0 || S.arg_dict < 0) {  // no batch reached the set (or there is no group to report)
    for (DeviceColumn* c : cols)
      if (c) DFX_RETURN_IF_ERROR(utf8_null_column(g, c));
    return Status::OK();
  }
  Utf8Dict& d = dicts_[(size_t)S.arg_dict].dict;
  // The id a NULL is gathered through: the empty string's, put into the dictionary if no row held it (the sets are not touched).
  // Every encode of this emit comes before the fold: growth replaces the dictionary's arrays (ids stay).
  uint64_t null_id = 0;
  {
    auto zero = device_alloc(16, &st);
    if (!zero) return st;
    DFX_HIP(hipMemsetAsync(zero.get(), 0, 16, s));
    DeviceColumn empty, id_col;
    empty.dtype = DFX_UTF8;
    empty.length = 1;
    empty.offsets = (const int32_t*)zero.get();
    empty.data = (const uint8_t*)zero.get() + 8;
    empty.owners.push_back(zero);
    DFX_RETURN_IF_ERROR(d.encode(empty, 1, opt().dict_capacity_log2, &id_col));
    DFX_HIP(hipMemcpyAsync(&null_id, id_col.values, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    DFX_HIP(hipStreamSynchronize(s));
    if (null_id >= d.ids_used) return Status::Err(DFX_INTERNAL_ERROR, "MIN/MAX of Utf8: the dictionary did not take the empty string");
  }
  DevDistinctKeys K;
  std::vector<DeviceColumn> key_ids;
  DFX_RETURN_IF_ERROR(emitted_keys(inner_out, &K, &key_ids));
  uint32_t hc[CTRL_WORDS];
  DFX_RETURN_IF_ERROR(read_ctrl(S, hc));
  if (!S.want_count) counters().distinct_inserted += (long long)hc[CTRL_OCCUPIED];  // (emit_counts adds it for a set it reads too)
  EmitTable E;
  DFX_RETURN_IF_ERROR(alloc_emit_table(S.kw, hc[CTRL_OCCUPIED], 2, &E));
  DFX_HIP(launch_utf8_extrema_fold(S.T, E.T, d.D, d.ids_used, (S.want_min ? 1u : 0u) | (S.want_max ? 2u : 0u), s));
  for (int plane = 0; plane < 2; ++plane) {
    if (!cols[plane]) continue;
    auto ids = device_alloc(sizeof(uint64_t) * (size_t)g, &st);
    if (!ids) return st;
    auto validity = device_alloc(sizeof(uint64_t) * (size_t)((g + 63) / 64), &st);
    if (!validity) return st;
    auto nulls = device_alloc(sizeof(uint64_t), &st);
    if (!nulls) return st;
    DFX_HIP(hipMemsetAsync(nulls.get(), 0, sizeof(uint64_t), s));
    DFX_HIP(launch_utf8_extrema_lookup(E.T, K, kw_out_, g, plane, null_id, (uint64_t*)ids.get(), (uint64_t*)validity.get(), (uint64_t*)nulls.get(), s));
    uint64_t null_count = 0;
    uint32_t cc[CTRL_WORDS];
    DFX_HIP(hipMemcpyAsync(&null_count, nulls.get(), sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    DFX_HIP(hipMemcpyAsync(cc, E.T.ctrl, sizeof(cc), hipMemcpyDeviceToHost, s));
    DFX_HIP(hipStreamSynchronize(s));
    if (cc[CTRL_ERROR] & 0x200u) return Status::Err(DFX_INTERNAL_ERROR, "MIN/MAX of Utf8: a tuple's argument is no id of the dictionary");
    if (cc[CTRL_ERROR]) return Status::Err(DFX_INTERNAL_ERROR, "MIN/MAX of Utf8: extrema table overflow");
    DFX_RETURN_IF_ERROR(d.to_utf8((const uint64_t*)ids.get(), g, validity, (int64_t)null_count, "Utf8 MIN/MAX results", cols[plane]));
  }
  return Status::OK();
}

// the set's count per emitted group (grouped) or its tuple count (ungrouped)
Status DistinctAggregateRelation::emit_counts(DistinctSet& S, const DeviceBatch& inner_out, DeviceColumn* col, uint64_t* ungrouped_total) {
  hipStream_t s = ctx().stream;
  Status st;
  uint32_t hc[CTRL_WORDS];
  DFX_RETURN_IF_ERROR(read_ctrl(S, hc));
  const uint64_t occupied = hc[CTRL_OCCUPIED];
  counters().distinct_inserted += (long long)occupied;
  auto total = device_alloc(sizeof(uint64_t), &st);
  if (!total) return st;
  DFX_HIP(hipMemsetAsync(total.get(), 0, sizeof(uint64_t), s));
  if (kw_out_ == 0) {
    DevTable none;
    memset(&none, 0, sizeof(none));
    DFX_HIP(launch_distinct_count(S.T, none, (uint64_t*)total.get(), s));
    DFX_HIP(hipMemcpyAsync(ungrouped_total, total.get(), sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    DFX_HIP(hipStreamSynchronize(s));
    return Status::OK();
  }
  // count table: the key prefix + one ACC_ADD_U64 plane
  EmitTable E;
  DFX_RETURN_IF_ERROR(alloc_emit_table(S.kw, occupied, 1, &E));
  const DevTable& Cn = E.T;
  DFX_HIP(launch_distinct_count(S.T, Cn, (uint64_t*)total.get(), s));
  const int64_t g = inner_out.num_rows;
  DevDistinctKeys K;
  std::vector<DeviceColumn> ids;
  DFX_RETURN_IF_ERROR(emitted_keys(inner_out, &K, &ids));
  auto vals = device_alloc(sizeof(uint64_t) * (size_t)std::max<int64_t>(g, 1), &st);
  if (!vals) return st;
  DFX_HIP(launch_distinct_lookup(Cn, K, kw_out_, g, (uint64_t*)vals.get(), s));
  uint32_t cc[CTRL_WORDS];
  DFX_HIP(hipMemcpyAsync(cc, Cn.ctrl, sizeof(cc), hipMemcpyDeviceToHost, s));
  DFX_HIP(hipStreamSynchronize(s));
  if (cc[CTRL_ERROR]) return Status::Err(DFX_INTERNAL_ERROR, "COUNT_DISTINCT: count table overflow");
  col->dtype = DFX_UINT64;
  col->length = g;
  col->null_count = 0;
  col->values = vals.get();
  col->validity = nullptr;
  col->owners.push_back(vals);
  return Status::OK();
}

Status DistinctAggregateRelation::next(DeviceBatch* out, bool* has) {
  *has = false;
  if (done_) return Status::OK();
  done_ = true;
  DeviceBatch in;
  bool in_has = false;
  DFX_RETURN_IF_ERROR(inner_->next(&in, &in_has));  // drains the input through the tap
  if (!in_has) return Status::OK();
  DFX_HIP(hipStreamSynchronize(ctx().stream));
  for (auto& sp : sets_) {  // the last batch's spill and growth
    DistinctSet& S = *sp;
    if (!S.T.keys) continue;
    S.snap_pending = false;
    uint32_t hc[CTRL_WORDS];
    DFX_RETURN_IF_ERROR(read_ctrl(S, hc));
    DFX_RETURN_IF_ERROR(settle(S, hc, true));
  }
  out->num_rows = in.num_rows;
  out->columns.clear();
  for (int k = 0; k < kw_out_; ++k) out->columns.push_back(in.columns[(size_t)k]);
  std::vector<DeviceColumn> set_cols(sets_.size()), min_cols(sets_.size()), max_cols(sets_.size());
  std::vector<uint64_t> set_total(sets_.size(), 0);
  for (size_t si = 0; si < sets_.size(); ++si) {
    DistinctSet& S = *sets_[si];
    if (S.want_min || S.want_max) DFX_RETURN_IF_ERROR(emit_extrema(S, in, &min_cols[si], &max_cols[si]));
    if (!S.want_count) continue;
    if (!S.T.keys) {  // no batch reached the set: every group counts 0
      if (kw_out_ > 0) DFX_RETURN_IF_ERROR(zero_count_column(in.num_rows, &set_cols[si]));
      continue;
    }
    DFX_RETURN_IF_ERROR(emit_counts(S, in, &set_cols[si], &set_total[si]));
  }
  if (kw_out_ == 0) {  // one row: the set's count, valid exactly where COUNT(x) of the same rows is
    for (size_t si = 0; si < sets_.size(); ++si) {
      if (!sets_[si]->want_count) continue;
      const bool valid = hidden_count_[si] < 0 || in.columns[(size_t)hidden_count_[si]].null_count == 0;
      DFX_RETURN_IF_ERROR(ungrouped_count_row(set_total[si], valid, &set_cols[si]));
    }
  }
  for (size_t j = 0; j < out_src_.size(); ++j) {
    const int src = out_src_[j];
    if (src >= 0) out->columns.push_back(in.columns[(size_t)src]);
    else out->columns.push_back((out_role_[j] == ROLE_MIN ? min_cols : out_role_[j] == ROLE_MAX ? max_cols : set_cols)[(size_t)(-1 - src)]);
  }
  *has = true;
  return Status::OK();
}

}  // namespace dfx
