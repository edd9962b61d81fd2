// dfx_aggregate_partial.cpp -- AggregateRelation: multi-GPU export / import of group partials and ungrouped state.
#include "dfx_aggregate_impl.hpp"

namespace dfx {

// ---- multi-GPU partial exchange ---------------------------------------------------------------------
Status AggregateRelation::partial_build(int world, int* n_words, int64_t* counts) {
  if (!impl_->dicts.empty())
    return Status::Err(DFX_NOT_IMPLEMENTED, "multi-GPU exchange of Utf8 GROUP BY keys (dictionary ids are rank-local)");
  Impl& m = *impl_;
  if (!m.deferred.ok()) return m.deferred;
  if (m.kw == 0) return Status::Err(DFX_NOT_IMPLEMENTED, "partial exchange is for GROUP BY aggregates");
  if (world < 1 || world > 1024) return Status::Err(DFX_GENERAL, "world must be in 1..1024");
  DFX_RETURN_IF_ERROR(m.partial_view_check());  // (by accumulators, not by chunks: the drain may re-chunk -- one scan per aggregate)
  DFX_RETURN_IF_ERROR(m.drain());
  hipStream_t s = ctx().stream;
  Status st;
  auto dc = device_alloc(sizeof(uint64_t) * (size_t)world, &st);
  if (!dc) return st;
  DFX_HIP(hipMemsetAsync(dc.get(), 0, sizeof(uint64_t) * (size_t)world, s));
  DFX_HIP(launch_partial_count(m.T, world, (uint64_t*)dc.get(), s));
  m.export_counts.assign((size_t)world, 0);
  DFX_HIP(hipMemcpyAsync(m.export_counts.data(), dc.get(), sizeof(uint64_t) * (size_t)world, hipMemcpyDeviceToHost, s));
  DFX_HIP(hipStreamSynchronize(s));
  for (int r = 0; r < world; ++r) counts[r] = (int64_t)m.export_counts[r];
  *n_words = m.kw + m.na_total;
  return Status::OK();
}

Status AggregateRelation::partial_export(void* dst_device, int64_t dst_words) {
  Impl& m = *impl_;
  if (m.export_counts.empty()) return Status::Err(DFX_GENERAL, "partial_build must precede partial_export");
  std::vector<int64_t> counts(m.export_counts.begin(), m.export_counts.end());
  return partial_export_with(counts, dst_device, dst_words, true, /*all_planes=*/true);
}

// the count step of partial_build with the counts left on the device: d_counts[0, world) = groups per destination
// rank, d_counts[world, 2 world) = scratch for the counts received from the peers
Status AggregateRelation::partial_count_device(int world, int* n_words, uint64_t** d_counts, std::shared_ptr<void>* owner) {
  if (!impl_->dicts.empty())
    return Status::Err(DFX_NOT_IMPLEMENTED, "multi-GPU exchange of Utf8 GROUP BY keys (dictionary ids are rank-local)");
  Impl& m = *impl_;
  if (!m.deferred.ok()) return m.deferred;
  if (m.kw == 0) return Status::Err(DFX_INTERNAL_ERROR, "partial_count_device is for GROUP BY aggregates");
  if (world < 1 || world > 1024) return Status::Err(DFX_GENERAL, "world must be in 1..1024");
  DFX_RETURN_IF_ERROR(m.partial_view_check());
  DFX_RETURN_IF_ERROR(m.drain());
  hipStream_t s = ctx().stream;
  Status st;
  *owner = device_alloc(sizeof(uint64_t) * (size_t)world * 2, &st);
  if (!*owner) return st;
  DFX_HIP(hipMemsetAsync(owner->get(), 0, sizeof(uint64_t) * (size_t)world * 2, s));
  DFX_HIP(launch_partial_count(m.T, world, (uint64_t*)owner->get(), s));
  *d_counts = (uint64_t*)owner->get();
  *n_words = m.kw + m.na_total;
  m.export_counts.assign((size_t)world, 0);  // (filled by partial_export_with)
  return Status::OK();
}

Status AggregateRelation::partial_export_with(const std::vector<int64_t>& counts, void* dst_device, int64_t dst_words, bool sync, bool all_planes) {
  Impl& m = *impl_;
  const int world = (int)counts.size();
  // all_planes: the public partial_* path -- every accumulator in one row, whatever chunking the drain installed;
  // otherwise the ACTIVE chunk's planes (the in-library exchange walks the chunks itself)
  const DevTable Tv = all_planes ? m.full_view(m.T, m.accs_full) : m.T;
  const int na_v = all_planes ? m.na_total : m.na();
  m.export_counts.assign(counts.begin(), counts.end());
  std::vector<uint64_t> base((size_t)world, 0);
  uint64_t total = 0;
  for (int r = 0; r < world; ++r) {
    base[r] = total;
    total += m.export_counts[r];
  }
  if ((uint64_t)dst_words < total * (uint64_t)(m.kw + na_v))
    return Status::Err(DFX_GENERAL, "partial export buffer too small");
  hipStream_t s = ctx().stream;
  Status st;
  auto dbase = device_alloc(sizeof(uint64_t) * (size_t)world * 3, &st);
  if (!dbase) return st;
  uint64_t* d = (uint64_t*)dbase.get();
  {  // bucket bases, bucket counts, zeroed cursors: one blocking copy of 3 x world words (the host vector dies with this scope)
    std::vector<uint64_t> hw((size_t)world * 3, 0);
    for (int r = 0; r < world; ++r) {
      hw[(size_t)r] = base[(size_t)r];
      hw[(size_t)world + r] = m.export_counts[(size_t)r];
    }
    DFX_HIP(hipMemcpy(d, hw.data(), sizeof(uint64_t) * hw.size(), hipMemcpyHostToDevice));
  }
  if (m.kw == 1) DFX_HIP(launch_fill_u64(m.T.keys + m.T.mask + 1, kEmptyKey, 1, s));
  DFX_HIP(launch_partial_scatter(Tv, world, d, d + world, d + 2 * world, (uint64_t*)dst_device, s));
  if (sync) {
    DFX_HIP(hipStreamSynchronize(s));
  } else {
    m.table_owners.push_back(dbase);  // the scatter kernel is still queued: keep its base / count words alive
  }
  return Status::OK();
}

// ---- the in-library exchange, piece by piece (dfx_exchange.cpp drives the collectives between them) ---------------------
int AggregateRelation::exchange_chunks() const { return std::max<int>(1, (int)impl_->chunks.size()); }
int AggregateRelation::exchange_chunk_words(int c) const {
  const Impl& m = *impl_;
  return m.kw + (m.chunks.empty() ? 0 : m.chunks[(size_t)c].n);
}
int AggregateRelation::exchange_dicts() const { return (int)impl_->dicts.size(); }

Status AggregateRelation::exchange_drain() {
  Impl& m = *impl_;
  if (!m.deferred.ok()) return m.deferred;
  if (m.kw == 0) return Status::Err(DFX_INTERNAL_ERROR, "exchange_drain is for GROUP BY aggregates");
  return m.drain();
}

// the groups of the drained table as the host knows them (the control block's count after the drain's last check) + the
// sentinel group's slot: what partial_count can find at most
uint64_t AggregateRelation::exchange_group_bound() const { return impl_->dec.occupied_known + 1; }

Status AggregateRelation::exchange_count(int world, uint64_t* d_counts) {
  Impl& m = *impl_;
  if (world < 1 || world > 1024) return Status::Err(DFX_GENERAL, "world must be in 1..1024");
  hipStream_t s = ctx().stream;
  DFX_HIP(hipMemsetAsync(d_counts, 0, sizeof(uint64_t) * (size_t)world, s));
  DFX_HIP(launch_partial_count(m.T, world, d_counts, s));
  return Status::OK();
}

Status AggregateRelation::exchange_export_chunk(int c, const std::vector<int64_t>& counts, void* dst_device, int64_t dst_words) {
  Impl& m = *impl_;
  if (m.chunks.size() > 1) m.activate(c);
  return partial_export_with(counts, dst_device, dst_words, /*sync=*/false, /*all_planes=*/false);
}

Status AggregateRelation::exchange_import_begin(uint64_t total_groups) {
  Impl& m = *impl_;
  if (!m.built) return Status::Err(DFX_GENERAL, "the input must be drained before the import");
  const int cap_log2 = std::max(10, ceil_log2(4 * (total_groups + 1)));
  if (cap_log2 > 31) return Status::Err(DFX_EXECUTION_ERROR, "GROUP BY table would exceed 2^31 slots");
  m.import_owners.clear();
  m.import_accs_full = nullptr;
  if (m.chunks.size() > 1) m.activate(0);
  m.import_keep = {m.ctrl, m.stats};  // the OLD table's control block stays readable: later chunks are still exported from it
  DFX_RETURN_IF_ERROR(m.alloc_table(cap_log2, &m.import_T, &m.import_owners, true, &m.import_accs_full));
  return Status::OK();
}

// rows of nw words, bucket after bucket, into a table sized for all of them
static Status merge_buckets(const void* src_device, int nw, const int64_t* counts, int n_buckets, const DevTable& into, hipStream_t s) {
  uint64_t off = 0;
  for (int b = 0; b < n_buckets; ++b) {
    if (counts[b] > 0)
      DFX_HIP(launch_merge_bucket((const uint64_t*)src_device + (size_t)nw * off, (uint64_t)counts[b], into, no_spill_rows(), s));
    off += (uint64_t)counts[b];
  }
  return Status::OK();
}

Status AggregateRelation::exchange_import_chunk(int c, const void* src_device, const int64_t* counts, int n_buckets) {
  Impl& m = *impl_;
  hipStream_t s = ctx().stream;
  // chunk c's planes of the NEW table; the first chunk inserts the keys, the others find them
  const DevTable Tc = m.chunks.size() > 1 ? m.view_of(m.import_T, m.import_accs_full, c) : m.import_T;
  return merge_buckets(src_device, exchange_chunk_words(c), counts, n_buckets, Tc, s);
}

Status AggregateRelation::exchange_import_finish() {
  Impl& m = *impl_;
  DFX_HIP(hipStreamSynchronize(ctx().stream));
  m.replace_table(m.import_T, m.import_accs_full, m.import_owners, true);
  m.import_owners.clear();
  m.import_keep.clear();
  m.export_counts.clear();
  if (m.chunks.size() > 1) m.activate(0);
  uint32_t hc[CTRL_WORDS];
  DFX_RETURN_IF_ERROR(m.read_ctrl(hc));
  if (hc[CTRL_ERROR]) return error_from_ctrl(hc[CTRL_ERROR]);
  m.dec.occupied_known = hc[CTRL_OCCUPIED];
  return Status::OK();
}

// the strings of dictionary d in local-id order (lengths + bytes back to back)
Status AggregateRelation::exchange_dict_local(int d, std::vector<uint32_t>* lens, std::vector<uint8_t>* pool) {
  return impl_->dicts[(size_t)d].dict.download(lens, pool);
}

// installs the GLOBAL dictionary (strings by global id: lens + bytes back to back) as dictionary d and rewrites the key
// plane of that GROUP BY column: local id -> remap[local id].  The table is not probed again before the exchange scatters
// it (count / scatter walk the slots), and what the import builds is keyed by global ids from the start.
Status AggregateRelation::exchange_dict_globalise(int d, const std::vector<uint32_t>& lens, const std::vector<uint8_t>& pool,
                                                   const std::vector<uint64_t>& remap) {
  Impl& m = *impl_;
  Impl::DictKey& k = m.dicts[(size_t)d];
  hipStream_t s = ctx().stream;
  Status st;
  if (!remap.empty()) {
    auto dremap = device_alloc(sizeof(uint64_t) * remap.size(), &st);
    if (!dremap) return st;
    DFX_HIP(hipMemcpy(dremap.get(), remap.data(), sizeof(uint64_t) * remap.size(), hipMemcpyHostToDevice));
    uint64_t* plane = m.T.keys + (uint64_t)k.key * m.T.stride;
    DFX_HIP(launch_dict_remap_plane(plane, m.T.mask + 2, (const uint64_t*)dremap.get(), (uint64_t)remap.size(), s));
    DFX_HIP(hipStreamSynchronize(s));  // dremap dies with this scope
  }
  return k.dict.install(lens, pool);
}

Status AggregateRelation::ungrouped_select_chunk(int c) {
  Impl& m = *impl_;
  if (c < 0 || c >= exchange_chunks()) return Status::Err(DFX_GENERAL, "no such chunk");
  if (m.chunks.size() > 1) m.activate(c);
  return Status::OK();
}

static uint64_t host_wrap_to(uint8_t t, uint64_t x) {  // == wrap_to (dfx_k_base_inl.hpp)
  switch (t) {
    case DFX_INT8: return (uint64_t)(int64_t)(int8_t)x;
    case DFX_INT16: return (uint64_t)(int64_t)(int16_t)x;
    case DFX_INT32: return (uint64_t)(int64_t)(int32_t)x;
    case DFX_UINT8: return (uint64_t)(uint8_t)x;
    case DFX_UINT16: return (uint64_t)(uint16_t)x;
    case DFX_UINT32: return (uint64_t)(uint32_t)x;
    default: return x;
  }
}

// ---- ungrouped aggregates across ranks ---------------------------------------------------------------
bool AggregateRelation::is_ungrouped() const { return impl_->deferred.ok() && impl_->group.empty(); }
Status AggregateRelation::ungrouped_state_begin() {
  Impl& m = *impl_;
  if (!m.deferred.ok()) return m.deferred;
  if (m.group.empty() && m.aggr.empty())
    return Status::Err(DFX_INTERNAL_ERROR, "assertion failed: record batch needs at least one column");
  return m.drain();
}
int AggregateRelation::ungrouped_state_words() const { return 2 * kMaxAggs; }
const void* AggregateRelation::ungrouped_state_device() const { return impl_->chunks.empty() ? nullptr : impl_->cur().state.get(); }

// AccumulatorSet::accumulate_scalar (aggregate.rs:107-145,176-214,245-283) between the ranks' scalars, folded in rank
// order: the same arms as the device's batch fold (k_reduce_fold)
Status AggregateRelation::ungrouped_state_merge(const uint64_t* all, int world, int rank) {
  (void)rank;
  Impl& m = *impl_;
  uint64_t out[2 * kMaxAggs];
  memset(out, 0, sizeof(out));
  for (int a = 0; a < m.na(); ++a) {
    const int a0 = m.chunks[(size_t)m.cur_chunk].a0;  // arg_dtype / func are indexed over ALL accumulators, the state block over the active chunk's
    const int t = m.arg_dtype[a0 + a], f = m.func[a0 + a];
    bool has = false;
    uint64_t cur = 0;
    for (int r = 0; r < world; ++r) {
      const uint64_t* st = all + (size_t)r * 2 * kMaxAggs;
      if (!st[2 * a]) continue;
      const uint64_t val = st[2 * a + 1];
      if (!has) {
        has = true;
        cur = val;
        continue;
      }
      if (f == AGG_COUNT) {
        cur += val;
      } else if (t == DFX_FLOAT64) {
        double x, y;
        memcpy(&x, &cur, 8);
        memcpy(&y, &val, 8);
        const double o = f == AGG_MIN ? fmin(x, y) : f == AGG_MAX ? fmax(x, y) : x + y;
        memcpy(&cur, &o, 8);
      } else if (t == DFX_FLOAT32) {
        float x, y;
        const uint32_t cx = (uint32_t)cur, cy = (uint32_t)val;
        memcpy(&x, &cx, 4);
        memcpy(&y, &cy, 4);
        const float o = f == AGG_MIN ? fminf(x, y) : f == AGG_MAX ? fmaxf(x, y) : x + y;
        uint32_t ob;
        memcpy(&ob, &o, 4);
        cur = ob;
      } else if (dtype_is_signed(t)) {
        const int64_t x = (int64_t)cur, y = (int64_t)val;
        cur = f == AGG_MIN ? (uint64_t)std::min(x, y) : f == AGG_MAX ? (uint64_t)std::max(x, y) : host_wrap_to((uint8_t)t, cur + val);
      } else {
        cur = f == AGG_MIN ? std::min(cur, val) : f == AGG_MAX ? std::max(cur, val) : host_wrap_to((uint8_t)t, cur + val);
      }
    }
    out[2 * a] = has ? 1 : 0;
    out[2 * a + 1] = cur;
  }
  DFX_HIP(hipMemcpy(m.cur().state.get(), out, sizeof(out), hipMemcpyHostToDevice));
  return Status::OK();
}

Status AggregateRelation::partial_import(const void* src_device, const int64_t* counts, int n_buckets) {
  Impl& m = *impl_;
  if (!m.built) return Status::Err(DFX_GENERAL, "partial_build must precede partial_import");
  hipStream_t s = ctx().stream;
  uint64_t total = 0;
  for (int b = 0; b < n_buckets; ++b) total += (uint64_t)counts[b];
  const int cap_log2 = std::max(10, ceil_log2(4 * (total + 1)));
  if (cap_log2 > 31) return Status::Err(DFX_EXECUTION_ERROR, "GROUP BY table would exceed 2^31 slots");
  DevTable Tn;
  std::vector<std::shared_ptr<void>> owners;
  uint64_t* accs_full_new = nullptr;
  DFX_RETURN_IF_ERROR(m.partial_view_check());
  DFX_RETURN_IF_ERROR(m.alloc_table(cap_log2, &Tn, &owners, true, &accs_full_new));
  // rows as partial_export wrote them: every accumulator
  DFX_RETURN_IF_ERROR(merge_buckets(src_device, m.kw + m.na_total, counts, n_buckets, m.full_view(Tn, accs_full_new), s));
  DFX_HIP(hipStreamSynchronize(s));
  m.replace_table(Tn, accs_full_new, owners, false);
  m.export_counts.clear();
  uint32_t hc[CTRL_WORDS];
  DFX_RETURN_IF_ERROR(m.read_ctrl(hc));
  m.dec.occupied_known = hc[CTRL_OCCUPIED];
  return Status::OK();
}

}  // namespace dfx

using namespace dfx;

extern "C" {

// a stream over distinct sets (COUNT_DISTINCT, MIN / MAX of Utf8) has no partial state to exchange
static Status distinct_stream_refusal(struct ArrowArrayStream* s) { return distinct_sets_exchange_refusal(peek_exported(s)); }

static AggregateRelation* as_aggregate(struct ArrowArrayStream* s) {
  Relation* r = peek_exported(s);
  if (!r || r->kind() != REL_AGGREGATE) return nullptr;
  return static_cast<AggregateRelation*>(r);
}

int32_t dfx_aggregate_partial_build(struct ArrowArrayStream* agg, int32_t world, int32_t* n_words, int64_t* counts,
                                    char* err, size_t errlen) {
  return c_abi_guard(err, errlen, [&]() -> int32_t {
    if (Status refused = distinct_stream_refusal(agg); !refused.ok()) return to_c(refused, err, errlen);
    AggregateRelation* a = as_aggregate(agg);
    if (!a) return to_c(Status::Err(DFX_GENERAL, "not an aggregate stream of this library"), err, errlen);
    int nw = 0;
    Status st = a->partial_build(world, &nw, counts);
    if (n_words) *n_words = nw;
    return to_c(st, err, errlen);
  });
}

int32_t dfx_aggregate_partial_export(struct ArrowArrayStream* agg, void* dst_device, int64_t dst_words, char* err,
                                     size_t errlen) {
  return c_abi_guard(err, errlen, [&]() -> int32_t {
    if (Status refused = distinct_stream_refusal(agg); !refused.ok()) return to_c(refused, err, errlen);
    AggregateRelation* a = as_aggregate(agg);
    if (!a) return to_c(Status::Err(DFX_GENERAL, "not an aggregate stream of this library"), err, errlen);
    return to_c(a->partial_export(dst_device, dst_words), err, errlen);
  });
}

int32_t dfx_aggregate_partial_import(struct ArrowArrayStream* agg, const void* src_device, const int64_t* counts,
                                     int32_t n_buckets, char* err, size_t errlen) {
  return c_abi_guard(err, errlen, [&]() -> int32_t {
    if (Status refused = distinct_stream_refusal(agg); !refused.ok()) return to_c(refused, err, errlen);
    AggregateRelation* a = as_aggregate(agg);
    if (!a) return to_c(Status::Err(DFX_GENERAL, "not an aggregate stream of this library"), err, errlen);
    return to_c(a->partial_import(src_device, counts, n_buckets), err, errlen);
  });
}

}  // extern "C"
