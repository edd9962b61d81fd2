// dfx_k_parquet_write_dict.hip -- the "dictionary" option of the Parquet writer on the device (deviation D13):
// per column chunk a dictionary in order of first occurrence, built launch by launch, and pages of dictionary indices.  The format, the
// sizes and the per-launch decision are dfx_parquet_dict_enc.hpp's, which the host encoder restates sequentially; the tables between the
// kernels and the order of the chain are in dfx_parquet_write.hpp.
//
// No lane waits for another lane's store.  insert: a lane claims a table slot by an agent-scope CAS on its key word and uses only what the
// CAS returns (a stale read of an empty word only sends it into the CAS, which arbitrates; a key word never changes once set), then
// lowers the slot's first_row by an agent-scope min whose result it ignores.  Who introduces an entry (the row that IS first_row), which
// id it gets (prefix sums of the introducing rows, in row order: first occurrence) and where its bytes go are settled by LATER launches
// on the same stream: mark, decide, commit.  No spin, no claim-fill-publish.
//
// Shared words.  Bit-packed indices of two tiles share words and a value block starts at any byte, so EVERY store of a dictionary data
// page is an agent-scope atomicOr on an aligned 32-bit word of the page's own span in a zeroed buffer (pqw_or_bits' rule for Boolean
// pages); pages start 8-byte aligned.  The dictionary body is written with plain stores: entries are disjoint bytes.
//
// Bounds.  commit and encode store only after they have found their own recount equal to what decide / scan were given, every id
// below the chunk's entries, and every span inside the body, the page and the buffer; otherwise they store nothing and raise ctrl
// bit 0.  Utf8 rows are clamped as in dfx_k_parquet_write.hip.
#include <algorithm>

#include "dfx_k_parquet_write_inl.hpp"
#include "dfx_launch.hpp"

namespace dfx {

using namespace pqw;

namespace {
DEV uint64_t pqwd_mix(uint64_t x) {  // (the 64-bit finaliser of MurmurHash3: a bijection)
  x ^= x >> 33;
  x *= 0xFF51AFD7ED558CCDull;
  x ^= x >> 33;
  x *= 0xC4CEB9FE1A85EC53ull;
  x ^= x >> 33;
  return x;
}
DEV uint64_t pqwd_hash_bytes(const uint8_t* p, uint32_t n) {  // FNV-1a over the bytes, then mixed with the length
  uint64_t h = 0xCBF29CE484222325ull;
  for (uint32_t i = 0; i < n; ++i) h = (h ^ p[i]) * 0x100000001B3ull;
  return pqwd_mix(h ^ ((uint64_t)n << 32));
}
// the same job by the whole wave: lane l takes bytes l, l + 64, ... into an FNV-1a stream seeded with l; the 64 streams, mixed, are summed
DEV uint64_t pqwd_hash_strided(const uint8_t* p, uint32_t n, int lane) {
  uint64_t h = 0xCBF29CE484222325ull ^ (uint64_t)lane;
  for (uint32_t i = (uint32_t)lane; i < n; i += 64u) h = (h ^ p[i]) * 0x100000001B3ull;
  return pqwd_mix(pqw_wave_sum(pqwd_mix(h)) ^ ((uint64_t)n << 32));
}
DEV uint64_t pqwd_stored(const DevPqwCol& col, int64_t row) {
  uint64_t raw;
  switch (col.dtype) {
    case T_I8:
    case T_U8: raw = ((const uint8_t*)col.values)[row]; break;
    case T_I16:
    case T_U16: raw = ((const uint16_t*)col.values)[row]; break;
    case T_I32:
    case T_U32:
    case T_F32: raw = ((const uint32_t*)col.values)[row]; break;
    default: raw = ((const uint64_t*)col.values)[row];
  }
  return widen((int)col.dtype, raw);
}
DEV uint32_t pqwd_wave_min(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = std::min(v, (uint32_t)__shfl_xor((int)v, d, 64));
  return v;
}
DEV uint32_t pqwd_wave_max(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = std::max(v, (uint32_t)__shfl_xor((int)v, d, 64));
  return v;
}
// ORs the low bits of v into the buffer from absolute bit `bit` on (v << (bit & 31) fits 64 bits); a word without a bit is skipped
DEV void pqwd_or_value(uint32_t* out32, uint64_t bit, uint32_t v) {
  const uint64_t x = (uint64_t)v << (uint32_t)(bit & 31u);
  if ((uint32_t)x) __hip_atomic_fetch_or(out32 + (bit >> 5), (uint32_t)x, RLX_AGENT);
  if (x >> 32) __hip_atomic_fetch_or(out32 + (bit >> 5) + 1, (uint32_t)(x >> 32), RLX_AGENT);
}
// whether the lane's row introduces an entry: it reached a slot without an id and is the least such row of the launch
DEV bool pqwd_introduces(const PqwdSlot& s, bool has, int64_t row) { return has && s.id == kPqwdNone && s.first_row == (uint32_t)row; }
// copies n bytes, a lane per value up to kLongValue bytes and the whole wave on every longer one (`live` lanes have a value)
DEV void pqwd_copy_values(uint8_t* dst, const uint8_t* src, uint32_t n, bool live, int lane) {
  const bool is_long = live && n > kLongValue;
  if (live && !is_long)
    for (uint32_t i = 0; i < n; ++i) dst[i] = src[i];
  uint64_t todo = __ballot(is_long);
  while (todo) {
    const int from = (int)__builtin_ctzll(todo);
    todo &= todo - 1ull;
    uint8_t* d = (uint8_t*)__shfl((unsigned long long)dst, from, 64);
    const uint8_t* s = (const uint8_t*)__shfl((unsigned long long)src, from, 64);
    const uint32_t len = (uint32_t)__shfl((int)n, from, 64);
    for (uint32_t i = (uint32_t)lane; i < len; i += 64u) d[i] = s[i];
  }
}
}  // namespace

// a lane per row of every column: the valid row's key finds or claims its slot; an unassigned slot learns its least row
__global__ __launch_bounds__(kPqwBlock) void k_pqwd_insert(const DevPqwdPlan P, uint32_t* __restrict__ slot_of_row) {
  const int lane = lane_id();
  const int64_t t = (int64_t)blockIdx.x * (kPqwBlock / 64) + (int64_t)(threadIdx.x >> 6);
  if (t >= P.base.n_tiles * P.base.n_cols) return;
  const int c = (int)(t / P.base.n_tiles);
  const int64_t row = (t % P.base.n_tiles) * 64 + lane;
  const bool in = row < P.base.rows;
  const DevPqwCol col = P.base.col[c];
  const DevPqwdCol D = P.dict[c];
  const PqwRow r = pqw_row(col, row, in, P.base.rows);
  uint64_t key = 0;
  if (col.dtype == T_UTF8) {  // a lane per value; the whole wave on every value longer than kLongValue, as mark and commit split them
    const bool is_long = r.valid && r.len > kLongValue;
    if (r.valid && !is_long) key = pqwd_hash_bytes(col.data + r.begin, r.len);
    uint64_t todo = __ballot(is_long);
    while (todo) {
      const int from = (int)__builtin_ctzll(todo);
      todo &= todo - 1ull;
      const uint8_t* p = col.data + (int64_t)__shfl((long long)r.begin, from, 64);
      const uint32_t len = (uint32_t)__shfl((int)r.len, from, 64);
      const uint64_t whole = pqwd_hash_strided(p, len, lane);
      if (lane == from) key = whole;
    }
    key &= P.hash_mask;
  } else if (r.valid) {
    key = pqwd_stored(col, row);
  }
  uint32_t slot = kPqwdNone;
  bool claimed = false;
  if (r.valid) {
    if (key == kPqwdEmpty) {
      slot = D.mask + 1u;  // the empty word's own value: the slot after the table, which no probe reaches
    } else {
      const uint32_t bound = std::min(D.mask + 1u, kPqwdMaxProbe);
      uint32_t at = (uint32_t)pqwd_mix(key) & D.mask;
      for (uint32_t k = 0; k < bound && slot == kPqwdNone; ++k, at = (at + 1u) & D.mask) {
        // (a launch whose overflow flag is up falls back whatever this row finds: once the flag is seen -- late or never, a stale
        // read only costs probes -- a filling table is not walked a thousand slots per row)
        if ((k & 31u) == 0u && (__hip_atomic_load(&D.state->flags, RLX_AGENT) & PQWD_OVERFLOW)) break;
        uint64_t seen = __hip_atomic_load(&D.slots[at].key, RLX_AGENT);
        if (seen == kPqwdEmpty) {  // (on failure the CAS leaves the word's value in `seen`)
          claimed = __hip_atomic_compare_exchange_strong(&D.slots[at].key, &seen, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          if (claimed) seen = key;
        }
        if (seen == key) slot = at;
      }
    }
    // (first_row only falls: a stale read of it costs an atomic that changes nothing, never a missed one)
    if (slot != kPqwdNone && D.slots[slot].id == kPqwdNone && __hip_atomic_load(&D.slots[slot].first_row, RLX_AGENT) > (uint32_t)row)
      __hip_atomic_fetch_min(&D.slots[slot].first_row, (uint32_t)row, RLX_AGENT);
  }
  // Key words claimed in this launch are distinct keys the chunk has not held: new entries (for Utf8 at most as many as the new
  // strings).  Once they exceed the room N - E the rule makes the launch fall back, so the flag goes up then -- at half the table --
  // and not only when a row finds the table full.  One add per wave that claimed; its returned value is all the wave uses.
  // (the flag is one word per column: a wave raises it once, and only while it does not read it raised -- a million lanes ORing one
  // address would cost more than the probing)
  const uint32_t wave_claims = (uint32_t)__popcll(__ballot(claimed));
  const bool wave_lost = __ballot(r.valid && slot == kPqwdNone) != 0ull;
  if ((wave_claims || wave_lost) && lane == 0) {
    bool raise = wave_lost;
    if (wave_claims) raise = raise || D.state->entries + __hip_atomic_fetch_add(&D.state->claimed, wave_claims, RLX_AGENT) + wave_claims > (uint64_t)D.limit;
    if (raise && !(__hip_atomic_load(&D.state->flags, RLX_AGENT) & PQWD_OVERFLOW)) __hip_atomic_fetch_or(&D.state->flags, PQWD_OVERFLOW, RLX_AGENT);
  }
  if (in) slot_of_row[(int64_t)c * P.base.rows + row] = slot;
}

// one wave per tile of every column: valid rows, the rows that introduce an entry and their body bytes, the least and greatest slot;
// Utf8: every valid row's bytes against its slot's representative (an earlier launch's entry in the body, or row first_row of this one)
__global__ __launch_bounds__(kPqwBlock) void k_pqwd_mark(const DevPqwdPlan P, const uint32_t* __restrict__ slot_of_row, PqwdTile* __restrict__ tiles) {
  const int lane = lane_id();
  const int64_t t = (int64_t)blockIdx.x * (kPqwBlock / 64) + (int64_t)(threadIdx.x >> 6);
  if (t >= P.base.n_tiles * P.base.n_cols) return;
  const int c = (int)(t / P.base.n_tiles);
  const int64_t row = (t % P.base.n_tiles) * 64 + lane;
  const DevPqwCol col = P.base.col[c];
  const DevPqwdCol D = P.dict[c];
  const PqwRow r = pqw_row(col, row, row < P.base.rows, P.base.rows);
  const uint32_t slot = r.valid ? slot_of_row[(int64_t)c * P.base.rows + row] : kPqwdNone;
  const bool has = slot != kPqwdNone;
  PqwdSlot S = {0, 0, 0};
  if (has) S = D.slots[slot];
  const bool intro = pqwd_introduces(S, has, row);
  const uint32_t cnt = (uint32_t)__popcll(__ballot(r.valid));
  const uint32_t entries = (uint32_t)__popcll(__ballot(intro));
  const uint64_t bytes = pqw_wave_sum(intro ? dict_entry_bytes((int)col.dtype, r.len) : 0ull);
  const uint32_t lo = pqwd_wave_min(has ? slot : kPqwdNone), hi = pqwd_wave_max(has ? slot : 0u);
  if (col.dtype == T_UTF8) {
    const bool cmp = has && !intro;
    const uint8_t* rep = col.data;
    uint32_t rep_len = 0;
    bool differs = false;
    if (cmp && S.id != kPqwdNone) {
      const uint8_t* e = D.body + D.entry_off[S.id];
      rep_len = *(const pqw_u32*)e;
      rep = e + 4;
    } else if (cmp && (int64_t)S.first_row < P.base.rows) {
      const PqwRow f = pqw_row(col, (int64_t)S.first_row, true, P.base.rows);
      rep = col.data + f.begin;
      rep_len = f.len;
    } else if (cmp) {
      differs = true;
    }
    differs = differs || (cmp && rep_len != r.len);
    const bool is_long = cmp && !differs && r.len > kLongValue;
    if (cmp && !differs && !is_long)
      for (uint32_t i = 0; i < r.len && !differs; ++i) differs = col.data[r.begin + i] != rep[i];
    uint64_t todo = __ballot(is_long);
    bool long_differs = false;
    while (todo) {  // the whole wave on every value longer than kLongValue
      const int from = (int)__builtin_ctzll(todo);
      todo &= todo - 1ull;
      const uint8_t* a = col.data + (int64_t)__shfl((long long)r.begin, from, 64);
      const uint8_t* b = (const uint8_t*)__shfl((unsigned long long)rep, from, 64);
      const uint32_t len = (uint32_t)__shfl((int)r.len, from, 64);
      for (uint32_t i = (uint32_t)lane; i < len && !long_differs; i += 64u) long_differs = a[i] != b[i];
    }
    if (__ballot(differs || long_differs) && lane == 0) __hip_atomic_fetch_or(&D.state->flags, PQWD_COLLISION, RLX_AGENT);
  }
  if (lane == 0) {
    PqwdTile T;
    T.non_null = cnt;
    T.rank_base = 0;
    T.entries = entries;
    T.entry_base = 0;
    T.min_slot = lo;
    T.max_slot = hi;
    T.bytes = bytes;
    T.byte_base = 0;
    tiles[t] = T;
  }
}

// one workgroup per column: the exclusive scan of its tiles' {entries, bytes}, then the rule of the launch and the chunk's state
__global__ __launch_bounds__(1024) void k_pqwd_decide(const DevPqwdPlan P, PqwdTile* __restrict__ tiles) {
  __shared__ uint64_t se[1024], sb[1024];
  const int t = (int)threadIdx.x, c = (int)blockIdx.x;
  PqwdTile* tp = tiles + (int64_t)c * P.base.n_tiles;
  const int64_t n = P.base.n_tiles, chunk = (n + 1023) / 1024;
  const int64_t b = std::min<int64_t>((int64_t)t * chunk, n), e = std::min<int64_t>(b + chunk, n);
  uint64_t ne = 0, nb = 0;
  for (int64_t i = b; i < e; ++i) {
    ne += tp[i].entries;
    nb += tp[i].bytes;
  }
  se[t] = ne;
  sb[t] = nb;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const uint64_t ve = t >= d ? se[t - d] : 0ull, vb = t >= d ? sb[t - d] : 0ull;
    __syncthreads();
    se[t] += ve;
    sb[t] += vb;
    __syncthreads();
  }
  uint64_t re = se[t] - ne, rb = sb[t] - nb;
  for (int64_t i = b; i < e; ++i) {
    tp[i].entry_base = (uint32_t)re;
    tp[i].byte_base = rb;
    re += tp[i].entries;
    rb += tp[i].bytes;
  }
  if (t == 1023) {
    PqwdState st = *P.dict[c].state;
    if (st.mode == PQWD_MODE_DICT) {
      st.entries_before = st.entries;
      st.body_before = st.body_bytes;
      if (st.flags == 0u && dict_stays(st.entries, se[1023], st.body_bytes, sb[1023], P.dict[c].limit)) {
        st.entries += se[1023];
        st.body_bytes += sb[1023];
        st.width = dict_index_width(st.entries);
      } else {
        st.mode = PQWD_MODE_PLAIN;
      }
      st.claimed = 0;  // (insert's count of this launch's claims)
      *P.dict[c].state = st;
    }
  }
}

// one wave per page: the exclusive prefix of every tile's valid rows inside its page, whether all its indices are equal, its sizes
__global__ __launch_bounds__(kPqwBlock) void k_pqwd_scan(const DevPqwdPlan P, PqwdTile* __restrict__ tiles, PqwPage* __restrict__ pages) {
  const int lane = lane_id();
  const int64_t pg = (int64_t)blockIdx.x * (kPqwBlock / 64) + (int64_t)(threadIdx.x >> 6);
  if (pg >= P.base.n_pages * P.base.n_cols) return;
  const int c = (int)(pg / P.base.n_pages);
  const int64_t p = pg % P.base.n_pages;
  const int64_t tpp = P.base.page_rows / 64;
  const int64_t first = p * tpp;
  const int64_t count = std::min<int64_t>(tpp, P.base.n_tiles - first);
  const uint64_t n = (uint64_t)std::min<int64_t>(P.base.page_rows, P.base.rows - p * P.base.page_rows);
  PqwdTile* tp = tiles + (int64_t)c * P.base.n_tiles + first;
  uint64_t run_cnt = 0;
  uint32_t lo = kPqwdNone, hi = 0u;
  for (int64_t k = 0; k < count; k += 64) {
    const bool live = k + lane < count;
    const uint64_t cnt = live ? tp[k + lane].non_null : 0ull;
    const uint64_t icnt = wave_inclusive_scan(cnt);
    if (live) {
      tp[k + lane].rank_base = (uint32_t)(run_cnt + icnt - cnt);
      lo = std::min(lo, tp[k + lane].min_slot);
      hi = std::max(hi, tp[k + lane].max_slot);
    }
    run_cnt += (uint64_t)__shfl((unsigned long long)icnt, 63, 64);
  }
  lo = pqwd_wave_min(lo);
  hi = pqwd_wave_max(hi);
  if (lane == 0) {
    const DevPqwCol col = P.base.col[c];
    const PqwdState st = *P.dict[c].state;
    PqwPage g;
    g.base = 0;
    g.non_null = (uint32_t)run_cnt;
    g.kind = 0;
    g.level_bytes = 0;
    g.val_bytes = 0;
    g.flags = 0;
    if (st.mode == PQWD_MODE_DICT) {  // (a chunk that fell back in this launch takes no room: its pages are encoded PLAIN)
      const uint32_t lk = level_kind(col.optional != 0, n, run_cnt), run = dict_run_kind(run_cnt, lo == hi);
      g.kind = lk | run << kPqwdRunShift;
      g.level_bytes = (uint32_t)level_block_bytes(lk, n);
      g.val_bytes = dict_value_bytes(run, st.width, run_cnt);
      g.flags = body_fits(g.level_bytes, g.val_bytes) ? 0u : PQW_PAGE_TOO_LARGE;
    }
    pages[pg] = g;
  }
}

// one wave per tile of the columns that stayed in dictionary mode: the introducing rows take their ids, in row order, and append
// their entries to the dictionary body -- which IS the dictionary page's body
__global__ __launch_bounds__(kPqwBlock) void k_pqwd_commit(const DevPqwdPlan P, const uint32_t* __restrict__ slot_of_row, const PqwdTile* __restrict__ tiles,
                                                          uint64_t* __restrict__ ctrl) {
  const int lane = lane_id();
  const int64_t t = (int64_t)blockIdx.x * (kPqwBlock / 64) + (int64_t)(threadIdx.x >> 6);
  if (t >= P.base.n_tiles * P.base.n_cols) return;
  const int c = (int)(t / P.base.n_tiles);
  const DevPqwdCol D = P.dict[c];
  const PqwdState st = *D.state;
  if (st.mode != PQWD_MODE_DICT) return;
  const int64_t row = (t % P.base.n_tiles) * 64 + lane;
  const DevPqwCol col = P.base.col[c];
  const PqwdTile T = tiles[t];
  const PqwRow r = pqw_row(col, row, row < P.base.rows, P.base.rows);
  const uint32_t slot = r.valid ? slot_of_row[(int64_t)c * P.base.rows + row] : kPqwdNone;
  const bool has = slot != kPqwdNone;
  PqwdSlot S = {0, 0, 0};
  if (has) S = D.slots[slot];
  const bool intro = pqwd_introduces(S, has, row);
  const uint64_t iw = __ballot(intro);
  const uint32_t entries = (uint32_t)__popcll(iw), rank = (uint32_t)__popcll(iw & ((1ull << lane) - 1ull));
  const uint64_t mine = intro ? dict_entry_bytes((int)col.dtype, r.len) : 0ull;
  const uint64_t incl = wave_inclusive_scan(mine);
  const uint64_t bytes = (uint64_t)__shfl((unsigned long long)incl, 63, 64);
  // ---- the guard: wave-uniform ----
  bool ok = entries == T.entries && bytes == T.bytes;
  ok = ok && st.entries_before + T.entry_base + entries <= st.entries && st.entries <= (uint64_t)D.limit && st.entries <= (uint64_t)D.mask + 1u;
  ok = ok && st.body_before + T.byte_base + bytes >= st.body_before && st.body_before + T.byte_base + bytes <= st.body_bytes && st.body_bytes <= D.body_cap;
  if (!ok) {
    if (lane == 0) atomicOr((unsigned long long*)&ctrl[0], 1ull);
    return;
  }
  const uint32_t id = (uint32_t)st.entries_before + T.entry_base + rank;
  const uint64_t at = st.body_before + T.byte_base + (incl - mine);
  uint8_t* dst = D.body + at;
  if (col.dtype == T_UTF8) {
    if (intro) {
      D.slots[slot].id = id;
      D.entry_off[id] = (uint32_t)at;
      *(pqw_u32*)dst = r.len;
    }
    pqwd_copy_values(dst + 4, col.data + r.begin, r.len, intro, lane);
  } else if (intro) {
    D.slots[slot].id = id;
    const uint64_t w = pqwd_stored(col, row);
    if (stored_width((int)col.dtype) == 4) *(pqw_u32*)dst = (uint32_t)w;
    else *(pqw_u64*)dst = w;
  }
}

// one wave per tile of the columns that stayed in dictionary mode: recount, check, then the tile's share of its page's level block,
// the width byte and run header (the page's first tile), and the indices -- every store an atomicOr on a word of the zeroed buffer
__global__ __launch_bounds__(kPqwBlock) void k_pqwd_encode(const DevPqwdPlan P, const uint32_t* __restrict__ slot_of_row, const PqwdTile* __restrict__ tiles,
                                                          const PqwPage* __restrict__ pages, uint8_t* __restrict__ out, const uint64_t out_bytes,
                                                          uint64_t* __restrict__ ctrl) {
  const int lane = lane_id();
  const int64_t t = (int64_t)blockIdx.x * (kPqwBlock / 64) + (int64_t)(threadIdx.x >> 6);
  if (t >= P.base.n_tiles * P.base.n_cols) return;
  const int c = (int)(t / P.base.n_tiles);
  const int64_t tile = t % P.base.n_tiles;
  const DevPqwdCol D = P.dict[c];
  const PqwdState st = *D.state;
  if (st.mode != PQWD_MODE_DICT) return;
  const DevPqwCol col = P.base.col[c];
  const int64_t tpp = P.base.page_rows / 64;
  const int64_t p = tile / tpp, tile_in_page = tile % tpp;
  const PqwPage g = pages[(int64_t)c * P.base.n_pages + p];
  const PqwdTile T = tiles[t];
  const uint64_t n = (uint64_t)std::min<int64_t>(P.base.page_rows, P.base.rows - p * P.base.page_rows);  // rows of the page
  const int64_t row = tile * 64 + lane;
  const uint32_t tile_rows = (uint32_t)std::min<int64_t>(64, P.base.rows - tile * 64);
  const PqwRow r = pqw_row(col, row, row < P.base.rows, P.base.rows);
  const uint64_t vw = __ballot(r.valid);
  const uint32_t cnt = (uint32_t)__popcll(vw);
  const uint32_t rank = (uint32_t)__popcll(vw & ((1ull << lane) - 1ull));
  const uint32_t slot = r.valid ? slot_of_row[(int64_t)c * P.base.rows + row] : kPqwdNone;
  const uint32_t id = slot != kPqwdNone ? D.slots[slot].id : kPqwdNone;
  const uint32_t lk = g.kind & ((1u << kPqwdRunShift) - 1u), run = g.kind >> kPqwdRunShift, w = st.width;

  // ---- the guard: everything below is wave-uniform ----
  uint64_t lo = 0, hi = 0;
  const uint32_t prefix = lk == LEVELS_NONE ? 0u : level_block_prefix(lk, n, &lo, &hi);
  const uint32_t lev_bytes = (tile_rows + 7u) / 8u;  // of a mixed page's bitmap that this tile writes
  const uint64_t lev_off = (uint64_t)prefix + 8ull * (uint64_t)tile_in_page;
  bool ok = g.flags == 0u && cnt == T.non_null;
  ok = ok && lk == level_kind(col.optional != 0, n, g.non_null) && (uint64_t)g.level_bytes == level_block_bytes(lk, n);
  ok = ok && (lk == LEVELS_MIXED || cnt == (lk == LEVELS_ALL_NULL ? 0u : tile_rows));
  ok = ok && (lk != LEVELS_MIXED || lev_off + lev_bytes <= (uint64_t)g.level_bytes);
  ok = ok && (uint64_t)T.rank_base + cnt <= (uint64_t)g.non_null;
  ok = ok && (run == DICT_RUN_RLE || run == dict_run_kind(g.non_null, false)) && (run != DICT_RUN_RLE || g.non_null > 0u);
  ok = ok && w >= 1u && w <= 32u && w == dict_index_width(st.entries) && g.val_bytes == dict_value_bytes(run, w, g.non_null);
  ok = ok && __ballot(r.valid && (uint64_t)id >= st.entries) == 0ull;  // (an id of w bits: below the entries)
  // (the page's span rounded up to 8 bytes: the last word a page ORs into is the page's own and inside the buffer)
  ok = ok && body_fits(g.level_bytes, g.val_bytes) && (g.base & 7ull) == 0ull && g.base <= out_bytes &&
       (((uint64_t)g.level_bytes + g.val_bytes + 7ull) & ~7ull) <= out_bytes - g.base;
  if (!ok) {
    if (lane == 0) atomicOr((unsigned long long*)&ctrl[0], 1ull);  // mark / scan / commit and this kernel disagree: store nothing
    return;
  }
  uint32_t* out32 = (uint32_t*)out;
  if (tile_in_page == 0 && prefix) {
    pqw_or_bits(out32, g.base * 8ull, lo, lane);
    pqw_or_bits(out32, (g.base + 8ull) * 8ull, hi, lane);
  }
  if (lk == LEVELS_MIXED) pqw_or_bits(out32, (g.base + lev_off) * 8ull, vw, lane);
  const uint64_t vals = g.base + (uint64_t)g.level_bytes;  // byte of the width byte
  const uint64_t header = dict_run_header(run, g.non_null);
  const uint32_t head = 1u + (run == DICT_RUN_NONE ? 0u : varint_len(header));  // bytes before the index / the groups
  if (tile_in_page == 0) {  // the width byte and the run header's varint (at most 5 bytes: the page holds fewer than 2^31 values)
    uint64_t word = (uint64_t)w;
    if (run != DICT_RUN_NONE) {
      uint32_t k = 1;
      for (uint64_t h = header;; h >>= 7, ++k) {
        word |= (h >= 0x80 ? (h & 0x7F) | 0x80 : h) << (8u * k);
        if (h < 0x80) break;
      }
    }
    pqw_or_bits(out32, vals * 8ull, word, lane);
  }
  if (run == DICT_RUN_RLE) {  // every tile's first valid row ORs the one index: the same bits
    if (r.valid && rank == 0u) pqwd_or_value(out32, (vals + head) * 8ull, id);
  } else if (r.valid) {
    pqwd_or_value(out32, (vals + head) * 8ull + ((uint64_t)T.rank_base + rank) * w, id);
  }
}

static unsigned pqwd_grid(int64_t waves) { return (unsigned)((waves + kPqwBlock / 64 - 1) / (kPqwBlock / 64)); }

hipError_t launch_pqwd_measure(const DevPqwdPlan& plan, uint32_t* slot_of_row, PqwdTile* tiles, PqwPage* pages, hipStream_t s) {
  const DevPqwPlan& b = plan.base;
  if (b.rows <= 0 || b.n_cols <= 0) return hipSuccess;
  Scope sc(KID_PARQUET_WRITE, s, 0.0);
  hipLaunchKernelGGL(k_pqwd_insert, dim3(pqwd_grid(b.n_tiles * b.n_cols)), dim3(kPqwBlock), 0, s, plan, slot_of_row);
  hipLaunchKernelGGL(k_pqwd_mark, dim3(pqwd_grid(b.n_tiles * b.n_cols)), dim3(kPqwBlock), 0, s, plan, slot_of_row, tiles);
  hipLaunchKernelGGL(k_pqwd_decide, dim3((unsigned)b.n_cols), dim3(1024), 0, s, plan, tiles);
  hipLaunchKernelGGL(k_pqwd_scan, dim3(pqwd_grid(b.n_pages * b.n_cols)), dim3(kPqwBlock), 0, s, plan, tiles, pages);
  return hipGetLastError();
}

hipError_t launch_pqwd_encode(const DevPqwdPlan& plan, const uint32_t* slot_of_row, const PqwdTile* tiles, const PqwPage* pages, uint8_t* out,
                              uint64_t out_bytes, uint64_t* ctrl, hipStream_t s) {
  const DevPqwPlan& b = plan.base;
  if (b.rows <= 0 || b.n_cols <= 0) return hipSuccess;
  Scope sc(KID_PARQUET_WRITE, s, (double)out_bytes);
  hipLaunchKernelGGL(k_pqwd_commit, dim3(pqwd_grid(b.n_tiles * b.n_cols)), dim3(kPqwBlock), 0, s, plan, slot_of_row, tiles, ctrl);
  hipLaunchKernelGGL(k_pqwd_encode, dim3(pqwd_grid(b.n_tiles * b.n_cols)), dim3(kPqwBlock), 0, s, plan, slot_of_row, tiles, pages, out, out_bytes, ctrl);
  return hipGetLastError();
}

}  // namespace dfx
