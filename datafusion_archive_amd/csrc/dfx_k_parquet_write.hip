// dfx_k_parquet_write.hip -- Arrow columns -> Parquet page bodies on the device (deviation D13; the executor of PhysicalPlan::Write,
// src/execution/physicalplan.rs:24-29, which the reference declares and never runs; kind = Parquet).  The unit of work is the tile of
// 64 rows, a wave each, as in dfx_k_csvwrite.hip: measure -> scan -> encode.  Every size comes from dfx_parquet_enc.hpp, the rules
// the host encoder restates sequentially.
//
// Bounds.  Utf8 rows are clamped into [offsets[0], offsets[rows]) of the launch before a byte is read.  The encode kernel stores a
// tile only after it has found its own recount (valid rows, Utf8 bytes) equal to what the scan was given, its span inside its page's
// blocks and the page inside the buffer; otherwise it stores nothing and raises ctrl bit 0.
//
// Shared words.  The dense bits of a Boolean page are shared between tiles that may run on XCDs whose L2s are not coherent: two tiles
// can own bits of one word.  In a BOOLEAN column EVERY store -- level prefix, level bitmap, value bits -- is therefore an agent-scope
// atomicOr on an aligned 32-bit word of the page's own span in a zeroed buffer (what k_pq_bits does for the same reason); a word that
// would receive no bit is not touched.  Pages start 8-byte aligned, so no word belongs to two pages.  In every other column tiles
// write disjoint BYTES with plain stores.  No LDS, no workgroup barrier outside the bases kernel.
#include <algorithm>

#include "dfx_k_parquet_write_inl.hpp"
#include "dfx_launch.hpp"

namespace dfx {

using namespace pqw;

// one wave per tile of every column: the tile's valid rows and, for Utf8, the bytes its values take
__global__ __launch_bounds__(kPqwBlock) void k_pqw_measure(const DevPqwPlan P, PqwTile* __restrict__ tiles) {
  const int lane = lane_id();
  const int64_t t = (int64_t)blockIdx.x * (kPqwBlock / 64) + (int64_t)(threadIdx.x >> 6);
  if (t >= P.n_tiles * P.n_cols) return;
  const int c = (int)(t / P.n_tiles);
  const int64_t tile = t % P.n_tiles;
  const DevPqwCol col = P.col[c];
  const int64_t row = tile * 64 + lane;
  const PqwRow r = pqw_row(col, row, row < P.rows, P.rows);
  const uint32_t cnt = (uint32_t)__popcll(__ballot(r.valid));
  uint64_t bytes = 0;
  if (col.dtype == T_UTF8) bytes = pqw_wave_sum(r.valid ? 4ull + r.len : 0ull);
  if (lane == 0) {
    tiles[t].non_null = cnt;
    tiles[t].bytes = bytes;
  }
}

// one wave per page: the exclusive prefix of every tile inside its page, the page's sums, level-run kind and sizes
__global__ __launch_bounds__(kPqwBlock) void k_pqw_scan(const DevPqwPlan P, PqwTile* __restrict__ tiles, PqwPage* __restrict__ pages) {
  const int lane = lane_id();
  const int64_t pg = (int64_t)blockIdx.x * (kPqwBlock / 64) + (int64_t)(threadIdx.x >> 6);
  if (pg >= P.n_pages * P.n_cols) return;
  const int c = (int)(pg / P.n_pages);
  const int64_t p = pg % P.n_pages;
  const int64_t tpp = P.page_rows / 64;
  const int64_t first = p * tpp;
  const int64_t count = std::min<int64_t>(tpp, P.n_tiles - first);
  const uint64_t n = (uint64_t)std::min<int64_t>(P.page_rows, P.rows - p * P.page_rows);
  PqwTile* tp = tiles + (int64_t)c * P.n_tiles + first;
  uint64_t run_cnt = 0, run_bytes = 0;
  for (int64_t k = 0; k < count; k += 64) {
    const bool live = k + lane < count;
    const uint64_t cnt = live ? tp[k + lane].non_null : 0ull;
    const uint64_t by = live ? tp[k + lane].bytes : 0ull;
    const uint64_t icnt = wave_inclusive_scan(cnt), iby = wave_inclusive_scan(by);
    if (live) {
      tp[k + lane].rank_base = (uint32_t)(run_cnt + icnt - cnt);
      tp[k + lane].byte_base = run_bytes + iby - by;
    }
    run_cnt += (uint64_t)__shfl((unsigned long long)icnt, 63, 64);
    run_bytes += (uint64_t)__shfl((unsigned long long)iby, 63, 64);
  }
  if (lane == 0) {
    const DevPqwCol col = P.col[c];
    PqwPage g;
    g.base = 0;
    g.kind = level_kind(col.optional != 0, n, run_cnt);
    g.level_bytes = (uint32_t)level_block_bytes(g.kind, n);
    g.val_bytes = value_bytes((int)col.dtype, run_cnt, run_bytes);
    g.non_null = (uint32_t)run_cnt;
    g.flags = body_fits(g.level_bytes, g.val_bytes) ? 0u : PQW_PAGE_TOO_LARGE;
    pages[pg] = g;
  }
}

// exclusive scan of the page bodies (each rounded up to 8 bytes) into 64-bit bases, pages[n].base = the buffer's length: one workgroup
__global__ __launch_bounds__(1024) void k_pqw_bases(PqwPage* __restrict__ pages, const int64_t n) {
  __shared__ uint64_t sums[1024];
  const int t = (int)threadIdx.x;
  const int64_t chunk = (n + 1023) / 1024;
  const int64_t b = std::min<int64_t>((int64_t)t * chunk, n), e = std::min<int64_t>(b + chunk, n);
  auto room = [&](int64_t i) { return pages[i].flags ? 0ull : ((uint64_t)pages[i].level_bytes + pages[i].val_bytes + 7ull) & ~7ull; };
  uint64_t s = 0;
  for (int64_t i = b; i < e; ++i) s += room(i);
  sums[t] = s;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const uint64_t v = t >= d ? sums[t - d] : 0ull;
    __syncthreads();
    sums[t] += v;
    __syncthreads();
  }
  uint64_t run = sums[t] - s;
  for (int64_t i = b; i < e; ++i) {
    pages[i].base = run;
    run += room(i);
  }
  if (t == 1023) pages[n].base = sums[1023];
}

// one wave per tile of every column: recount, check, then the tile's share of its page's level block and value block
__global__ __launch_bounds__(kPqwBlock) void k_pqw_encode(const DevPqwPlan P, const PqwTile* __restrict__ tiles, const PqwPage* __restrict__ pages,
                                                         uint8_t* __restrict__ out, const uint64_t out_bytes, uint64_t* __restrict__ ctrl) {
  const int lane = lane_id();
  const int64_t t = (int64_t)blockIdx.x * (kPqwBlock / 64) + (int64_t)(threadIdx.x >> 6);
  if (t >= P.n_tiles * P.n_cols) return;
  const int c = (int)(t / P.n_tiles);
  const int64_t tile = t % P.n_tiles;
  const DevPqwCol col = P.col[c];
  const int64_t tpp = P.page_rows / 64;
  const int64_t p = tile / tpp, tile_in_page = tile % tpp;
  const PqwPage g = pages[(int64_t)c * P.n_pages + p];
  const PqwTile T = tiles[t];
  const uint64_t n = (uint64_t)std::min<int64_t>(P.page_rows, P.rows - p * P.page_rows);  // rows of the page
  const int64_t row = tile * 64 + lane;
  const uint32_t tile_rows = (uint32_t)std::min<int64_t>(64, P.rows - tile * 64);
  const PqwRow r = pqw_row(col, row, row < P.rows, P.rows);
  const uint64_t vw = __ballot(r.valid);
  const uint32_t cnt = (uint32_t)__popcll(vw);
  const uint32_t rank = (uint32_t)__popcll(vw & ((1ull << lane) - 1ull));
  const bool utf8 = col.dtype == T_UTF8, boolean = col.dtype == T_BOOL;
  const uint64_t mine = utf8 && r.valid ? 4ull + r.len : 0ull;
  const uint64_t incl = utf8 ? wave_inclusive_scan(mine) : 0ull;
  const uint64_t bytes = (uint64_t)__shfl((unsigned long long)incl, 63, 64);
  const uint32_t sw = stored_width((int)col.dtype);

  // ---- the guard: everything below is wave-uniform ----
  uint64_t lo = 0, hi = 0;
  const uint32_t prefix = g.kind == LEVELS_NONE ? 0u : level_block_prefix(g.kind, n, &lo, &hi);
  const uint32_t lev_bytes = (tile_rows + 7u) / 8u;  // of a mixed page's bitmap that this tile writes
  const uint64_t lev_off = (uint64_t)prefix + 8ull * (uint64_t)tile_in_page;
  bool ok = g.flags == 0u && cnt == T.non_null && bytes == T.bytes;
  ok = ok && g.kind == level_kind(col.optional != 0, n, g.non_null) && (uint64_t)g.level_bytes == level_block_bytes(g.kind, n);
  ok = ok && (g.kind == LEVELS_MIXED || cnt == (g.kind == LEVELS_ALL_NULL ? 0u : tile_rows));
  ok = ok && (g.kind != LEVELS_MIXED || lev_off + lev_bytes <= (uint64_t)g.level_bytes);
  ok = ok && (uint64_t)T.rank_base + cnt <= (uint64_t)g.non_null;
  if (utf8) ok = ok && T.byte_base + bytes >= T.byte_base && T.byte_base + bytes <= g.val_bytes;
  else ok = ok && g.val_bytes == value_bytes((int)col.dtype, g.non_null, 0);
  // (the page's span rounded up to 8 bytes: the last word a Boolean page ORs into is the page's own and inside the buffer)
  ok = ok && body_fits(g.level_bytes, g.val_bytes) && (g.base & 7ull) == 0ull && g.base <= out_bytes &&
       (((uint64_t)g.level_bytes + g.val_bytes + 7ull) & ~7ull) <= out_bytes - g.base;
  if (!ok) {
    if (lane == 0) atomicOr((unsigned long long*)&ctrl[0], 1ull);  // measure / scan and this kernel disagree: store nothing
    return;
  }
  uint8_t* body = out + g.base;
  uint8_t* vals = body + g.level_bytes;

  if (boolean) {  // every store an atomicOr on an aligned word of the zeroed buffer
    uint32_t* out32 = (uint32_t*)out;
    if (tile_in_page == 0 && prefix) {
      pqw_or_bits(out32, g.base * 8ull, lo, lane);
      pqw_or_bits(out32, (g.base + 8ull) * 8ull, hi, lane);
    }
    if (g.kind == LEVELS_MIXED) pqw_or_bits(out32, (g.base + lev_off) * 8ull, vw, lane);
    const bool bit = r.valid && get_bit((const uint8_t*)col.values, col.bit_offset + row);
    const uint64_t dense = pqw_wave_or(bit ? 1ull << rank : 0ull);
    pqw_or_bits(out32, (g.base + (uint64_t)g.level_bytes) * 8ull + (uint64_t)T.rank_base, dense, lane);
    return;
  }

  if (tile_in_page == 0 && (uint32_t)lane < prefix) body[lane] = (uint8_t)(lane < 8 ? lo >> (8 * lane) : hi >> (8 * (lane - 8)));
  if (g.kind == LEVELS_MIXED && (uint32_t)lane < lev_bytes) body[lev_off + (uint64_t)lane] = (uint8_t)(vw >> (8 * lane));

  if (!utf8) {
    if (r.valid) {
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
      const uint64_t w = widen((int)col.dtype, raw);
      uint8_t* dst = vals + ((uint64_t)T.rank_base + rank) * sw;
      if (sw == 4) *(pqw_u32*)dst = (uint32_t)w;
      else *(pqw_u64*)dst = w;
    }
    return;
  }

  // Utf8: {u32 length}{bytes}; a lane per short value, the wave on every value longer than kLongValue
  uint8_t* dst = vals + T.byte_base + (incl - mine);
  const bool is_long = r.valid && r.len > kLongValue;
  if (r.valid) {
    *(pqw_u32*)dst = r.len;
    if (!is_long)
      for (uint32_t i = 0; i < r.len; ++i) dst[4 + i] = col.data[r.begin + i];
  }
  uint64_t todo = __ballot(is_long);
  while (todo) {
    const int src = (int)__builtin_ctzll(todo);
    todo &= todo - 1ull;
    const int64_t sb = (int64_t)__shfl((long long)r.begin, src, 64);
    const uint32_t sl = (uint32_t)__shfl((int)r.len, src, 64);
    const uint64_t so = (uint64_t)__shfl((unsigned long long)(incl - mine), src, 64);
    uint8_t* d = vals + T.byte_base + so + 4;
    for (uint32_t i = (uint32_t)lane; i < sl; i += 64u) d[i] = col.data[sb + i];
  }
}

static unsigned pqw_grid(int64_t waves) { return (unsigned)((waves + kPqwBlock / 64 - 1) / (kPqwBlock / 64)); }

hipError_t launch_pqw_measure(const DevPqwPlan& plan, PqwTile* tiles, hipStream_t s) {
  if (plan.rows <= 0 || plan.n_cols <= 0) return hipSuccess;
  Scope sc(KID_PARQUET_WRITE, s, 0.0);
  hipLaunchKernelGGL(k_pqw_measure, dim3(pqw_grid(plan.n_tiles * plan.n_cols)), dim3(kPqwBlock), 0, s, plan, tiles);
  return hipGetLastError();
}

hipError_t launch_pqw_scan(const DevPqwPlan& plan, PqwTile* tiles, PqwPage* pages, hipStream_t s) {
  if (plan.rows <= 0 || plan.n_cols <= 0) return hipSuccess;
  Scope sc(KID_PARQUET_WRITE, s, 0.0);
  hipLaunchKernelGGL(k_pqw_scan, dim3(pqw_grid(plan.n_pages * plan.n_cols)), dim3(kPqwBlock), 0, s, plan, tiles, pages);
  hipLaunchKernelGGL(k_pqw_bases, dim3(1), dim3(1024), 0, s, pages, plan.n_pages * plan.n_cols);
  return hipGetLastError();
}

hipError_t launch_pqw_bases(pqw::PqwPage* pages, int64_t n, hipStream_t s) {
  Scope sc(KID_PARQUET_WRITE, s, 0.0);
  hipLaunchKernelGGL(k_pqw_bases, dim3(1), dim3(1024), 0, s, pages, n);
  return hipGetLastError();
}

hipError_t launch_pqw_encode(const DevPqwPlan& plan, const PqwTile* tiles, const PqwPage* pages, uint8_t* out, uint64_t out_bytes, uint64_t* ctrl,
                             hipStream_t s) {
  if (plan.rows <= 0 || plan.n_cols <= 0) return hipSuccess;
  Scope sc(KID_PARQUET_WRITE, s, (double)out_bytes);
  hipLaunchKernelGGL(k_pqw_encode, dim3(pqw_grid(plan.n_tiles * plan.n_cols)), dim3(kPqwBlock), 0, s, plan, tiles, pages, out, out_bytes, ctrl);
  return hipGetLastError();
}

}  // namespace dfx
