// dfx_k_parquet_write_lz4.hip -- the Parquet writer's "compression" option (deviation D13): page bodies that an
// earlier launch encoded are packed into raw LZ4 blocks (Parquet codec 7, LZ4_RAW) before they leave the device.  gfx950, wave64.
//
//   k_pqw_lz4          one wave per page, the rule of dfx_parquet_lz4_enc.hpp: 64 positions per step, the hash table (16 KB) in LDS.
//                      The block goes into the page's own slot of lz4_bound(len) bytes; the wave leaves its size and sequence count.
//   k_pqw_lz4_bases    the sizes scanned into 8-byte-aligned bases (one workgroup, as k_pqw_bases)
//   k_pqw_lz4_compact  every block copied from its slot to its base: what the host copies is the compressed total and nothing else
//
// The block is the sequential host encoder's (lz4_encode_block), byte for byte: every position of a step reads the table as it stood
// before the step (the wave's lookups are complete before its first insert: the ballot over their results stands between them), and
// the inserts are LDS atomic maxima, so the table does not depend on which lane wins a same-address store.
//
// Bounds.  A wave reads [src, src + len) only -- a position's word where p <= len - 12, a match byte where s + k < len - 5 -- and
// stores into its slot only: before a sequence stores anything its whole span is checked against the slot; on overrun the wave stores
// nothing more and raises ctrl bit 1, as it does for a slot that lies outside the buffer.  The kernels read only bytes an earlier
// launch wrote; no lane waits for another lane's global store.
#include <algorithm>

#include "dfx_k_base_inl.hpp"
#include "dfx_launch.hpp"
#include "dfx_parquet_write.hpp"

namespace dfx {

using namespace pqw;

namespace {

typedef uint32_t lz4_u32 __attribute__((aligned(1)));  // a position's word sits at any byte of a body

// bytes [from, from + n) -> [to, to + n), a byte per lane and trip
DEV void lz4_copy(uint8_t* __restrict__ to, const uint8_t* __restrict__ from, uint64_t n, int lane) {
#pragma unroll 4
  for (uint64_t k = (uint64_t)lane; k < n; k += 64) to[k] = from[k];
}
// the extension chain of a length spread over the wave
DEV void lz4_put_ext(uint8_t* to, uint64_t v, int lane) {
  const uint32_t n = lz4_ext_bytes(v);
  for (uint32_t k = (uint32_t)lane; k < n; k += 64) to[k] = lz4_ext_byte(v, k);
}
// one sequence at to[0 ...]: the wave stores lz4_sequence_bytes(lit, match_len) bytes (match_len 0: the last sequence)
DEV void lz4_store_sequence(uint8_t* to, const uint8_t* lits, uint64_t lit, uint32_t offset, uint64_t match_len, int lane) {
  const uint64_t ml = match_len ? match_len - 4 : 0;
  const uint32_t le = lz4_ext_bytes(lit);
  if (lane == 0) to[0] = (uint8_t)((lit < 15 ? lit : 15) << 4 | (ml < 15 ? ml : 15));
  lz4_put_ext(to + 1, lit, lane);
  lz4_copy(to + 1 + le, lits, lit, lane);
  if (match_len) {
    uint8_t* m = to + 1 + le + lit;
    if (lane < 2) m[lane] = (uint8_t)(offset >> (8 * lane));
    lz4_put_ext(m + 2, ml, lane);
  }
}

}  // namespace

__global__ __launch_bounds__(64) void k_pqw_lz4(const PqwLz4In* __restrict__ in, const int64_t n_pages, uint8_t* __restrict__ slots, const uint64_t slots_bytes,
                                                PqwLz4Out* __restrict__ out, uint64_t* __restrict__ ctrl) {
  __shared__ uint32_t table[kLz4TableEntries];
  const int lane = lane_id();
  const int64_t pg = (int64_t)blockIdx.x;
  if (pg >= n_pages) return;
  const PqwLz4In e = in[pg];
  const uint8_t* __restrict__ src = e.src;
  const uint64_t n = e.len;
  const uint64_t cap = lz4_bound(n);
  // the slot: where the host put it, 8-byte aligned, inside the buffer
  if ((e.slot_off & 7ull) != 0ull || e.slot_off > slots_bytes || cap > slots_bytes - e.slot_off || !lz4_body_fits(n)) {
    if (lane == 0) {
      atomicOr((unsigned long long*)&ctrl[0], 2ull);
      out[pg].bytes = 0;
      out[pg].sequences = 0;
    }
    return;
  }
  uint8_t* dst = slots + e.slot_off;
  for (uint32_t k = (uint32_t)lane; k < kLz4TableEntries; k += 64) table[k] = 0u;
  __syncthreads();

  uint64_t anchor = 0, op = 0;
  uint32_t sequences = 0;
  bool overrun = false;
  if (n >= kLz4MinInput) {
    const uint64_t last = n - kLz4LastMatch;
    uint64_t cur = 0;
    while (cur <= last) {
      const uint64_t p = cur + (uint64_t)lane;
      const bool live = p <= last;
      const uint32_t word = live ? *(const lz4_u32*)(src + p) : 0u;
      const uint32_t h = lz4_hash(word);
      const uint32_t entry = live ? table[h] : 0u;
      const uint64_t ref = (uint64_t)entry - 1ull;
      const bool in_window = live && entry != 0u && ref < p && p - ref <= (uint64_t)kLz4MaxOffset;
      const bool holds = in_window && *(const lz4_u32*)(src + ref) == word;
      const uint64_t held = __ballot(holds);
      const int pick = held ? (int)__builtin_ctzll(held) : 64;
      __syncthreads();  // (one wave: every lookup of the step is done before its first insert)
      if (live && lane <= pick) atomicMax(&table[h], (uint32_t)(p + 1ull));
      __syncthreads();
      if (pick == 64) {
        cur += kLz4Step;
        continue;
      }
      const uint64_t s = cur + (uint64_t)pick;
      const uint64_t r = (uint64_t)__shfl((unsigned long long)ref, pick, 64);
      const uint64_t stop = n - kLz4LastLiterals;  // the match ends here or before
      uint64_t len = 4;
      for (;;) {
        const uint64_t q = s + len + (uint64_t)lane;
        const bool equal = q < stop && src[r + len + (uint64_t)lane] == src[q];
        const uint64_t differs = __ballot(!equal);
        if (differs) {
          len += (uint64_t)__builtin_ctzll(differs);
          break;
        }
        len += 64;
      }
      const uint64_t lit = s - anchor;
      const uint64_t size = lz4_sequence_bytes(lit, len);
      if (size > cap - op) {  // the guard: nothing of the sequence is stored
        overrun = true;
        break;
      }
      lz4_store_sequence(dst + op, src + anchor, lit, (uint32_t)(s - r), len, lane);
      op += size;
      ++sequences;
      anchor = cur = s + len;
    }
  }
  if (!overrun) {
    const uint64_t lit = n - anchor;
    const uint64_t size = lz4_sequence_bytes(lit, 0);
    if (size > cap - op) {
      overrun = true;
    } else {
      lz4_store_sequence(dst + op, src + anchor, lit, 0u, 0, lane);
      op += size;
      ++sequences;
    }
  }
  if (lane == 0) {
    if (overrun) atomicOr((unsigned long long*)&ctrl[0], 2ull);
    out[pg].bytes = overrun ? 0u : (uint32_t)op;
    out[pg].sequences = overrun ? 0u : sequences;
  }
}

// exclusive scan of the block sizes (each rounded up to 8 bytes) into 64-bit bases, out[n].base = the compact buffer's length
__global__ __launch_bounds__(1024) void k_pqw_lz4_bases(PqwLz4Out* __restrict__ out, const int64_t n) {
  __shared__ uint64_t sums[1024];
  const int t = (int)threadIdx.x;
  const int64_t chunk = (n + 1023) / 1024;
  const int64_t b = std::min<int64_t>((int64_t)t * chunk, n), e = std::min<int64_t>(b + chunk, n);
  auto room = [&](int64_t i) { return ((uint64_t)out[i].bytes + 7ull) & ~7ull; };
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
    out[i].base = run;
    run += room(i);
  }
  if (t == 1023) {
    out[n].base = sums[1023];
    out[n].bytes = 0;
    out[n].sequences = 0;
  }
}

constexpr int kLz4CompactSplit = 4;  // workgroups that share one block's copy

// every block from its slot to its base, 8 bytes per lane and trip (slots and bases are 8-byte aligned), the tail by bytes
__global__ __launch_bounds__(256) void k_pqw_lz4_compact(const PqwLz4In* __restrict__ in, const PqwLz4Out* __restrict__ out, const int64_t n_pages,
                                                        const uint8_t* __restrict__ slots, const uint64_t slots_bytes, uint8_t* __restrict__ packed,
                                                        const uint64_t packed_bytes, uint64_t* __restrict__ ctrl) {
  const int64_t pg = (int64_t)blockIdx.x;
  if (pg >= n_pages) return;
  const PqwLz4In e = in[pg];
  const PqwLz4Out o = out[pg];
  const uint64_t bytes = o.bytes;
  if ((e.slot_off & 7ull) != 0ull || e.slot_off > slots_bytes || bytes > slots_bytes - e.slot_off || bytes > lz4_bound(e.len) || (o.base & 7ull) != 0ull ||
      o.base > packed_bytes || bytes > packed_bytes - o.base) {
    if (threadIdx.x == 0 && blockIdx.y == 0) atomicOr((unsigned long long*)&ctrl[0], 2ull);
    return;
  }
  const uint8_t* from = slots + e.slot_off;
  uint8_t* to = packed + o.base;
  const uint64_t words = bytes / 8;
  const uint64_t t = (uint64_t)blockIdx.y * 256ull + (uint64_t)threadIdx.x;
  for (uint64_t k = t; k < words; k += 256ull * kLz4CompactSplit) ((uint64_t*)to)[k] = ((const uint64_t*)from)[k];
  if (blockIdx.y == 0 && (uint64_t)threadIdx.x < bytes - words * 8) to[words * 8 + threadIdx.x] = from[words * 8 + threadIdx.x];
}

hipError_t launch_pqw_lz4(const PqwLz4In* in, int64_t n_pages, uint8_t* slots, uint64_t slots_bytes, PqwLz4Out* out, uint64_t* ctrl, hipStream_t s) {
  if (n_pages <= 0) return hipSuccess;
  Scope sc(KID_PARQUET_WRITE_LZ4, s, 0.0);
  hipLaunchKernelGGL(k_pqw_lz4, dim3((unsigned)n_pages), dim3(64), 0, s, in, n_pages, slots, slots_bytes, out, ctrl);
  hipLaunchKernelGGL(k_pqw_lz4_bases, dim3(1), dim3(1024), 0, s, out, n_pages);
  return hipGetLastError();
}

hipError_t launch_pqw_lz4_compact(const PqwLz4In* in, const PqwLz4Out* out, int64_t n_pages, const uint8_t* slots, uint64_t slots_bytes, uint8_t* packed,
                                  uint64_t packed_bytes, uint64_t* ctrl, hipStream_t s) {
  if (n_pages <= 0) return hipSuccess;
  Scope sc(KID_PARQUET_WRITE_LZ4, s, (double)packed_bytes);
  hipLaunchKernelGGL(k_pqw_lz4_compact, dim3((unsigned)n_pages, kLz4CompactSplit), dim3(256), 0, s, in, out, n_pages, slots, slots_bytes, packed, packed_bytes, ctrl);
  return hipGetLastError();
}

}  // namespace dfx
