// dfx_k_parquet.hip -- Parquet column chunks (UNCOMPRESSED, or LZ4_RAW inflated here first) -> Arrow columns on the device (deviation D12; the executor of
// DataSourceMeta::ParquetFile, src/execution/datasource.rs:87-92, which the reference declares and never runs).  The host has
// copied a chunk's bytes to HBM and walked its page HEADERS (dfx_parquet_meta.hpp: walk_chunk); the page table it uploads
// (dfx_parquet_rle.hpp: PqPage) holds, per data page, the extents of the levels and of the values, all inside the chunk.
//
// Four kernels per column, all wave64, in launch order on one stream (a kernel reads what an earlier LAUNCH wrote, never what
// another workgroup of its own launch writes):
//   k_pq_bits      one wave per page: walks the run headers of a hybrid stream at width 1 wave-uniformly and expands every run
//                  with its 64 lanes into a bitmap.  The definition levels of an optional column give the column's Arrow validity
//                  bitmap (a bit-packed run at width 1 IS bitmap bytes, an RLE run is a fill); the RLE values of a Boolean V2 page
//                  give the page's dense value bits.  A page starts at an arbitrary bit, so every word is written with an
//                  agent-scope atomicOr into a zeroed buffer: no word has two plain writers.
//   k_pq_rank      one wave per page of an optional column: per 64-row word the number of valid rows before it in its page (what
//                  gives a row its index into the page's dense values), and the page's count of non-null values.
//   k_pq_dict      one wave per dictionary-encoded page: the same run walk at the page's index width; an RLE run is a broadcast,
//                  a bit-packed run a per-lane extraction.  Writes the page's dense indices, each checked against the dictionary's
//                  size: a larger one raises PQ_ERR_DICT_INDEX and is CLAMPED to 0, so nothing is ever read outside the dictionary.
//   k_pq_plain     one lane per row of the row group: finds its page by binary search on the first rows, its rank from the word
//                  ranks, and stores the value -- read from a PLAIN page, through the decoded index from the dictionary, or from the
//                  expanded Boolean bits -- in the column's Arrow width (null slots 0; Boolean rows as one ballot word per wave;
//                  Utf8 rows as a source offset and a length, for the offset scan and the byte gather that follow).  A chunk that
//                  starts dictionary-encoded and falls back to PLAIN pages is therefore handled page by page.
//
// A compressed chunk (codec 7, LZ4_RAW) takes one kernel more, in front of the four: k_pq_inflate, at the end of this file, one wave
// per page of the chunk (dictionary page included), inflates or copies every page body into the INFLATED IMAGE, which `chunk` then
// names; the page table's extents lie inside the image (dfx_parquet_meta.hpp: walk_headers, walk_bodies).
//
// Bounds.  Every offset taken from file bytes -- a run's payload, a value's position, a dictionary index, a string's extent (the
// host walked the length chains and uploads them) -- is checked against the page's extent before it is used; a violation sets a
// PQ_ERR_* bit in the control block's CTRL_ERROR word (error_from_ctrl: DFX_PARSER_ERROR) and the slot gets 0.  Values of a page
// start at an arbitrary byte: a value is loaded in one access only where its address is aligned, byte by byte otherwise.
#include "../../include/dfx.h"
#include "dfx_k_base_inl.hpp"
#include "dfx_launch.hpp"
#include "dfx_parquet_rle.hpp"

namespace dfx {

namespace {
constexpr int kPqBlock = 256;  // 4 waves: 4 pages per workgroup in the wave-per-page kernels

DEV void pq_raise(uint32_t* ctrl, uint32_t bits) { atomicOr(ctrl + CTRL_ERROR, bits); }

DEV void pq_or_bits(uint64_t* words, uint64_t bit, uint64_t v, uint32_t nbits) {  // v: nbits <= 8 bits at `bit`
  if (v == 0) return;
  const uint32_t sh = (uint32_t)(bit & 63);
  atomicOr((unsigned long long*)(words + (bit >> 6)), (unsigned long long)(v << sh));
  if (sh + nbits > 64 && (v >> (64 - sh)) != 0)  // (masked to the page's rows: a set bit up there is a row of the buffer)
    atomicOr((unsigned long long*)(words + (bit >> 6) + 1), (unsigned long long)(v >> (64 - sh)));
}

DEV void pq_fill_bits(uint64_t* words, uint64_t begin, uint64_t end, int lane) {  // sets [begin, end)
  if (end <= begin) return;
  const uint64_t w0 = begin >> 6, w1 = (end - 1) >> 6;
  for (uint64_t w = w0 + (uint64_t)lane; w <= w1; w += 64) {
    uint64_t m = ~0ull;
    if (w == w0) m &= ~0ull << (begin & 63);
    if (w == w1 && (end & 63)) m &= (1ull << (end & 63)) - 1ull;
    atomicOr((unsigned long long*)(words + w), (unsigned long long)m);
  }
}

// the bits of 64-row word w that are rows of the page [first, first + n)
DEV uint64_t pq_page_mask(uint64_t w, uint64_t first, uint64_t n) {
  const uint64_t lo = w << 6, hi = lo + 64, b = first > lo ? first : lo, e = first + n < hi ? first + n : hi;
  if (e <= b) return 0;
  uint64_t m = ~0ull << (b - lo);
  if (e < hi) m &= (1ull << (e - lo)) - 1ull;
  return m;
}

// expands up to `want` values of the width-1 hybrid stream [s, s + len) into the bits from bit0 on; returns the values expanded
DEV uint32_t pq_expand_bits(const uint8_t* s, uint32_t len, uint32_t want, uint64_t* words, uint64_t bit0, int lane, uint32_t* ctrl,
                            uint32_t* rle_runs, uint32_t* packed_runs) {
  uint64_t pos = 0;
  uint32_t got = 0;
  while (got < want && pos < len) {
    PqRun r;
    if (!pq_read_run(s, len, pos, 1, &r)) {
      if (lane == 0) pq_raise(ctrl, PQ_ERR_RUN);
      break;
    }
    const uint32_t n = r.count < want - got ? r.count : want - got;
    if (r.packed) {
      const uint32_t nb = (n + 7) / 8;  // <= the payload's bytes: n <= 8 * groups
      for (uint32_t b = (uint32_t)lane; b < nb; b += 64) {
        uint32_t v = s[r.payload + b];
        const uint32_t rem = n - b * 8;
        if (rem < 8) v &= (1u << rem) - 1u;  // the last group's padding
        pq_or_bits(words, bit0 + got + (uint64_t)b * 8, v, 8);
      }
      ++*packed_runs;
    } else {
      if (r.value & 1) pq_fill_bits(words, bit0 + got, bit0 + got + n, lane);
      ++*rle_runs;
    }
    got += n;
    pos = r.next;
  }
  return got;
}

// mode 0: definition levels -> validity; mode 1: RLE Boolean values -> dense bits
__global__ __launch_bounds__(kPqBlock) void k_pq_bits(const DevPqColumn C, const int mode) {
  const uint32_t p = (uint32_t)((blockIdx.x * kPqBlock + threadIdx.x) >> 6);
  const int lane = (int)(threadIdx.x & 63);
  if (p >= C.n_pages) return;
  const PqPage pg = C.pages[p];
  uint32_t rle = 0, packed = 0;
  if (mode == 0) {
    if (pg.lev_len == 0) {  // no levels written: every row is there
      pq_fill_bits(C.validity, pg.first_row, (uint64_t)pg.first_row + pg.num_values, lane);
    } else {
      const uint32_t got = pq_expand_bits(C.chunk + pg.lev_off, pg.lev_len, pg.num_values, C.validity, pg.first_row, lane, C.ctrl, &rle, &packed);
      if (got != pg.num_values && lane == 0) pq_raise(C.ctrl, PQ_ERR_RUN);
    }
  } else {
    if (pg.enc != PQ_ENC_RLE_BOOL) return;
    const uint32_t got = pq_expand_bits(C.chunk + pg.val_off, pg.val_len, pg.num_values, C.dense_bits, pg.dense_base, lane, C.ctrl, &rle, &packed);
    if (lane == 0) C.page_decoded[p] = got;
  }
  if (lane == 0) {
    if (rle) atomicAdd((unsigned long long*)(C.stats + 0), (unsigned long long)rle);
    if (packed) atomicAdd((unsigned long long*)(C.stats + 1), (unsigned long long)packed);
  }
}

__global__ __launch_bounds__(kPqBlock) void k_pq_rank(const DevPqColumn C) {
  const uint32_t p = (uint32_t)((blockIdx.x * kPqBlock + threadIdx.x) >> 6);
  const int lane = (int)(threadIdx.x & 63);
  if (p >= C.n_pages) return;
  const PqPage pg = C.pages[p];
  uint32_t running = 0;
  if (pg.num_values > 0) {
    const uint64_t w0 = pg.first_row >> 6, w1 = ((uint64_t)pg.first_row + pg.num_values - 1) >> 6;
    for (uint64_t base = w0; base <= w1; base += 64) {
      const uint64_t w = base + (uint64_t)lane;
      const uint32_t cnt = w <= w1 ? (uint32_t)__popcll(C.validity[w] & pq_page_mask(w, pg.first_row, pg.num_values)) : 0u;
      uint32_t incl = cnt;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
      }
      if (w <= w1) C.word_rank[pg.rank_base + (uint32_t)(w - w0)] = running + incl - cnt;
      running += __shfl(incl, 63, 64);
    }
  }
  if (lane == 0) {
    C.page_nonnull[p] = running;
    if (running != pg.num_values) atomicAdd((unsigned long long*)(C.stats + 2), (unsigned long long)(pg.num_values - running));
  }
}

__global__ __launch_bounds__(kPqBlock) void k_pq_dict(const DevPqColumn C) {
  const uint32_t p = (uint32_t)((blockIdx.x * kPqBlock + threadIdx.x) >> 6);
  const int lane = (int)(threadIdx.x & 63);
  if (p >= C.n_pages) return;
  const PqPage pg = C.pages[p];
  if (pg.enc != PQ_ENC_DICT) return;
  const uint32_t want = C.optional ? C.page_nonnull[p] : pg.num_values;  // <= num_values: the page's share of dense_idx
  const uint8_t* s = C.chunk + pg.val_off;
  uint64_t pos = 0;
  uint32_t got = 0, rle = 0, packed = 0;
  bool bad_index = false;
  while (got < want && pos < pg.val_len) {
    PqRun r;
    if (!pq_read_run(s, pg.val_len, pos, pg.bit_width, &r)) {
      if (lane == 0) pq_raise(C.ctrl, PQ_ERR_RUN);
      break;
    }
    const uint32_t n = r.count < want - got ? r.count : want - got;
    for (uint32_t i = (uint32_t)lane; i < n; i += 64) {
      uint32_t idx = r.packed ? pq_unpack(s + r.payload, i, pg.bit_width) : r.value;
      if (idx >= C.dict_n) {
        bad_index = true;
        idx = 0;  // clamped: k_pq_plain reads entry 0 at most (and nothing when the dictionary is empty)
      }
      C.dense_idx[pg.dense_base + got + i] = idx;
    }
    if (r.packed) ++packed; else ++rle;
    got += n;
    pos = r.next;
  }
  if (bad_index) pq_raise(C.ctrl, PQ_ERR_DICT_INDEX);
  if (lane == 0) {
    C.page_decoded[p] = got;
    if (rle) atomicAdd((unsigned long long*)(C.stats + 0), (unsigned long long)rle);
    if (packed) atomicAdd((unsigned long long*)(C.stats + 1), (unsigned long long)packed);
  }
}

// `width` bytes at chunk + off (inside the chunk: the caller checked), little-endian
DEV uint64_t pq_load_value(const uint8_t* chunk, uint32_t off, uint32_t width) {
  const uint8_t* a = chunk + off;
  if (width == 8) {
    if (((uintptr_t)a & 7) == 0) return *(const uint64_t*)a;
    if (((uintptr_t)a & 3) == 0) return (uint64_t)((const uint32_t*)a)[0] | (uint64_t)((const uint32_t*)a)[1] << 32;
  } else if (((uintptr_t)a & 3) == 0) {
    return *(const uint32_t*)a;
  }
  uint64_t v = 0;
  for (uint32_t k = 0; k < width; ++k) v |= (uint64_t)a[k] << (8 * k);
  return v;
}

__global__ __launch_bounds__(kPqBlock) void k_pq_plain(const DevPqColumn C, void* __restrict__ out, int32_t* __restrict__ out_starts,
                                                       int32_t* __restrict__ out_lens) {
  const uint32_t r = blockIdx.x * kPqBlock + threadIdx.x;  // the grid covers the rows rounded up to whole waves
  const bool live = r < C.rows;
  uint64_t bits = 0;
  uint32_t start = 0, len = 0;
  if (live) {
    uint32_t lo = 0, hi = C.n_pages - 1;  // the last page whose first row is <= r
    while (lo < hi) {
      const uint32_t mid = (lo + hi + 1) >> 1;
      if (C.pages[mid].first_row <= r) lo = mid; else hi = mid - 1;
    }
    const PqPage pg = C.pages[lo];
    bool valid = r - pg.first_row < pg.num_values;
    uint32_t rank = r - pg.first_row;
    if (valid && C.optional) {
      const uint64_t word = C.validity[r >> 6];
      valid = (word >> (r & 63)) & 1;
      rank = C.word_rank[pg.rank_base + ((r >> 6) - (pg.first_row >> 6))] +
             (uint32_t)__popcll(word & pq_page_mask(r >> 6, pg.first_row, pg.num_values) & ((1ull << (r & 63)) - 1ull));
    }
    if (valid) {
      bool ok = true;
      const bool utf8 = C.dtype == DFX_UTF8, boolean = C.dtype == DFX_BOOLEAN;
      if (pg.enc == PQ_ENC_PLAIN) {
        if (utf8) {
          ok = rank < pg.pad;
          if (ok) {
            const uint32_t a = C.str_offs[pg.str_base + rank], b = C.str_offs[pg.str_base + rank + 1];
            start = a + 4;
            len = b - a - 4;
          }
        } else if (boolean) {
          ok = (uint64_t)rank < (uint64_t)pg.val_len * 8;
          if (ok) bits = (C.chunk[pg.val_off + (rank >> 3)] >> (rank & 7)) & 1;
        } else {
          ok = ((uint64_t)rank + 1) * C.width <= pg.val_len;
          if (ok) bits = pq_load_value(C.chunk, pg.val_off + rank * C.width, C.width);
        }
      } else if (pg.enc == PQ_ENC_RLE_BOOL) {
        ok = rank < C.page_decoded[lo];
        if (ok) bits = (C.dense_bits[((uint64_t)pg.dense_base + rank) >> 6] >> (((uint64_t)pg.dense_base + rank) & 63)) & 1;
      } else {
        ok = rank < C.page_decoded[lo] && C.dict_n > 0;
        if (ok) {
          const uint32_t idx = C.dense_idx[pg.dense_base + rank];  // < dict_n: k_pq_dict clamped it
          if (utf8) {
            const uint32_t a = C.dict_str[idx], b = C.dict_str[idx + 1];
            start = a + 4;
            len = b - a - 4;
          } else {
            bits = pq_load_value(C.chunk, C.dict_off + idx * C.width, C.width);
          }
        }
      }
      if (!ok) pq_raise(C.ctrl, PQ_ERR_VALUE);
    }
  }
  switch (C.dtype) {
    case DFX_BOOLEAN: {
      const uint64_t word = __ballot(live && (bits & 1));
      if ((threadIdx.x & 63) == 0 && live) ((uint64_t*)out)[r >> 6] = word;
      break;
    }
    case DFX_UTF8: {
      if (live) {
        out_starts[r] = (int32_t)start;
        out_lens[r] = (int32_t)len;
      }
      // the column's bytes, summed in 64 bits (a dictionary string may be referenced by any number of rows: the sum is not bounded
      // by the chunk): the host refuses a total beyond Arrow's 32-bit offsets BEFORE it scans the lengths, allocates and gathers
      unsigned long long sum = len;
#pragma unroll
      for (int d = 32; d > 0; d >>= 1) sum += __shfl_down(sum, d, 64);
      if ((threadIdx.x & 63) == 0 && sum) atomicAdd((unsigned long long*)(C.stats + 3), sum);
      break;
    }
    case DFX_INT8:
    case DFX_UINT8:
      if (live) ((uint8_t*)out)[r] = (uint8_t)bits;
      break;
    case DFX_INT16:
    case DFX_UINT16:
      if (live) ((uint16_t*)out)[r] = (uint16_t)bits;
      break;
    case DFX_INT32:
    case DFX_UINT32:
    case DFX_FLOAT32:
      if (live) ((uint32_t*)out)[r] = (uint32_t)bits;
      break;
    default:
      if (live) ((uint64_t*)out)[r] = bits;
  }
}

}  // namespace

hipError_t launch_pq_decode(const DevPqColumn& C, bool has_rle_bool, bool has_dict, void* out, int32_t* out_starts, int32_t* out_lens,
                            double algo_bytes, hipStream_t s) {
  if (C.rows == 0 || C.n_pages == 0) return hipSuccess;
  Scope sc(KID_PARQUET, s, algo_bytes);
  const int page_grid = (int)(((uint64_t)C.n_pages * 64 + kPqBlock - 1) / kPqBlock);
  if (C.optional) {
    hipLaunchKernelGGL(k_pq_bits, dim3(page_grid), dim3(kPqBlock), 0, s, C, 0);
    hipLaunchKernelGGL(k_pq_rank, dim3(page_grid), dim3(kPqBlock), 0, s, C);
  }
  if (has_rle_bool) hipLaunchKernelGGL(k_pq_bits, dim3(page_grid), dim3(kPqBlock), 0, s, C, 1);
  if (has_dict) hipLaunchKernelGGL(k_pq_dict, dim3(page_grid), dim3(kPqBlock), 0, s, C);
  const int row_grid = (int)(((uint64_t)C.rows + kPqBlock - 1) / kPqBlock);
  hipLaunchKernelGGL(k_pq_plain, dim3(row_grid), dim3(kPqBlock), 0, s, C, out, out_starts, out_lens);
  return hipGetLastError();
}

// ---- the inflate stage ------------------------------------------------------------------------------------------------------------
namespace {

// Stores of earlier sequences -> loads of this match, between lanes of ONE wave.  The wave's stores are drained (vmcnt counts
// stores on gfx9) inside a workgroup-scope release / acquire pair: the lanes of a wave share their CU's L1, which is written
// through and holds no stale copy of a line this CU stored to once the store has completed, so no cache needs invalidating; the
// fences keep the compiler from moving the stores below or the loads above the wait.  (The wait is spelled out in asm as well:
// the compiler may drop a fence's own wait where it believes the counter empty.)
DEV void pq_stores_visible_to_wave() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// One wave per page.  The sequences are parsed wave-uniformly (every lane runs lz4_next_sequence over the same bytes: the block is
// read-only here); the copies are spread over the 64 lanes.  All extents of a sequence were checked by the parser before a byte of
// it moves, against the page's extents the host checked against the chunk and the image: nothing is read or stored outside either.
__global__ __launch_bounds__(kPqBlock) void k_pq_inflate(const DevPqInflate I) {
  const uint32_t p = (uint32_t)((blockIdx.x * kPqBlock + threadIdx.x) >> 6);
  const uint32_t lane = threadIdx.x & 63u;
  if (p >= I.n_pages) return;
  const PqInflatePage pg = I.pages[p];
  const uint8_t* body = I.chunk + pg.src_off;
  uint8_t* page = I.image + pg.dst_off;
  for (uint32_t i = lane; i < pg.prefix_len; i += 64) page[i] = body[i];  // V2: the levels are never compressed
  const uint8_t* src = body + pg.prefix_len;
  uint8_t* out = page + pg.prefix_len;
  const uint32_t src_len = pg.src_len - pg.prefix_len, out_len = pg.dst_len - pg.prefix_len;
  uint32_t sequences = 0;
  if (!(pg.flags & PQ_INFLATE_COMPRESSED)) {
    for (uint32_t i = lane; i < out_len; i += 64) out[i] = src[i];  // a stored page (out_len == src_len: the header pass)
  } else if (src_len != 0 || out_len != 0) {
    uint64_t pos = 0, produced = 0;
    for (;;) {
      Lz4Seq q;
      if (!lz4_next_sequence(src, src_len, pos, produced, out_len, &q)) {
        if (lane == 0) pq_raise(I.ctrl, PQ_ERR_INFLATE);  // the page's remainder stays zero
        break;
      }
      ++sequences;
      for (uint32_t i = lane; i < q.lit_len; i += 64) out[produced + i] = src[q.lit_pos + i];
      produced += q.lit_len;
      if (q.last) break;
      // byte i of the match is byte (i mod offset) of the `offset` bytes before it: only bytes produced before the match began are
      // read, so an overlapping match (offset 1 included) has no dependence between the lanes of one copy
      pq_stores_visible_to_wave();
      const uint8_t* from = out + (produced - q.offset);
      for (uint32_t i = lane; i < q.match_len; i += 64) out[produced + i] = from[i % q.offset];
      produced += q.match_len;
      pos = q.next;
    }
  }
  // the page's prologue: lanes 0-3 load the bytes of the word at body offset 0, lanes 4-7 those of the word at the probe offset
  pq_stores_visible_to_wave();
  uint32_t mine = (lane < 4 && lane < pg.dst_len) ? (uint32_t)page[lane] << (8 * lane) : 0u;
  uint32_t word0 = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) word0 |= __shfl(mine, k, 64);
  const uint64_t at = pq_probe_offset(pg, word0) + (lane & 3u);
  mine = (lane >= 4 && lane < 8 && at < pg.dst_len) ? (uint32_t)page[at] << (8 * (lane & 3u)) : 0u;
  uint32_t probe = 0;
#pragma unroll
  for (int k = 4; k < 8; ++k) probe |= __shfl(mine, k, 64);
  if (lane == 0) {
    I.prologues[p].word0 = word0;
    I.prologues[p].probe = probe;
    if (sequences) atomicAdd((unsigned long long*)I.stats, (unsigned long long)sequences);
  }
}

}  // namespace

hipError_t launch_pq_inflate(const DevPqInflate& I, double image_bytes, hipStream_t s) {
  if (I.n_pages == 0) return hipSuccess;
  Scope sc(KID_PARQUET_INFLATE, s, image_bytes);
  const int page_grid = (int)(((uint64_t)I.n_pages * 64 + kPqBlock - 1) / kPqBlock);
  hipLaunchKernelGGL(k_pq_inflate, dim3(page_grid), dim3(kPqBlock), 0, s, I);
  return hipGetLastError();
}

}  // namespace dfx
