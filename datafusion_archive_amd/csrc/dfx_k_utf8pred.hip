// dfx_k_utf8pred.hip -- Utf8 string terms on the device (deviation D9): `Utf8 column <op> Utf8 literal` for the six
// comparisons and LIKE / NOT LIKE, one term over one batch into an Arrow LSB bitmap.  The operators bind that bitmap to the
// fused programs as a virtual Boolean column (dfx_expr_utf8.cpp: Utf8Terms), the way a Utf8 GROUP BY key reaches them as a
// virtual id column; a predicate that is one term uses the bitmap as the filter's mask directly.
//
// Shape (the one k_csv_parse settled on): one wave owns a tile of 64 rows and its ballot is the tile's bitmap word.  The
// tile's strings are ONE contiguous span of `data` (offsets[r0] .. offsets[r0 + 64]), so the span is copied to the wave's
// share of LDS with coalesced 16-byte loads and every lane evaluates its row from there with the matcher the host runs too
// (dfx_utf8_match.hpp).  The term's literal bytes and segment table are staged to LDS once per workgroup.
//   * A row that the lengths decide (equality with another length, a LIKE value shorter than the pattern's minimum) or that
//     is null reads no data; a tile of such rows reads none at all, and a tile with a few undecided rows reads just those.
//   * A tile whose span does not fit the wave's share of LDS takes a loop over its rows, the wave on one row at a time:
//     lanes stride over the string in 64-byte chunks and a ballot finds the first chunk that differs (comparisons, prefix,
//     suffix) or the first start that matches (contains).  General patterns stay one lane per row, read from global memory.
//
// Bounds.  Every row's [begin, end) is clamped into [offsets[0], offsets[n]) of the batch -- the bytes the column references,
// DeviceColumn::data_bytes -- before anything is read, so a load never leaves that range whatever the offsets say.  The span
// copy reads 16 bytes wide only where a whole ALIGNED 16-byte word lies inside the span; the bytes before the first such word
// and after the last one are loaded one byte per lane.  No load is rounded outwards: nothing is assumed about what the
// column's owner allocated around the bytes it references.
#include <algorithm>

#include "dfx_k_base_inl.hpp"
#include "dfx_launch.hpp"
#include "dfx_utf8_match.hpp"

namespace dfx {

namespace {
constexpr int kU8Block = 256;                 // four waves
constexpr int kU8Waves = kU8Block / 64;
constexpr uint32_t kU8Span = 4096;            // bytes of a tile's span a wave keeps in LDS (+ 16 of alignment slack)
constexpr uint32_t kU8SpanLds = kU8Span + 16;
typedef uint32_t u8_word16 __attribute__((ext_vector_type(4)));
constexpr int kU8FewRows = 4;                 // a tile with at most this many undecided rows reads them in place

// the wave on ONE row (wave-uniform arguments): first differing byte of v[0, n) and w[0, n), n if there is none
DEV uint32_t u8_wave_mismatch(const uint8_t* v, const uint8_t* w, uint32_t n, int lane) {
  for (uint32_t k = 0; k < n; k += 64u) {
    const uint32_t i = k + (uint32_t)lane;
    const bool diff = i < n && v[i] != w[i];
    const uint64_t b = __ballot(diff);
    if (b) return k + (uint32_t)__builtin_ctzll(b);
  }
  return n;
}

DEV bool u8_wave_row(const Utf8Term& t, const uint8_t* lit, const uint8_t* v, uint32_t vlen, int lane) {
  bool r;
  switch (t.cls) {
    case U8_CMP: {
      const uint32_t n = vlen < t.lit_len ? vlen : t.lit_len;
      const uint32_t at = u8_wave_mismatch(v, lit, n, lane);
      const uint32_t way = at < n ? (v[at] < lit[at] ? 1u : 4u) : (vlen < t.lit_len ? 1u : vlen == t.lit_len ? 2u : 4u);
      return (way & t.m) != 0u;
    }
    case U8_PREFIX: r = u8_wave_mismatch(v, lit, t.lit_len, lane) == t.lit_len; break;
    case U8_SUFFIX: r = u8_wave_mismatch(v + (vlen - t.lit_len), lit, t.lit_len, lane) == t.lit_len; break;
    default: {  // U8_CONTAINS: a lane per start position
      r = false;
      const uint32_t starts = vlen - t.lit_len + 1u;
      for (uint32_t k = 0; k < starts && !r; k += 64u) {
        const uint32_t p = k + (uint32_t)lane;
        r = __ballot(p < starts && utf8_bytes_equal(v + p, lit, t.lit_len)) != 0ull;
      }
      break;
    }
  }
  return r != (t.inv != 0u);
}
}  // namespace

__global__ __launch_bounds__(kU8Block) void k_utf8_pred(const int32_t* __restrict__ offsets, const uint8_t* __restrict__ data,
                                                       const uint8_t* __restrict__ validity, const int64_t bit_offset, const int64_t n,
                                                       const DevUtf8Pred T, uint64_t* __restrict__ mask_words) {
  extern __shared__ __attribute__((aligned(16))) uint8_t u8_lds[];
  const Utf8Term t = T.t;
  const uint32_t term_bytes = (utf8_term_image_bytes(t) + 15u) & ~15u;
  // the literal and the segment table: once per workgroup (T.lit holds them in this layout, 4-byte words)
  for (uint32_t i = threadIdx.x * 4u; i < utf8_term_image_bytes(t); i += kU8Block * 4u) *(uint32_t*)(u8_lds + i) = *(const uint32_t*)(T.lit + i);
  __syncthreads();
  const uint8_t* lit = u8_lds;
  const Utf8Seg* segs = (const Utf8Seg*)(u8_lds + utf8_term_segs_at(t));
  const int lane = lane_id();
  const int wave = (int)(threadIdx.x >> 6);
  uint8_t* span = u8_lds + term_bytes + (uint32_t)wave * kU8SpanLds;
  const int64_t n_words = (n + 63) / 64;
  const int64_t lo_all = (int64_t)offsets[0], hi_all = (int64_t)offsets[n];  // the bytes this batch references
  // The next tile's offsets are requested before this tile is worked on, so that a wave's trip for the offsets overlaps the work
  // on the tile before.  (Measured: it did not move the kernel's time, DESIGN.md section 9b -- the floor is elsewhere.)
  const int64_t stride = (int64_t)gridDim.x * kU8Waves;
  int64_t w = (int64_t)blockIdx.x * kU8Waves + wave;
  int32_t nb = 0, ne = 0;
  if (w < n_words && w * 64 + lane < n) {
    nb = offsets[w * 64 + lane];
    ne = offsets[w * 64 + lane + 1];
  }
  for (; w < n_words; w += stride) {
    const int64_t row = w * 64 + lane;
    const bool in_range = row < n;
    const int32_t ob = nb, oe = ne;
    {
      const int64_t row2 = (w + stride) * 64 + lane;
      if (w + stride < n_words && row2 < n) {
        nb = offsets[row2];
        ne = offsets[row2 + 1];
      }
    }
    int64_t b = lo_all, e = lo_all;
    bool valid = false;
    if (in_range) {
      b = (int64_t)ob;
      e = (int64_t)oe;
      b = b < lo_all ? lo_all : b > hi_all ? hi_all : b;  // never outside the referenced bytes
      e = e < b ? b : e > hi_all ? hi_all : e;
      valid = validity == nullptr || get_bit(validity, bit_offset + row) != 0u;
    }
    const uint32_t vlen = (uint32_t)(e - b);
    bool pass = false, undecided = false;
    if (in_range) {
      if (!valid) pass = t.if_null != 0u;
      else if (t.cls == U8_CMP && (t.m == 2u || t.m == 5u) && vlen != t.lit_len) pass = t.m == 5u;
      else if (t.cls != U8_CMP && vlen < t.min_len) pass = t.inv != 0u;
      else undecided = true;
    }
    const uint64_t todo = __ballot(undecided);
    if (todo != 0ull) {
      // the tile's span: rows are consecutive, so lane 0's begin and the last row's end bracket every row's bytes
      const int64_t sb = __shfl(b, 0, 64);
      int64_t se = e;
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) {
        const int64_t o = __shfl_xor(se, d, 64);
        se = o > se ? o : se;
      }
      const uint32_t pad = (uint32_t)((uintptr_t)(data + sb) & 15u);
      const bool monotonic = __ballot(in_range && b < sb) == 0ull;
      const bool fits = (se - sb) + (int64_t)pad <= (int64_t)kU8Span;
      if (__popcll(todo) <= kU8FewRows || (t.cls == U8_GENERAL && !fits) || !monotonic) {
        // a few rows, or a general pattern over a span that does not fit: each lane reads its own row in place
        if (undecided) pass = utf8_term_eval(t, lit, segs, data + b, vlen);
      } else if (fits) {
        // span -> LDS.  LDS byte (g - a0) holds global byte g, a0 = the span's begin rounded down to 16: the aligned words of the
        // middle land on aligned LDS words.  Head [sb, h) and tail [tl, se) byte-wise, h / tl = the first / last 16-byte boundary
        // inside the span.
        const uint8_t* g0 = data + sb;
        const uint32_t len = (uint32_t)(se - sb);
        uint32_t head = (16u - pad) & 15u;
        head = head < len ? head : len;
        const uint32_t mid = (len - head) & ~15u;
        if ((uint32_t)lane < head) span[pad + (uint32_t)lane] = g0[lane];
        for (uint32_t i = (uint32_t)lane * 16u; i < mid; i += 64u * 16u)
          *(u8_word16*)(span + pad + head + i) = __builtin_nontemporal_load((const u8_word16*)(g0 + head + i));
        const uint32_t tail0 = head + mid;
        if (tail0 + (uint32_t)lane < len) span[pad + tail0 + (uint32_t)lane] = g0[tail0 + (uint32_t)lane];
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (undecided) pass = utf8_term_eval(t, lit, segs, span + pad + (uint32_t)(b - sb), vlen);
        __builtin_amdgcn_wave_barrier();  // the next tile overwrites the span
      } else {
        // long strings: the wave takes the undecided rows one at a time
        uint64_t left = todo;
        while (left) {
          const int src = (int)__builtin_ctzll(left);
          left &= left - 1ull;
          const int64_t rb = __shfl(b, src, 64);
          const uint32_t rl = (uint32_t)__shfl((int)vlen, src, 64);
          const bool r = u8_wave_row(t, lit, data + rb, rl, lane);
          if (lane == src) pass = r;
        }
      }
    }
    const uint64_t word = __ballot(pass);
    if (lane == 0) mask_words[w] = word;
  }
}

// per-tile popcounts of a finished bitmap (what k_predicate_mask leaves beside its words): one wave per 64-word tile
__global__ __launch_bounds__(256) void k_mask_tile_counts(const uint64_t* __restrict__ mask, uint32_t* __restrict__ tile_counts,
                                                          const int64_t n_words, const int64_t n_tiles) {
  const int lane = lane_id();
  const int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tile >= n_tiles) return;
  const int64_t w = tile * 64 + lane;
  uint32_t cnt = w < n_words ? (uint32_t)__popcll(mask[w]) : 0u;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) cnt += (uint32_t)__shfl_xor((int)cnt, m, 64);
  if (lane == 0) tile_counts[tile] = cnt;
}

hipError_t launch_utf8_pred(const int32_t* offsets, const uint8_t* data, const uint8_t* validity, int64_t bit_offset, int64_t n,
                            const DevUtf8Pred& T, uint64_t* mask_words, double algo_bytes, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  Scope sc(KID_UTF8_PRED, s, algo_bytes);
  const uint32_t term_bytes = (utf8_term_image_bytes(T.t) + 15u) & ~15u;  // (as the kernel rounds it: the spans stay 16-byte aligned)
  const size_t lds = (size_t)term_bytes + (size_t)kU8Waves * kU8SpanLds;
  const int64_t n_words = (n + 63) / 64;
  const int64_t blocks = (n_words + kU8Waves - 1) / kU8Waves;
  const int grid = (int)std::min<int64_t>(blocks, (int64_t)device_cu_count() * 32);
  hipLaunchKernelGGL(k_utf8_pred, dim3((unsigned)grid), dim3(kU8Block), lds, s, offsets, data, validity, bit_offset, n, T, mask_words);
  return hipGetLastError();
}

hipError_t launch_mask_tile_counts(const uint64_t* mask_words, uint32_t* tile_counts, int64_t n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int64_t n_words = (n + 63) / 64, n_tiles = (n + kTileRows - 1) / kTileRows;
  hipLaunchKernelGGL(k_mask_tile_counts, dim3((unsigned)((n_tiles + 3) / 4)), dim3(256), 0, s, mask_words, tile_counts, n_words, n_tiles);
  return hipGetLastError();
}

}  // namespace dfx
