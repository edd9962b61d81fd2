// dfx_k_csvwrite.hip -- Arrow columns -> CSV text on the device (deviation D11; the executor of PhysicalPlan::Write,
// src/execution/physicalplan.rs:24-29, which the reference declares and never runs).  The mirror image of dfx_k_csv.hip: one
// wave per tile of 64 rows, the tile staged in the wave's share of LDS, 16-byte global accesses.  dfx_csvwrite.hpp describes the
// two kernels and the slot records between them; the cell text itself comes from dfx_numfmt.hpp, the code the host tests run.
//
// Bounds.  Utf8 rows are clamped into [offsets[0], offsets[n]) of the launch before a byte is read, as k_utf8_pred does.  The
// assemble kernel writes a tile only after it has found its own sum of the row lengths equal to the span the scan gave the tile
// and the span inside the output buffer; otherwise it writes nothing and raises ctrl[0].  No workgroup barrier: a wave owns its
// tile and its share of LDS from start to end.
#include <algorithm>

#include "dfx_csvwrite.hpp"
#include "dfx_k_base_inl.hpp"
#include "dfx_launch.hpp"
#include "dfx_numfmt.hpp"

namespace dfx {

namespace {
constexpr int kCwBlock = 256;
constexpr size_t kCwLdsBudget = 65536;  // per workgroup: fewer waves per workgroup for wide schemas
typedef uint32_t cw_word16 __attribute__((ext_vector_type(4)));

DEV void cw_wave_sync() {  // the wave's LDS writes are visible to all of its lanes
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

DEV bool cw_valid(const DevCwCol& col, int64_t row) { return col.validity == nullptr || get_bit(col.validity, col.bit_offset + row); }

DEV uint64_t cw_load_bits(const DevCwCol& col, int64_t row) {
  switch (col.dtype) {
    case T_BOOL: return get_bit((const uint8_t*)col.values, col.bit_offset + row) ? 1ull : 0ull;
    case T_I8:
    case T_U8: return ((const uint8_t*)col.values)[row];
    case T_I16:
    case T_U16: return ((const uint16_t*)col.values)[row];
    case T_I32:
    case T_U32:
    case T_F32: return ((const uint32_t*)col.values)[row];
    default: return ((const uint64_t*)col.values)[row];
  }
}

// the bytes of a Utf8 row, never outside [lo, hi) = the bytes the launch references; a null or out-of-range row is empty
DEV void cw_utf8_row(const DevCwCol& col, int64_t row, bool live, int64_t lo, int64_t hi, int64_t* begin, uint32_t* len) {
  int64_t b = lo, e = lo;
  if (live && cw_valid(col, row)) {
    b = (int64_t)col.offsets[row];
    e = (int64_t)col.offsets[row + 1];
    b = b < lo ? lo : b > hi ? hi : b;
    e = e < b ? b : e > hi ? hi : e;
  }
  *begin = b;
  *len = (uint32_t)(e - b);
}

DEV uint64_t cw_wave_sum(uint64_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += (uint64_t)__shfl_xor((long long)v, d, 64);
  return v;
}
}  // namespace

__global__ __launch_bounds__(kCwBlock) void k_csvw_format(const DevCwPlan P, const int64_t n, uint8_t* __restrict__ slots,
                                                         uint64_t* __restrict__ tile_bytes) {
  extern __shared__ __attribute__((aligned(16))) uint8_t cw_lds[];
  const int lane = lane_id();
  const int wave = (int)(threadIdx.x >> 6);
  const int64_t tile = (int64_t)blockIdx.x * (int64_t)(blockDim.x >> 6) + wave;
  if (tile >= (n + 63) / 64) return;
  const uint32_t area = 64u * P.stride;
  uint8_t* ws = cw_lds + (size_t)wave * area;
  uint8_t* slot = ws + (uint32_t)lane * P.stride;
  const int64_t row = tile * 64 + lane;
  const bool in = row < n;
  const bool one = P.n_cols == 1;  // the reader skips blank lines: the empty cell of a one-column file is written ""
  uint64_t row_len = in ? (uint64_t)P.n_cols : 0ull;  // the delimiters and the terminator
  for (int c = 0; c < P.n_cols; ++c) {  // wave-uniform: one column, one dtype for all lanes
    const DevCwCol col = P.col[c];
    if (col.dtype == T_UTF8) {
      const int64_t lo = (int64_t)col.offsets[0], hi = (int64_t)col.offsets[n];
      int64_t b;
      uint32_t len;
      cw_utf8_row(col, row, in, lo, hi, &b, &len);
      uint64_t quotes = 0;
      bool special = false;
      const bool is_long = len > kCwLongCell;
      if (!is_long) special = nf_csv_scan(col.data + b, len, &quotes);
      uint64_t todo = __ballot(is_long);
      while (todo) {  // the wave on one long string
        const int src = (int)__builtin_ctzll(todo);
        todo &= todo - 1ull;
        const int64_t sb = __shfl((long long)b, src, 64);
        const uint32_t sl = (uint32_t)__shfl((int)len, src, 64);
        uint64_t q = 0;
        bool sp = false;
        for (uint32_t k = 0; k < sl; k += 64u) {
          const uint32_t i = k + (uint32_t)lane;
          const uint8_t ch = i < sl ? col.data[sb + i] : (uint8_t)0;
          q += (uint64_t)__popcll(__ballot(ch == '"'));
          sp = sp || __ballot(nf_csv_special(ch)) != 0ull;
        }
        if (lane == src) {
          quotes = q;
          special = sp;
        }
      }
      const bool quoted = special || (one && len == 0u);
      if (in) {
        *(uint32_t*)(slot + col.slot) = (uint32_t)quotes | (quoted ? 0x80000000u : 0u);
        row_len += nf_csv_cell_len(len, quotes, quoted);
      }
    } else if (in) {
      int l = 0;
      if (cw_valid(col, row)) {
        l = nf_format_value((int)col.dtype, cw_load_bits(col, row), slot + col.slot);
      } else if (one) {
        slot[col.slot] = '"';
        slot[col.slot + 1u] = '"';
        l = 2;
      }
      slot[c] = (uint8_t)l;
      row_len += (uint64_t)l;
    }
  }
  const uint64_t total = cw_wave_sum(row_len);
  if (lane == 0) tile_bytes[tile] = total;
  cw_wave_sync();
  uint8_t* dst = slots + (size_t)tile * area;  // the tile's slots: one contiguous, 16-byte aligned span
  for (uint32_t i = (uint32_t)lane * 16u; i < area; i += 1024u) *(cw_word16*)(dst + i) = *(const cw_word16*)(ws + i);
}

// exclusive scan of up to a few 10^4 tile lengths into 64-bit offsets, out[n] = the total: one workgroup
__global__ __launch_bounds__(1024) void k_csvw_scan(const uint64_t* __restrict__ in, const int64_t n, uint64_t* __restrict__ out) {
  __shared__ uint64_t sums[1024];
  const int t = (int)threadIdx.x;
  const int64_t chunk = (n + 1023) / 1024;
  const int64_t b = std::min<int64_t>((int64_t)t * chunk, n), e = std::min<int64_t>(b + chunk, n);
  uint64_t s = 0;
  for (int64_t i = b; i < e; ++i) s += in[i];
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
    out[i] = run;
    run += in[i];
  }
  if (t == 1023) out[n] = sums[1023];
}

__global__ __launch_bounds__(kCwBlock) void k_csvw_assemble(const DevCwPlan P, const int64_t n, const uint8_t* __restrict__ slots,
                                                           const uint64_t* __restrict__ tile_base, uint8_t* __restrict__ out,
                                                           const uint64_t out_bytes, uint64_t* __restrict__ ctrl) {
  extern __shared__ __attribute__((aligned(16))) uint8_t cw_lds[];
  const int lane = lane_id();
  const int wave = (int)(threadIdx.x >> 6);
  const int64_t tile = (int64_t)blockIdx.x * (int64_t)(blockDim.x >> 6) + wave;
  if (tile >= (n + 63) / 64) return;
  const uint32_t area = 64u * P.stride;
  uint8_t* ws = cw_lds + (size_t)wave * (area + P.window + 16u);
  uint8_t* win = ws + area;
  {  // the tile's slots -> LDS
    const uint8_t* src = slots + (size_t)tile * area;
    for (uint32_t i = (uint32_t)lane * 16u; i < area; i += 1024u) *(cw_word16*)(ws + i) = __builtin_nontemporal_load((const cw_word16*)(src + i));
  }
  cw_wave_sync();
  const uint8_t* slot = ws + (uint32_t)lane * P.stride;
  const int64_t row = tile * 64 + lane;
  const bool in = row < n;
  // the row's length, as the format kernel summed it
  uint64_t row_len = in ? (uint64_t)P.n_cols : 0ull;
  for (int c = 0; c < P.n_cols && in; ++c) {
    const DevCwCol col = P.col[c];
    if (col.dtype == T_UTF8) {
      int64_t b;
      uint32_t len;
      cw_utf8_row(col, row, true, (int64_t)col.offsets[0], (int64_t)col.offsets[n], &b, &len);
      const uint32_t desc = *(const uint32_t*)(slot + col.slot);
      row_len += nf_csv_cell_len(len, desc & 0x7FFFFFFFu, (desc >> 31) != 0u);
    } else {
      row_len += slot[c];
    }
  }
  uint64_t inc = row_len;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t o = (uint64_t)__shfl_up((long long)inc, d, 64);
    if (lane >= d) inc += o;
  }
  const uint64_t row_off = inc - row_len;
  const uint64_t total = (uint64_t)__shfl((long long)inc, 63, 64);
  const uint64_t base = tile_base[tile];
  if (total != tile_base[tile + 1] - base || base + total > out_bytes || base + total < base) {
    if (lane == 0) atomicOr((unsigned long long*)&ctrl[0], 1ull);  // the two kernels disagree: write nothing
    return;
  }
  uint8_t* g0 = out + base;
  const uint32_t pad = (uint32_t)((uintptr_t)g0 & 15u);
  if (total + pad <= (uint64_t)P.window) {
    // rows back to back in the window; LDS byte pad + i holds text byte i, so the aligned words of the span are aligned in LDS
    if (in) {
      uint8_t* p = win + pad + (uint32_t)row_off;
      for (int c = 0; c < P.n_cols; ++c) {
        const DevCwCol col = P.col[c];
        if (col.dtype == T_UTF8) {
          int64_t b;
          uint32_t len;
          cw_utf8_row(col, row, true, (int64_t)col.offsets[0], (int64_t)col.offsets[n], &b, &len);
          const uint32_t desc = *(const uint32_t*)(slot + col.slot);
          p += nf_csv_put_cell(col.data + b, len, (desc >> 31) != 0u, p);
        } else {
          const uint32_t l = slot[c];
          const uint8_t* t = slot + col.slot;
          for (uint32_t j = 0; j < l; ++j) p[j] = t[j];
          p += l;
        }
        *p++ = c + 1 < P.n_cols ? (uint8_t)',' : (uint8_t)'\n';
      }
    }
    cw_wave_sync();
    const uint32_t len = (uint32_t)total;
    uint32_t head = (16u - pad) & 15u;
    head = head < len ? head : len;
    const uint32_t mid = (len - head) & ~15u;
    if ((uint32_t)lane < head) g0[lane] = win[pad + (uint32_t)lane];
    for (uint32_t i = (uint32_t)lane * 16u; i < mid; i += 1024u) *(cw_word16*)(g0 + head + i) = *(const cw_word16*)(win + pad + head + i);
    const uint32_t tail0 = head + mid;
    if (tail0 + (uint32_t)lane < len) g0[tail0 + (uint32_t)lane] = win[pad + tail0 + (uint32_t)lane];
    return;
  }
  // general path: the tile's text is longer than the window.  A lane per row straight to its final position, the wave together
  // on every long Utf8 cell.
  if (lane == 0) atomicAdd((unsigned long long*)&ctrl[1], 1ull);
  uint64_t pos = base + row_off;
  for (int c = 0; c < P.n_cols; ++c) {  // wave-uniform
    const DevCwCol col = P.col[c];
    if (col.dtype == T_UTF8) {
      int64_t b;
      uint32_t len;
      cw_utf8_row(col, row, in, (int64_t)col.offsets[0], (int64_t)col.offsets[n], &b, &len);
      const uint32_t desc = in ? *(const uint32_t*)(slot + col.slot) : 0u;
      const bool quoted = (desc >> 31) != 0u;
      const bool is_long = in && len > kCwLongCell;
      if (in && !is_long) pos += nf_csv_put_cell(col.data + b, len, quoted, out + pos);
      uint64_t todo = __ballot(is_long);
      while (todo) {
        const int src = (int)__builtin_ctzll(todo);
        todo &= todo - 1ull;
        const int64_t sb = __shfl((long long)b, src, 64);
        const uint32_t sl = (uint32_t)__shfl((int)len, src, 64);
        const bool sq = __shfl(quoted ? 1 : 0, src, 64) != 0;
        uint64_t o = (uint64_t)__shfl((long long)pos, src, 64);
        if (sq) {
          if (lane == 0) out[o] = '"';
          o += 1;
        }
        for (uint32_t k = 0; k < sl; k += 64u) {
          const uint32_t i = k + (uint32_t)lane;
          const bool live = i < sl;
          const uint8_t ch = live ? col.data[sb + i] : (uint8_t)0;
          const bool dbl = sq && live && ch == '"';
          const uint64_t m = __ballot(dbl);
          if (live) {
            const uint64_t d = o + (uint64_t)lane + (uint64_t)__popcll(m & ((1ull << lane) - 1ull));
            out[d] = ch;
            if (dbl) out[d + 1] = '"';
          }
          o += (uint64_t)(sl - k < 64u ? sl - k : 64u) + (uint64_t)__popcll(m);
        }
        if (sq && lane == 0) out[o] = '"';
      }
      if (is_long) pos += nf_csv_cell_len(len, desc & 0x7FFFFFFFu, quoted);
    } else if (in) {
      const uint32_t l = slot[c];
      const uint8_t* t = slot + col.slot;
      for (uint32_t j = 0; j < l; ++j) out[pos + j] = t[j];
      pos += l;
    }
    if (in) out[pos++] = c + 1 < P.n_cols ? (uint8_t)',' : (uint8_t)'\n';
  }
}

uint32_t csvw_layout(DevCwPlan* plan) {
  uint32_t at = ((uint32_t)plan->n_cols + 3u) & ~3u;  // the cell length bytes, then the 4-byte Utf8 descriptors, then the cell text
  for (int c = 0; c < plan->n_cols; ++c)
    if (plan->col[c].dtype == T_UTF8) {
      plan->col[c].slot = at;
      at += 4u;
    }
  for (int c = 0; c < plan->n_cols; ++c)
    if (plan->col[c].dtype != T_UTF8) {
      plan->col[c].slot = at;
      at += (uint32_t)nf_max_cell((int)plan->col[c].dtype);
    }
  plan->stride = (at + 15u) & ~15u;
  // the window: no tile of fixed-width cells alone can miss it; what a workgroup's LDS budget leaves when the slots are large
  const uint32_t area = 64u * plan->stride;
  const uint32_t room = area + 16u + kCwWindowMin <= (uint32_t)kCwLdsBudget ? ((uint32_t)kCwLdsBudget - 16u - area) & ~15u : kCwWindowMin;
  plan->window = std::max(kCwWindowMin, std::min(std::min(kCwWindowMax, room), area + 2048u));
  return plan->stride;
}

size_t csvw_wave_lds(const DevCwPlan& plan) { return (size_t)64 * plan.stride + plan.window + 16u; }

static int csvw_waves(size_t per_wave) { return (int)std::max<size_t>(1, std::min<size_t>(kCwBlock / 64, kCwLdsBudget / per_wave)); }

hipError_t launch_csvw_format(const DevCwPlan& plan, int64_t n, uint8_t* slots, uint64_t* tile_bytes, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const size_t per_wave = (size_t)64 * plan.stride;
  if (per_wave > kCwLdsBudget) return hipErrorInvalidValue;
  const int waves = csvw_waves(per_wave);
  const int64_t n_tiles = (n + 63) / 64;
  Scope sc(KID_CSV_WRITE, s, 0.0);
  hipLaunchKernelGGL(k_csvw_format, dim3((unsigned)((n_tiles + waves - 1) / waves)), dim3((unsigned)(64 * waves)), per_wave * (size_t)waves, s, plan, n, slots,
                     tile_bytes);
  return hipGetLastError();
}

hipError_t launch_csvw_scan(const uint64_t* tile_bytes, int64_t n_tiles, uint64_t* tile_base, hipStream_t s) {
  if (n_tiles <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_csvw_scan, dim3(1), dim3(1024), 0, s, tile_bytes, n_tiles, tile_base);
  return hipGetLastError();
}

hipError_t launch_csvw_assemble(const DevCwPlan& plan, int64_t n, const uint8_t* slots, const uint64_t* tile_base, uint8_t* out,
                                uint64_t out_bytes, uint64_t* ctrl, double algo_bytes, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const size_t per_wave = csvw_wave_lds(plan);
  if (per_wave > kCwLdsBudget) return hipErrorInvalidValue;
  const int waves = csvw_waves(per_wave);
  const int64_t n_tiles = (n + 63) / 64;
  Scope sc(KID_CSV_WRITE, s, algo_bytes);
  hipLaunchKernelGGL(k_csvw_assemble, dim3((unsigned)((n_tiles + waves - 1) / waves)), dim3((unsigned)(64 * waves)), per_wave * (size_t)waves, s, plan, n, slots,
                     tile_base, out, out_bytes, ctrl);
  return hipGetLastError();
}

}  // namespace dfx
