// dfx_k_filter.hip -- the filter operator's kernels (FilterRelation, dfx_filter.cpp): predicate -> bitmap (K1), the single-pass
// filter (K1 + K4 with a look-back over the tiles' kept counts) and its dense flavour, the AND of two bitmaps, compaction (K4).
// Design rules and compile flags: see dfx_k_core.hip.
#include "dfx_kernels.hpp"

#include <hip/hip_runtime.h>

#include <atomic>
#include <type_traits>

#include "dfx_k_policy_inl.hpp"
#include "dfx_launch.hpp"

namespace dfx {

// ---------------------------------------------------------------------------------------------
// K1 predicate_mask
// ---------------------------------------------------------------------------------------------
template <typename POL>
__global__ __launch_bounds__(kBlock) void k_predicate_mask(const DevProgram P, const DevFastPlan F, const DevColumns C,
                                                           const uint8_t pred, const int64_t n,
                                                           uint64_t* __restrict__ mask_words,
                                                           uint32_t* __restrict__ tile_counts,
                                                           uint32_t* __restrict__ ctrl) {
  typedef typename POL::COLV COLV;
  constexpr int U = POL::U;
  __shared__ uint32_t wave_cnt[kBlock / 64];
  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  const int64_t n_words = (n + 63) >> 6;
  const int64_t n_tiles = (n + kTileRows - 1) / kTileRows;
  uint32_t err = 0;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    uint32_t cnt = 0;
    for (int i0 = 0; i0 < 16; i0 += U) {
      const int64_t w0 = tile * 64 + wave * 16 + i0;
      COLV col[U];
      uint32_t cv[U];
      FOR_U {
        const int64_t row = (w0 + u) * 64 + lane;
        POL::load(P, C, row, row < n, col[u], cv[u]);
      }
#pragma nounroll
      for (int uu = 0; uu < U; ++uu) {
        COLV cur;
        uint32_t curv;
        DFX_SELECT_BANK(uu, col, cv, cur, curv)
        const int64_t w = w0 + uu;
        const bool inb = w * 64 + lane < n;
        u64x16 reg;
        uint32_t rv = 0;
        POL::eval(P, F, cur, curv, reg, rv, inb, err);
        const bool pass = inb && POL::pass(P, F, pred, cur, curv, reg, rv);
        const uint64_t word = __ballot(pass);
        if (lane == 0 && w < n_words) mask_words[w] = word;
        cnt += (uint32_t)__popcll(word);
      }
    }
    if (tile_counts != nullptr) {
      if (lane == 0) wave_cnt[wave] = cnt;
      __syncthreads();
      if (threadIdx.x == 0) tile_counts[tile] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
      __syncthreads();
    }
  }
  if (err) atomicOr(&ctrl[CTRL_ERROR], err);
}

// ---------------------------------------------------------------------------------------------
// K1 + K4 in one pass: single-pass FilterRelation
// ---------------------------------------------------------------------------------------------
// The two-pass form (k_predicate_mask -> scan of the tile counts -> k_compact) reads a predicate column twice: once to
// evaluate it, once to compact it.  Here a workgroup evaluates a SUPER-TILE of four 4096-row tiles (one tile per wave),
// parks the passing rows' values of up to kFusedOutCols of the predicate's own columns in LDS (wave-private segments:
// position = rows the wave kept so far + rank inside the ballot word), learns where its super-tile starts in the output
// from a LOOK-BACK over the kept counts of the super-tiles before it, and copies its segments out in whole coalesced
// runs.  Row order is preserved (filter.rs:86-90).  The Arrow bitmap and the per-tile exclusive offsets are written as
// well: every OTHER column of the batch is compacted by k_compact from them, reading it once, too.
//
// Look-back, two levels.  Super-tiles are dealt round-robin to a co-resident grid (G ~ 1000 workgroups), which therefore
// runs in lockstep: the G super-tiles of a round publish their counts at about the same time and every one of them needs
// the sum of all earlier ones.  A flat decoupled look-back (64 predecessors per step) walks G/128 windows on average, and
// a status round trip under a streaming load costs microseconds (first version of this kernel, 4096-row units: 12 us of
// look-back per 5 us of streaming; two levels: still ~10 us, three dependent round trips).  So: (a) one status word per
// SUPER-TILE {ready, count} and one per GROUP of 64 consecutive super-tiles {aggregate | inclusive prefix}: a super-tile
// adds up the counts of the super-tiles before it in its own group -- one 64-wide load -- and the prefix before its group
// from the group words -- one more 64-wide load that covers 4096 units; both loads are in flight together; the last
// super-tile of a group publishes the group's aggregate as soon as it has the former, and the group's inclusive prefix
// when it has the latter; (b) 128 KB of column per synchronisation instead of 32; (c) the column loads are
// software-pipelined ACROSS super-tiles: a workgroup's first loads of its next super-tile are in flight while it sits in
// the two barriers and the look-back of the current one.
// LDS: a wave parks at most kFusedStage values per column (a quarter of its tile: selectivities up to ~24 %); a wave that
// keeps more reads its tile's passing rows AGAIN after the look-back (the bitmap words are in LDS) -- dense filters fall
// back to two reads of the column for those tiles, never to a wrong result.
// Forward progress: every workgroup takes its super-tiles in increasing order, publishes a count BEFORE it waits, a group
// aggregate needs counts only, a group prefix needs aggregates and the nearest earlier prefix (group 0 needs none): the
// smallest unpublished word never waits for anything unpublished.  The grid must be co-resident (launch_filter_fused
// sizes it from the occupancy API); the spin is bounded all the same (error bit 8).
constexpr uint64_t kLbAggregate = 1ull << 62, kLbInclusive = 2ull << 62, kLbFlags = 3ull << 62;
constexpr int kLbGroup = 64;            // super-tiles per second-level word
constexpr int kFusedTiles = kBlock / 64;  // tiles per super-tile: one per wave
constexpr int kFusedStage = 1024;       // values a wave can park per column

size_t filter_fused_sync_words(int64_t n) {
  const size_t tiles = (size_t)((n + kTileRows - 1) / kTileRows);
  const size_t units = (tiles + kFusedTiles - 1) / kFusedTiles;
  return 2 + units + (units + kLbGroup - 1) / kLbGroup;
}

DEV uint32_t mbcnt_u64(uint64_t m) {
  return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
DEV uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += shfl_xor_u64(v, m);
  return v;
}

// The look-back of one super-tile (wave 0 of its workgroup): publish the super-tile's kept count A, add up what the
// super-tiles before it kept (see above), publish the group words this super-tile owes, leave the exclusive prefix in *s_base.
DEV void filter_lookback(const int64_t unit, const int64_t n_units, const int64_t n_tiles, const uint32_t A, uint64_t* __restrict__ state,
                         uint64_t* __restrict__ gstate, uint64_t* __restrict__ sync, uint64_t* __restrict__ tile_offsets,
                         uint32_t* __restrict__ ctrl, const int lane, uint64_t* s_base, uint32_t& err) {
  if (lane == 0) __hip_atomic_store(&state[unit], kLbAggregate | (uint64_t)A, RLX_AGENT);
  const int64_t g = unit / kLbGroup;
  const int q = (int)(unit % kLbGroup);
  const bool last_of_group = q == kLbGroup - 1 || unit == n_units - 1;
  bool need_w = q > 0, need_g = g > 0, agg_pending = last_of_group && g > 0;
  uint64_t within = 0, before = 0;
  int64_t ghi = g - 1;  // lane l looks at group ghi - l
  uint32_t spins = 0;
  while (need_w || need_g) {
    uint64_t st = 0, gs = 0;
    if (need_w) st = __hip_atomic_load(&state[lane < q ? unit - 1 - lane : unit], RLX_AGENT);
    if (need_g) {
      const int64_t gj = ghi - lane;
      gs = __hip_atomic_load(&gstate[gj >= 0 ? gj : 0], RLX_AGENT);
      if (gj < 0) gs = kLbInclusive;  // before group 0: inclusive prefix 0
    }
    bool moved = false;
    if (need_w) {
      if (__ballot(lane < q && (st & kLbFlags) == 0) == 0) {  // every unit before this one in its group has published
        within = wave_sum_u64(lane < q ? (st & ~kLbFlags) : 0ull);
        need_w = false;
      }
    }
    if (!need_w && agg_pending) {  // the group's aggregate: everybody after this group waits for it
      if (lane == 0) __hip_atomic_store(&gstate[g], kLbAggregate | (within + (uint64_t)A), RLX_AGENT);
      agg_pending = false;
    }
    if (need_g) {
      const uint64_t fl = gs & kLbFlags;
      const uint64_t not_ready = __ballot(fl == 0);
      const uint64_t incl = __ballot(fl == kLbInclusive);
      if (incl != 0) {
        const int pl = __ffsll((unsigned long long)incl) - 1;  // nearest group with an inclusive prefix
        const uint64_t upto = pl == 63 ? ~0ull : ((1ull << (pl + 1)) - 1ull);
        if ((not_ready & upto) == 0) {
          before += wave_sum_u64(((upto >> lane) & 1ull) ? (gs & ~kLbFlags) : 0ull);
          need_g = false;
        }
      } else if (not_ready == 0) {  // 64 aggregates, no prefix among them: add them all, look 64 groups further back
        before += wave_sum_u64(gs & ~kLbFlags);
        ghi -= 64;
        moved = true;
      }
    }
    if (!(need_w || need_g) || moved) continue;
    if (++spins > (1u << 22)) {  // cannot happen (see above); never hang the device
      err |= 8u;
      break;
    }
    __builtin_amdgcn_s_sleep(1);
  }
  const uint64_t base = before + within;
  if (lane == 0) {
    if (last_of_group) __hip_atomic_store(&gstate[g], kLbInclusive | (base + (uint64_t)A), RLX_AGENT);
    *s_base = base;
    if (unit == n_units - 1) {
      tile_offsets[n_tiles] = base + (uint64_t)A;
      sync[1] = base + (uint64_t)A;  // kept rows of the batch
      ctrl[CTRL_PASSED_LO] = (uint32_t)(base + (uint64_t)A);  // ... and next to the error word: ONE read-back per batch
      ctrl[CTRL_PASSED_HI] = (uint32_t)((base + (uint64_t)A) >> 32);
    }
  }
}

// (a compile-time signature fits 128 VGPRs -- four workgroups per CU --, the generic policies take what they need)
template <typename POL>
__global__ __launch_bounds__(kBlock, (POL::kStaticNa == 0 && sizeof(typename POL::COLV) == 16 && POL::U == 8 && POL::kIsStatic) ? 4 : 1) void k_filter_fused(const DevProgram P, const DevFastPlan F, const DevColumns C,
                                                         const uint8_t pred, const int64_t n,
                                                         uint64_t* __restrict__ mask_words,
                                                         uint64_t* __restrict__ tile_offsets,
                                                         uint64_t* __restrict__ sync, const DevFusedOut O,
                                                         uint32_t* __restrict__ ctrl) {
  typedef typename POL::COLV COLV;
  constexpr int U = POL::U;
  constexpr int BANK = (int)(sizeof(COLV) / 8);
  constexpr int NW = kFusedTiles;              // waves per workgroup = tiles per super-tile
  constexpr int kTileWords = kTileRows / 64;   // 64 bitmap words per tile
  static_assert(kLbGroup == 64 && kTileWords == 64, "one lane per unit of a group / per bitmap word of a tile");
  extern __shared__ __attribute__((aligned(16))) uint64_t stage[];  // [O.n][NW][kFusedStage] kept values
  __shared__ uint64_t s_words[NW * kTileWords];
  __shared__ uint32_t s_wave_cnt[NW];
  __shared__ uint64_t s_base;
  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  const int64_t n_words = (n + 63) >> 6;
  const int64_t n_tiles = (n + kTileRows - 1) / kTileRows;
  const int64_t n_units = (n_tiles + NW - 1) / NW;
  uint64_t* const state = sync + 2;          // per super-tile
  uint64_t* const gstate = state + n_units;  // per group of kLbGroup super-tiles
  uint32_t err = 0;
  // the whole loop once per comparison FORM (StaticPolicy::pass_form: compile-time operators; 0: run-time masks)
  auto run = [&](auto form_tag) {
  constexpr int FORM = decltype(form_tag)::value;
  int64_t unit = blockIdx.x;
  COLV ncol[U];
  uint32_t ncv[U];
  load_trip<POL>(P, C, (unit * NW + wave) * kTileWords, unit < n_units, n, lane, ncol, ncv);  // the very first loads of this workgroup
  for (; unit < n_units; unit += gridDim.x) {
    const int64_t tile = unit * NW + wave;  // this wave's tile
    uint32_t cnt = 0;                       // rows this wave has kept in its tile (wave-uniform)
    for (int i0 = 0; i0 < kTileWords; i0 += U) {
      const int64_t w0 = tile * kTileWords + i0;
      COLV col[U];
      uint32_t cv[U];
      FOR_U {
        col[u] = ncol[u];
        cv[u] = ncv[u];
      }
      {  // the next trip's loads (of this tile, or the first ones of the workgroup's next super-tile) before this trip is evaluated
        const bool same = i0 + U < kTileWords;
        const int64_t nu = same ? unit : unit + gridDim.x;
        load_trip<POL>(P, C, (nu * NW + wave) * kTileWords + (same ? i0 + U : 0), nu < n_units, n, lane, ncol, ncv);
      }
      auto one_group = [&](const COLV& cur, uint32_t curv, int uu) {
        const int64_t w = w0 + uu;
        const bool inb = w * 64 + lane < n;
        u64x16 reg;
        uint32_t rv = 0;
        POL::eval(P, F, cur, curv, reg, rv, inb, err);
        const bool pass = inb && POL::template pass_form<FORM>(P, F, pred, cur, curv, reg, rv);
        const uint64_t word = __ballot(pass);
        if (lane == 0) s_words[wave * kTileWords + i0 + uu] = word;
        const uint32_t at = cnt + mbcnt_u64(word);
        if (pass && at < (uint32_t)kFusedStage) {
#pragma unroll
          for (int o = 0; o < kFusedOutCols; ++o) {
            if (o < O.n) {
              uint64_t v = cur[0];
#pragma unroll
              for (int c = 1; c < BANK; ++c) v = (O.slot[o] == c) ? cur[c] : v;
              stage[(size_t)(o * NW + wave) * kFusedStage + at] = v;
            }
          }
        }
        cnt += (uint32_t)__popcll(word);
      };
      if constexpr (POL::kIsStatic) {  // straight-line code is short here: unrolled (no scalar branch chain to pick the bank)
        FOR_U one_group(col[u], cv[u], u);
      } else {  // the interpreter's body is long: ONE copy, the group's bank re-selected at run time
#pragma nounroll
        for (int uu = 0; uu < U; ++uu) {
          COLV cur;
          uint32_t curv;
          DFX_SELECT_BANK(uu, col, cv, cur, curv)
          one_group(cur, curv, uu);
        }
      }
    }
    {  // this tile's 64 bitmap words: one coalesced 512-byte store per wave
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      const int64_t w = tile * kTileWords + lane;
      if (w < n_words) mask_words[w] = s_words[wave * kTileWords + lane];
    }
    if (lane == 0) s_wave_cnt[wave] = cnt;
    __syncthreads();
    uint32_t wc[NW];
    uint32_t A = 0;
#pragma unroll
    for (int k = 0; k < NW; ++k) {
      wc[k] = s_wave_cnt[k];
      A += wc[k];
    }
    if (wave == 0) filter_lookback(unit, n_units, n_tiles, A, state, gstate, sync, tile_offsets, ctrl, lane, &s_base, err);
    __syncthreads();
    uint64_t my_base = s_base;
#pragma unroll
    for (int k = 0; k < NW; ++k)
      if (k < wave) my_base += wc[k];
    if (lane == 0 && tile < n_tiles) tile_offsets[tile] = my_base;
#pragma unroll
    for (int o = 0; o < kFusedOutCols; ++o) {
      if (o < O.n) {
        const uint8_t t = O.dtype[o];
        // (the output buffers hold O.cap_rows rows: what lies beyond is the host's to compact again)
        const uint32_t room = my_base >= O.cap_rows ? 0u : (O.cap_rows - my_base < (uint64_t)cnt ? (uint32_t)(O.cap_rows - my_base) : cnt);
        if (cnt <= (uint32_t)kFusedStage) {  // (wave-uniform) everything this wave kept is parked in LDS
          const uint64_t* src = stage + (size_t)(o * NW + wave) * kFusedStage;
          if (t == T_F64 || t == T_I64 || t == T_U64) {
            uint64_t* dst = (uint64_t*)O.out[o] + my_base;
            for (uint32_t j = (uint32_t)lane; j < room; j += 64) dst[j] = src[j];
          } else {
            for (uint32_t j = (uint32_t)lane; j < room; j += 64) store_typed(t, O.out[o], (int64_t)(my_base + j), src[j]);
          }
        } else {  // a dense tile: its passing rows are read again (bitmap words from LDS), as k_compact would -- the tile was
                  // streamed through this CU microseconds ago, so the second read is an L2 / Infinity Cache hit, not HBM traffic.
                  // Eight row groups per step, their loads issued together: one dependent load -> store round trip per row group
                  // (64 per tile) made selectivities above a quarter cost 2.5 x the selective case (cfg2_filter_dense_sel50: 0.29).
          const int slot = O.slot[o];
          constexpr int kStep = 8;  // (16 was measured: the selective path lost 13 % -- 0.588 -> 0.510 -- to the registers the dense path asked for)
          static_assert(kTileWords % kStep == 0, "whole steps");
          uint32_t run = 0;
          const int64_t n_rows_m1 = n - 1;
          // (the width is decided once per tile, outside the steps: a dtype switch around every load would put a join --
          // and a conservative wait -- between them)
          auto steps = [&](auto load_one, auto store_one) {
            for (int i0 = 0; i0 < kTileWords; i0 += kStep) {
              uint64_t word[kStep], v[kStep];
#pragma unroll
              for (int j = 0; j < kStep; ++j) {
                word[j] = s_words[wave * kTileWords + i0 + j];
                int64_t row = (tile * kTileWords + i0 + j) * 64 + lane;
                row = row < n_rows_m1 ? row : n_rows_m1;  // (unconditional loads: rows past the end are never selected)
                v[j] = load_one(row);
              }
#pragma unroll
              for (int j = 0; j < kStep; ++j) {
                if ((word[j] >> lane) & 1ull) {
                  const uint32_t at = run + mbcnt_u64(word[j]);
                  if (at < room) store_one(my_base + at, v[j]);
                }
                run += (uint32_t)__popcll(word[j]);
              }
            }
          };
          if (t == T_F64 || t == T_I64 || t == T_U64) {
            const uint64_t* in8 = (const uint64_t*)C.c[slot].values;
            uint64_t* out8 = (uint64_t*)O.out[o];
            steps([&](int64_t row) { return in8[row]; }, [&](uint64_t at, uint64_t v) { out8[at] = v; });
          } else if (t == T_I32 || t == T_U32 || t == T_F32) {
            const uint32_t* in4 = (const uint32_t*)C.c[slot].values;
            uint32_t* out4 = (uint32_t*)O.out[o];
            steps([&](int64_t row) { return (uint64_t)in4[row]; }, [&](uint64_t at, uint64_t v) { out4[at] = (uint32_t)v; });
          } else {
            steps([&](int64_t row) { return load_canonical(t, C.c[slot].values, row, C.c[slot].bit_offset); },
                  [&](uint64_t at, uint64_t v) { store_typed(t, O.out[o], (int64_t)at, v); });
          }
        }
      }
    }
    // (the next super-tile's first barrier separates these reads of s_base / s_words / stage from their next writes)
  }
  };
  switch (POL::form_of(F)) {  // (wave-uniform: the plan sits in the kernarg segment)
    case 4 | (1 << 3): run(std::integral_constant<int, (POL::kIsStatic ? (4 | (1 << 3)) : 0)>{}); break;  // x >  a AND x <  b
    case 6 | (1 << 3): run(std::integral_constant<int, (POL::kIsStatic ? (6 | (1 << 3)) : 0)>{}); break;  // x >= a AND x <  b
    case 4 | (3 << 3): run(std::integral_constant<int, (POL::kIsStatic ? (4 | (3 << 3)) : 0)>{}); break;  // x >  a AND x <= b
    case 6 | (3 << 3): run(std::integral_constant<int, (POL::kIsStatic ? (6 | (3 << 3)) : 0)>{}); break;  // x >= a AND x <= b
    default: run(std::integral_constant<int, 0>{}); break;
  }
  if (err) atomicOr(&ctrl[CTRL_ERROR], err);
}

// DENSE flavour (round 4): the tile stays in REGISTERS.  k_filter_fused parks a wave's kept values in LDS -- at most a quarter of
// its tile -- and a wave that keeps more reads its passing rows a second time after the look-back: 8 + 8 sel + 8 sel bytes of
// traffic per row, which is all that selectivities of 0.5 / 0.9 could ever reach (0.40 / 0.44 of the roofline).  Here a wave loads
// its whole 4096-row tile up front -- 64 independent 512-byte loads, 128 vector registers --, evaluates the predicate from the
// registers, keeps bitmap word i in lane i (one coalesced 512-byte store per tile, `v_readlane` hands the words back after the
// look-back) and stores the kept values from the same registers: the column is read ONCE whatever the selectivity, nothing is
// staged in LDS.  Two workgroups per CU (256 registers each): while one waits in its look-back the other streams.
// For the shape config 2 is written in: a compile-time signature over ONE 8-byte column, which is also the one column the kernel
// compacts (launch_filter_fused checks); chosen by the host once a stream has kept more than a wave can park (DevFusedOut::dense).
template <typename POL, int FORM>
__global__ __launch_bounds__(kBlock, 2) void k_filter_fused_dense(const DevProgram P, const DevFastPlan F, const DevColumns C,
                                                                  const uint8_t pred, const int64_t n,
                                                                  uint64_t* __restrict__ mask_words,
                                                                  uint64_t* __restrict__ tile_offsets,
                                                                  uint64_t* __restrict__ sync, const DevFusedOut O,
                                                                  uint32_t* __restrict__ ctrl) {
  typedef typename POL::COLV COLV;
  constexpr int BANK = (int)(sizeof(COLV) / 8);
  constexpr int NW = kFusedTiles;
  constexpr int kTileWords = kTileRows / 64;
  static_assert(POL::kIsStatic && kTileWords == 64, "one lane per bitmap word of a tile; straight-line predicate code");
  __shared__ uint32_t s_wave_cnt[NW];
  __shared__ uint64_t s_base;
  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  const int64_t n_words = (n + 63) >> 6;
  const int64_t n_tiles = (n + kTileRows - 1) / kTileRows;
  const int64_t n_units = (n_tiles + NW - 1) / NW;
  uint64_t* const state = sync + 2;
  uint64_t* const gstate = state + n_units;
  const uint64_t* __restrict__ in = (const uint64_t*)C.c[0].values;
  uint64_t* __restrict__ out = (uint64_t*)O.out[0];
  uint32_t err = 0;
  {
    for (int64_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {
      const int64_t tile = unit * NW + wave;
      const int64_t row0 = tile * kTileRows;
      const int64_t left = n - row0;  // rows of this tile (<= 0: a wave past the end of the batch: it reads row 0 and keeps nothing)
      const uint32_t last = left <= 0 ? 0u : (uint32_t)((left < (int64_t)kTileRows ? left : (int64_t)kTileRows) - 1);
      const uint64_t* base = in + (left <= 0 ? 0 : row0);
      // (opaque per super-tile: everything derived from the lane number alone -- 64 row indices, 64 lane == i masks -- is loop
      // invariant, and hoisted out of this loop it occupies 128 vector and 128 scalar registers for the kernel's whole life)
      uint32_t lv = (uint32_t)lane;
      asm volatile("" : "+v"(lv));
      const int32_t left_lane = (int32_t)(left >= (int64_t)kTileRows ? (int64_t)kTileRows : (left < 0 ? 0 : left)) - (int32_t)lv;
      uint64_t keep[kTileWords];
      if (left >= (int64_t)kTileRows) {  // (wave-uniform) a whole tile: one lane offset, the row group in the instruction's immediate
        const uint64_t* mine = base + lv;
#pragma unroll
        for (int i = 0; i < kTileWords; ++i) keep[i] = __builtin_nontemporal_load(mine + i * 64);
      } else {  // the batch's last tile (or none of it): unconditional loads of clamped rows, masked below
#pragma unroll
        for (int i = 0; i < kTileWords; ++i) {
          const uint32_t idx = (uint32_t)(i * 64) + lv;
          keep[i] = __builtin_nontemporal_load(base + (idx < last ? idx : last));
          __builtin_amdgcn_sched_barrier(0);  // (one index register at a time: 64 of them at once spill)
        }
      }
      uint32_t cnt = 0;
      uint32_t my_lo = 0, my_hi = 0;  // lane i: bitmap word i of the tile
#pragma unroll
      for (int i = 0; i < kTileWords; ++i) {
        const bool inb = (int32_t)(i * 64) < left_lane;
        COLV cur;
#pragma unroll
        for (int c = 0; c < BANK; ++c) cur[c] = keep[i];
        u64x16 reg;
        uint32_t rv = 0;
        POL::eval(P, F, cur, 0xFFFFFFFFu, reg, rv, inb, err);
        const bool pass = inb && POL::template pass_form<FORM>(P, F, pred, cur, 0xFFFFFFFFu, reg, rv);
        const uint64_t word = __ballot(pass);
        my_lo = lv == (uint32_t)i ? (uint32_t)word : my_lo;
        my_hi = lv == (uint32_t)i ? (uint32_t)(word >> 32) : my_hi;
        cnt += (uint32_t)__popcll(word);
        __builtin_amdgcn_sched_barrier(0);  // (one ballot at a time: the scheduler would keep all 64 SGPR pairs alive)
      }
      {
        const int64_t w = tile * kTileWords + lane;
        if (w < n_words) mask_words[w] = ((uint64_t)my_hi << 32) | my_lo;
      }
      if (lane == 0) s_wave_cnt[wave] = cnt;
      __syncthreads();
      uint32_t wc[NW];
      uint32_t A = 0;
#pragma unroll
      for (int k = 0; k < NW; ++k) {
        wc[k] = s_wave_cnt[k];
        A += wc[k];
      }
      if (wave == 0) filter_lookback(unit, n_units, n_tiles, A, state, gstate, sync, tile_offsets, ctrl, lane, &s_base, err);
      __syncthreads();
      uint64_t my_base = s_base;
#pragma unroll
      for (int k = 0; k < NW; ++k)
        if (k < wave) my_base += wc[k];
      if (lane == 0 && tile < n_tiles) tile_offsets[tile] = my_base;
      // (the output buffer holds O.cap_rows rows: what lies beyond is the host's to compact again)
      const uint32_t room = my_base >= O.cap_rows ? 0u : (O.cap_rows - my_base < (uint64_t)cnt ? (uint32_t)(O.cap_rows - my_base) : cnt);
      uint64_t* dst = out + my_base;
      uint32_t run_at = 0;  // (wave-uniform)
      const uint32_t lo = my_lo, hi = my_hi;
#pragma unroll
      for (int i = 0; i < kTileWords; ++i) {
        const uint64_t word = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)hi, i) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)lo, i);
        const uint32_t at = run_at + mbcnt_u64(word);
        if (((word >> lane) & 1ull) && at < room) dst[at] = keep[i];
        run_at += (uint32_t)__popcll(word);
        __builtin_amdgcn_sched_barrier(0);
      }
      // (the next super-tile's first barrier separates these reads of s_base / s_wave_cnt from their next writes)
    }
  }
  if (err) atomicOr(&ctrl[CTRL_ERROR], err);
}

// mask &= other, per-tile counts of the result: a predicate too large for one fused program is evaluated as several
// conjuncts (FilterRelation, dfx_filter.cpp); one wave per 64-word tile
__global__ __launch_bounds__(256) void k_mask_and_count(uint64_t* __restrict__ mask, const uint64_t* __restrict__ other,
                                                        uint32_t* __restrict__ tile_counts, const int64_t n_words,
                                                        const int64_t n_tiles) {
  const int lane = lane_id();
  const int64_t tile = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tile >= n_tiles) return;
  const int64_t w = tile * 64 + lane;
  uint64_t word = 0;
  if (w < n_words) {
    word = mask[w] & other[w];
    mask[w] = word;
  }
  uint32_t cnt = (uint32_t)__popcll(word);
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) cnt += (uint32_t)__shfl_xor((int)cnt, m, 64);
  if (lane == 0) tile_counts[tile] = cnt;
}
hipError_t launch_mask_and_count(uint64_t* mask, const uint64_t* other, uint32_t* tile_counts, int64_t n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  const int64_t n_words = (n + 63) / 64, n_tiles = (n + kTileRows - 1) / kTileRows;
  hipLaunchKernelGGL(k_mask_and_count, dim3((unsigned)((n_tiles + 3) / 4)), dim3(256), 0, s, mask, other, tile_counts, n_words, n_tiles);
  return hipGetLastError();
}


// ---------------------------------------------------------------------------------------------
// K4 compact
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kBlock) void k_compact(const T* __restrict__ in,
                                                    const uint64_t* __restrict__ mask_words,
                                                    const uint64_t* __restrict__ tile_offsets,
                                                    const int64_t n, T* __restrict__ out, const uint64_t out_limit) {
  __shared__ uint32_t word_off[64];
  const int lane = lane_id();
  const int wave = threadIdx.x >> 6;
  const int64_t n_words = (n + 63) >> 6;
  const int64_t n_tiles = (n + kTileRows - 1) / kTileRows;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    if (wave == 0) {  // popcount of each of the tile's 64 words, exclusive-scanned by one wave
      const int64_t w = tile * 64 + lane;
      const uint32_t c = w < n_words ? (uint32_t)__popcll(mask_words[w]) : 0u;
      const uint64_t inc = wave_inclusive_scan((uint64_t)c);
      word_off[lane] = (uint32_t)(inc - c);
    }
    __syncthreads();
    const uint64_t tile_base = tile_offsets[tile];
#pragma unroll 4
    for (int i = 0; i < 16; ++i) {
      const int wi = wave * 16 + i;
      const int64_t w = tile * 64 + wi;
      if (w < n_words) {
        const uint64_t word = mask_words[w];  // wave-uniform address: one request
        const int64_t row = w * 64 + lane;
        if ((word >> lane) & 1) {
          const uint32_t rank = (uint32_t)__popcll(word & ((1ull << lane) - 1ull));
          const uint64_t at = tile_base + word_off[wi] + rank;
          if (at < out_limit) out[at] = in[row];  // (emit sizes `out` from the host's group count before the scan's total is back)
        }
      }
    }
    __syncthreads();
  }
}

hipError_t launch_predicate_mask(const DevProgram& P, const DevFastPlan& fast, const DevColumns& C, uint8_t pred,
                                 int64_t n, uint64_t* mask_words, uint32_t* tile_counts, uint32_t* ctrl,
                                 double algo_bytes, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  Scope sc(KID_PREDICATE_MASK, s, algo_bytes);
  const int64_t tiles = (n + kTileRows - 1) / kTileRows;
  const int grid = stream_grid(tiles, 8);
  auto run = [&](auto pol) {
    hipLaunchKernelGGL((k_predicate_mask<typename decltype(pol)::type>), dim3(grid), dim3(kBlock), 0, s, P, fast, C, pred, n, mask_words, tile_counts, ctrl);
    return hipGetLastError();
  };
  const uint8_t none[kMaxAggs] = {0};
  switch (choose_row_source(ScanKernel::predicate_mask, P, fast, 0, 0, none, none, false, 0)) {
    case RowSource::sig_pred2_f64: return run(Policy<StaticPolicy<2, 8, SigPred2F64>>{});
    case RowSource::fast_c2: return run(Policy<FastPolicy<2, 8>>{});
    case RowSource::fast_c4: return run(Policy<FastPolicy<4, 4>>{});
    case RowSource::fast_c8: return run(Policy<FastPolicy<8, 2>>{});
    case RowSource::interp_c2: return run(Policy<InterpPolicy<2, 8>>{});
    case RowSource::interp_c4: return run(Policy<InterpPolicy<4, 4>>{});
    case RowSource::interp_c8: return run(Policy<InterpPolicy<8, 2>>{});
    default: return hipErrorNotSupported;  // (no other source in this kernel's ladder)
  }
}

template <typename POL>
static hipError_t filter_fused_launch(const DevProgram& P, const DevFastPlan& fast, const DevColumns& C, uint8_t pred, int64_t n,
                                      uint64_t* mask_words, uint64_t* tile_offsets, uint64_t* sync, const DevFusedOut& O,
                                      uint32_t* ctrl, hipStream_t s) {
  const size_t lds = (size_t)O.n * kFusedTiles * kFusedStage * sizeof(uint64_t);
  // the grid must be co-resident (the look-back waits for other workgroups): workgroups per CU from the occupancy API,
  // asked once per (policy, LDS size)
  // (one device per process -- ctx().device --; the cache is atomic: two threads that both miss compute the same answer)
  static std::atomic<int> per_cu[kFusedOutCols + 1];
  int wg_per_cu = per_cu[O.n].load(std::memory_order_relaxed);
  if (wg_per_cu == 0) {
    int nb = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_filter_fused<POL>, kBlock, lds);
    if (e != hipSuccess) return e;
    wg_per_cu = nb > 0 ? nb : 1;
    per_cu[O.n].store(wg_per_cu, std::memory_order_relaxed);
  }
  const int64_t tiles = (n + kTileRows - 1) / kTileRows;
  const int64_t units = (tiles + kFusedTiles - 1) / kFusedTiles;
  const int64_t cap = (int64_t)device_cu_count() * wg_per_cu;
  const int grid = (int)(units < cap ? units : cap);
  hipLaunchKernelGGL((k_filter_fused<POL>), dim3(grid), dim3(kBlock), lds, s, P, fast, C, pred, n, mask_words, tile_offsets, sync, O, ctrl);
  return hipGetLastError();
}

template <typename POL, int FORM>
static hipError_t filter_fused_dense_launch(const DevProgram& P, const DevFastPlan& fast, const DevColumns& C, uint8_t pred, int64_t n,
                                            uint64_t* mask_words, uint64_t* tile_offsets, uint64_t* sync, const DevFusedOut& O,
                                            uint32_t* ctrl, hipStream_t s) {
  static std::atomic<int> per_cu{0};  // (co-resident grid, as above)
  int wg_per_cu = per_cu.load(std::memory_order_relaxed);
  if (wg_per_cu == 0) {
    int nb = 0;
    hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_filter_fused_dense<POL, FORM>, kBlock, 0);
    if (e != hipSuccess) return e;
    wg_per_cu = nb > 0 ? nb : 1;
    per_cu.store(wg_per_cu, std::memory_order_relaxed);
  }
  const int64_t tiles = (n + kTileRows - 1) / kTileRows;
  const int64_t units = (tiles + kFusedTiles - 1) / kFusedTiles;
  const int64_t cap = (int64_t)device_cu_count() * wg_per_cu;
  const int grid = (int)(units < cap ? units : cap);
  hipLaunchKernelGGL((k_filter_fused_dense<POL, FORM>), dim3(grid), dim3(kBlock), 0, s, P, fast, C, pred, n, mask_words, tile_offsets, sync, O, ctrl);
  return hipGetLastError();
}

hipError_t launch_filter_fused(const DevProgram& P, const DevFastPlan& fast, const DevColumns& C, uint8_t pred, int64_t n,
                               uint64_t* mask_words, uint64_t* tile_offsets, uint64_t* sync, const DevFusedOut& O,
                               uint32_t* ctrl, double algo_bytes, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (O.n < 0 || O.n > kFusedOutCols) return hipErrorInvalidValue;
  Scope sc(KID_PREDICATE_MASK, s, algo_bytes);
  auto run = [&](auto pol) { return filter_fused_launch<typename decltype(pol)::type>(P, fast, C, pred, n, mask_words, tile_offsets, sync, O, ctrl, s); };
  const uint8_t none[kMaxAggs] = {0};
  switch (choose_row_source(ScanKernel::filter_fused, P, fast, 0, 0, none, none, false, 0)) {
    case RowSource::sig_pred2_f64: {
      // dense streams: the tile in registers, the column read once (the signature's one column is the one column compacted)
      const bool one_wide_column = P.n_cols == 1 && O.n == 1 && O.slot[0] == 0 && (O.dtype[0] == T_F64 || O.dtype[0] == T_I64 || O.dtype[0] == T_U64);
      typedef StaticPolicy<2, 8, SigPred2F64> POLD;
      if (!(O.dense && one_wide_column)) return run(Policy<POLD>{});
      auto dense = [&](auto form) { return filter_fused_dense_launch<POLD, decltype(form)::value>(P, fast, C, pred, n, mask_words, tile_offsets, sync, O, ctrl, s); };
      switch (POLD::form_of(fast)) {  // the comparison form is a template argument: one loop per kernel
        case 4 | (1 << 3): return dense(std::integral_constant<int, 4 | (1 << 3)>{});  // x >  a AND x <  b
        case 6 | (1 << 3): return dense(std::integral_constant<int, 6 | (1 << 3)>{});  // x >= a AND x <  b
        case 4 | (3 << 3): return dense(std::integral_constant<int, 4 | (3 << 3)>{});  // x >  a AND x <= b
        case 6 | (3 << 3): return dense(std::integral_constant<int, 6 | (3 << 3)>{});  // x >= a AND x <= b
        default: return dense(std::integral_constant<int, 0>{});
      }
    }
    case RowSource::fast_c2: return run(Policy<FastPolicy<2, 8>>{});
    case RowSource::fast_c4: return run(Policy<FastPolicy<4, 4>>{});
    case RowSource::fast_c8: return run(Policy<FastPolicy<8, 2>>{});
    case RowSource::interp_c2: return run(Policy<InterpPolicy<2, 8>>{});
    case RowSource::interp_c4: return run(Policy<InterpPolicy<4, 4>>{});
    case RowSource::interp_c8: return run(Policy<InterpPolicy<8, 2>>{});
    default: return hipErrorNotSupported;  // (no other source in this kernel's ladder)
  }
}

hipError_t launch_compact(const void* in, int width, const uint64_t* mask_words, const uint64_t* tile_offsets,
                          int64_t n, void* out, double algo_bytes, hipStream_t s, uint64_t out_limit) {
  if (n <= 0) return hipSuccess;
  Scope sc(KID_COMPACT, s, algo_bytes);
  const int64_t tiles = (n + kTileRows - 1) / kTileRows;
  const int grid = stream_grid(tiles, 8);
  switch (width) {
    case 8: hipLaunchKernelGGL(k_compact<uint64_t>, dim3(grid), dim3(kBlock), 0, s, (const uint64_t*)in, mask_words, tile_offsets, n, (uint64_t*)out, out_limit); break;
    case 4: hipLaunchKernelGGL(k_compact<uint32_t>, dim3(grid), dim3(kBlock), 0, s, (const uint32_t*)in, mask_words, tile_offsets, n, (uint32_t*)out, out_limit); break;
    case 2: hipLaunchKernelGGL(k_compact<uint16_t>, dim3(grid), dim3(kBlock), 0, s, (const uint16_t*)in, mask_words, tile_offsets, n, (uint16_t*)out, out_limit); break;
    case 1: hipLaunchKernelGGL(k_compact<uint8_t>, dim3(grid), dim3(kBlock), 0, s, (const uint8_t*)in, mask_words, tile_offsets, n, (uint8_t*)out, out_limit); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace dfx
