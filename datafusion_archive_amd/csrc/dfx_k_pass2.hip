// dfx_k_pass2.hip -- pass 2 of the partitioned GROUP BY (the strategy: dfx_k_partition_inl.hpp): the flat-index kernel
// k_partition_agg, the streaming kernel k_partition_agg_lean with its row forms, and launch_partition_agg.  Which form a launch
// takes, with how much LDS and in how many launches, is choose_pass2 (dfx_pass2_forms.hpp, tested on the CPU).  The same kernel
// scans a window of a table's routed shadow and evaluates the predicate itself (launch_partition_scan, choose_pass2_scan).  build.py's guard
// of the hand-scheduled row registers compiles this unit a second time, to assembly.
#include "dfx_k_partition_ws_inl.hpp"
#include "dfx_pass2_forms.hpp"

namespace dfx {

static_assert(kABlock / 64 == kP2Waves, "choose_pass2 sizes the parked-row queues for the workgroup's waves");

// pass 2: one workgroup per partition (= table block).  The rows of all producers are visited as
// ONE flattened index space (prefix sums of the per-producer counts live in LDS), so all lanes stay
// busy however small the individual regions are.  Global loads are issued RU rows ahead of the LDS
// probing (the kernel is latency-bound otherwise: 16 waves, one dependent load each).
template <int NA1>  // NA1 == 1: one aggregate (16-byte rows); 0: any
__global__ __launch_bounds__(kABlock) void k_partition_agg(const DevTable T, const DevPartition PT, const DevRows spill) {
  extern __shared__ __attribute__((aligned(16))) uint64_t lds[];
  __shared__ uint32_t wave_tot[kABlock / 64];
  constexpr int RU = NA1 ? 4 : 2;
  constexpr int NV = NA1 ? 1 : kMaxAggs;
  const uint32_t S = T.block_mask + 1;
  const int NW = (int)PT.n_words;
  uint64_t* lkeys = lds;
  uint64_t* laccs = lds + S;
  uint32_t* pre = (uint32_t*)(lds + (size_t)S * NW);  // [n_producers + 1] exclusive prefix of counts
  const uint32_t p = blockIdx.x;
  const uint64_t slot0 = (uint64_t)p * S;
  const int lane = lane_id();
  // block -> LDS, 16-byte loads, all loads of a plane in flight before the LDS writes (S is a power of two >= 2)
  for (int w = 0; w < NW; ++w) {
    const uint64_t* src = (w == 0 ? T.keys : T.accs + (uint64_t)(w - 1) * T.stride) + slot0;
    uint64_t* dst = lds + (size_t)w * S;
    for (uint32_t i0 = threadIdx.x * 2; i0 < S; i0 += kABlock * 2 * 4) {
      const uint32_t ia = i0, ib = i0 + kABlock * 2, ic = i0 + kABlock * 4, id = i0 + kABlock * 6;
      const ulonglong2 ta = *(const ulonglong2*)(src + (ia < S ? ia : 0));  // clamped: all four loads in flight together
      const ulonglong2 tb = *(const ulonglong2*)(src + (ib < S ? ib : 0));
      const ulonglong2 tc = *(const ulonglong2*)(src + (ic < S ? ic : 0));
      const ulonglong2 td = *(const ulonglong2*)(src + (id < S ? id : 0));
      if (ia < S) *(ulonglong2*)(dst + ia) = ta;
      if (ib < S) *(ulonglong2*)(dst + ib) = tb;
      if (ic < S) *(ulonglong2*)(dst + ic) = tc;
      if (id < S) *(ulonglong2*)(dst + id) = td;
    }
  }
  // exclusive scan of the producer counts (n_producers <= 1024: one per thread)
  const uint32_t NP = PT.n_producers;
  const uint32_t c0 = threadIdx.x < NP ? PT.counts[(uint64_t)p * NP + threadIdx.x] : 0u;
  uint32_t inc = c0;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(inc, d, 64);
    if (lane >= d) inc += o;
  }
  if (lane == 63) wave_tot[threadIdx.x >> 6] = inc;
  __syncthreads();
  uint32_t base = 0, total = 0;
#pragma unroll
  for (int w = 0; w < kABlock / 64; ++w) {
    if (w < (int)(threadIdx.x >> 6)) base += wave_tot[w];
    total += wave_tot[w];
  }
  if (threadIdx.x < NP) pre[threadIdx.x] = base + inc - c0;
  if (threadIdx.x == 0) pre[NP] = total;
  __syncthreads();
  uint32_t new_keys = 0;
  // software pipeline: the rows of trip t + 1 are loaded while trip t probes the LDS block
  const float inv = total ? (float)NP / (float)total : 0.f;
  uint64_t key[RU][1], nkey[RU][1];
  uint64_t val[RU][NV], nval[RU][NV];
  bool inb[RU], ninb[RU];
  auto row_of = [&](uint32_t i) -> const uint64_t* {  // flattened row i: the producers' counts are near-uniform, so interpolate and correct
    uint32_t lo = (uint32_t)((float)i * inv);
    if (lo >= NP) lo = NP - 1;
    while (pre[lo] > i) --lo;
    while (pre[lo + 1] <= i) ++lo;
    return region_row(PT, p, lo, i - pre[lo]);
  };
  auto fetch = [&](uint32_t i0, uint64_t (&k)[RU][1], uint64_t (&v)[RU][NV], bool (&ib)[RU]) {
#pragma unroll
    for (int r = 0; r < RU; ++r) {
      const uint32_t i = i0 + (uint32_t)r * kABlock + threadIdx.x;
      ib[r] = i < total;
      k[r][0] = 0;
#pragma unroll
      for (int a = 0; a < NV; ++a) v[r][a] = 0;
      if (NA1) {
        // unconditional load (idle lanes re-read the partition's first row): a branch around it makes the compiler
        // wait with vmcnt(0) -- a full memory round trip per trip -- instead of counting the loads in flight
        const uint64_t* src = PT.rows + (uint64_t)p * PT.part_stride;
        if (ib[r]) src = row_of(i);
        typedef uint64_t u64x2_t __attribute__((ext_vector_type(2)));
        const u64x2_t kv = __builtin_nontemporal_load((const u64x2_t*)src);
        ib[r] = ib[r] && kv.x != kEmptyKey;  // padding rows (pass 1 rounds every region up to whole chunks)
        k[r][0] = ib[r] ? kv.x : 0ull;
        v[r][0] = ib[r] ? kv.y : 0ull;
      } else if (ib[r]) {
        const uint64_t* src = row_of(i);
        k[r][0] = src[0];
#pragma unroll
        for (int a = 0; a < NV; ++a)
          if (a < T.na) v[r][a] = src[1 + a];
        if (k[r][0] == kEmptyKey) ib[r] = false;  // padding row
      }
    }
  };
  fetch(0, nkey, nval, ninb);
  for (uint32_t i0 = 0; i0 < total; i0 += kABlock * RU) {  // wave-uniform trip count
#pragma unroll
    for (int r = 0; r < RU; ++r) {
      key[r][0] = nkey[r][0];
      inb[r] = ninb[r];
#pragma unroll
      for (int a = 0; a < NV; ++a) val[r][a] = nval[r][a];
    }
    if (i0 + kABlock * RU < total) fetch(i0 + kABlock * RU, nkey, nval, ninb);
#pragma unroll
    for (int r = 0; r < RU; ++r) {
      bool todo = inb[r];
      if (inb[r]) {
        const uint64_t h = hash_keys<1>(key[r]);
        const uint32_t slot = (uint32_t)((h >> T.shift) & T.mask) & T.block_mask;
        int found = -1;
        // Linear probing, FOUR slots per step (two 16-byte LDS reads of the aligned group): a wave pays for
        // the longest probe sequence among its 64 lanes.  The home slot is the group base (table_upsert_slot),
        // so the probe ORDER is exactly home, home + 1, ... and the block stays a valid linear-probing table for
        // the global kernels; most lookups end in the first group.
        uint32_t g = slot >> 2;
        for (uint32_t it = 0; it <= (S >> 2) && found < 0;) {
          const ulonglong2 ka = *(const ulonglong2*)&lkeys[g * 4];
          const ulonglong2 kb = *(const ulonglong2*)&lkeys[g * 4 + 2];
          const uint64_t kk = key[r][0];
          const uint32_t mm = (ka.x == kk ? 1u : 0u) | (ka.y == kk ? 2u : 0u) | (kb.x == kk ? 4u : 0u) | (kb.y == kk ? 8u : 0u);
          const uint32_t em = (ka.x == kEmptyKey ? 1u : 0u) | (ka.y == kEmptyKey ? 2u : 0u) | (kb.x == kEmptyKey ? 4u : 0u) | (kb.y == kEmptyKey ? 8u : 0u);
          if (mm) {
            found = (int)(g * 4 + (uint32_t)__ffs((int)mm) - 1u);
          } else if (em) {
            const uint32_t at = g * 4 + (uint32_t)__ffs((int)em) - 1u;
            const uint64_t old = atomicCAS((unsigned long long*)&lkeys[at], (unsigned long long)kEmptyKey, (unsigned long long)kk);
            if (old == kEmptyKey) {
              found = (int)at;
              ++new_keys;
            } else if (old == kk) {
              found = (int)at;
            }  // else: another key claimed it meanwhile -- look at the same group again
          } else {
            g = (g + 1) & ((S >> 2) - 1);
            ++it;
          }
        }
        if (found >= 0) {
#pragma unroll
          for (int a = 0; a < NV; ++a)
            if (a < T.na) acc_atomic(T.acc_kind[a], &laccs[(size_t)a * S + found], val[r][a]);
          todo = false;
        }
      }
      if (__ballot(todo) != 0) {  // block full: grow-and-replay takes the row
        uint64_t sv[kMaxAggs];
#pragma unroll
        for (int a = 0; a < kMaxAggs; ++a) sv[a] = a < NV ? val[r][a < NV ? a : 0] : 0;
        spill_row<1>(T, spill, todo, key[r], sv);
      }
    }
  }
  __syncthreads();
  for (int w = 0; w < NW; ++w) {
    uint64_t* dst = (w == 0 ? T.keys : T.accs + (uint64_t)(w - 1) * T.stride) + slot0;
    const uint64_t* src = lds + (size_t)w * S;
    for (uint32_t i = threadIdx.x * 2; i < S; i += kABlock * 2) *(ulonglong2*)(dst + i) = *(const ulonglong2*)(src + i);
  }
#pragma unroll
  for (int mm = 32; mm >= 1; mm >>= 1) new_keys += __shfl_xor(new_keys, mm, 64);
  if (lane == 0 && new_keys) atomicAdd(&T.ctrl[CTRL_OCCUPIED], new_keys);
  if (p == 0 && threadIdx.x == 0) __hip_atomic_store(&T.ctrl[CTRL_MAX_FILL], 0u, RLX_AGENT);  // the regions are empty again
  snapshot_ctrl_if_last(T, PT);
}

// ---- pass 2, streaming form --------------------------------------------------------------------------------
// What round 2 measured about the kernel above (and two rewrites of it): 4.9 us per million routed rows + ~20 us per
// launch WHATEVER the row width (16 / 12 bytes), the hash (3 multiplies / none), the LDS traffic per probe (32 / 16
// bytes) or the depth of the row prefetch -- 1.3 us per 64-row trip and wave.  The disassembly says why: ~110 vector,
// ~180 scalar and ~45 branch instructions per trip (divergent find-or-claim with its EXEC bookkeeping, a run-time switch
// over the accumulator kind, spill checks, 64-bit address arithmetic).  A wave issues one instruction at a time and a
// SIMD one scalar instruction per cycle across its four waves: the loop is bound by instruction ISSUE, mostly scalar.
//
// k_partition_agg_lean is the same algorithm with a short common path:
//   * a WAVE walks whole regions (wave w owns the regions of producers w, w + 16, ...; their row counts sit in one VGPR,
//     lane j = producer w + 16 j, read back with v_readlane), so a row's address is a scalar base + lane * row bytes;
//   * the accumulator kind is a template parameter;
//   * FAST PATH, branch-free: the row's home group of four slots is read (one 16-byte LDS read of 32-bit tags, or two of
//     64-bit keys), four compares, the matching slot picked with v_cndmask, one LDS atomic under the match mask.  In a
//     table that has seen its keys (every batch but the first) 96 % of the rows end here;
//   * a row whose home group does not hold its key (it lives further along the probe sequence, or is new, or the block is
//     full) is parked in a per-wave LDS queue; up to 64 parked rows at a time take the general find-or-claim (same probe
//     order as the global kernels: the block stays a valid linear-probing table) at full lane utilisation;
//   * the row loads of kPF trips are in flight per wave.  The compiler tracks vector-memory results with ONE in-order
//     counter (vmcnt) and is pessimistic after conditional code that contains memory operations, so the loads are
//     issued by inline assembly into VGPRs v88..v119, which the kernel withholds from the register allocator
//     (amdgpu_num_vgpr(88)): nothing the compiler generates can read or reuse them while a load is in flight, and
//     `s_waitcnt vmcnt(kPF - 1)` + v_mov hands a landed row over.  (A first version let the compiler allocate those
//     registers and tied them through the wait with a "+v" constraint; it copied half of an in-flight row BEFORE the wait.)
// Narrow rows (PTF_NARROW): 12-byte rows {hash image, operand}; the LDS block holds 32-bit TAGS instead of keys: tag = hash
// image of the slot's key (a bijection for keys below 2^32, see ring_route), kTagEmpty for an empty slot, kTagForeign for
// a slot whose key has no image (>= 2^32, inserted by the general path: occupied, never equal to a row's image).  12
// bytes per slot: 96 KB of LDS instead of 128; claimed tags become keys again at write-back.
// Padding rows (pass 1 rounds every region up to whole chunks: key kEmptyKey / image kTagEmpty) are skipped.
//
// The ROW FORM of a launch -- the bytes a lane loads and what the launch does with the operand -- is a policy type, one per
// Pass2Rows (dfx_pass2_forms.hpp).  PTF_PAIR (two operand columns, 20-byte routed rows): a launch aggregates ONE operand into one
// accumulator plane and loads only that operand's twelve bytes -- {operand lo, operand hi, image} for operand 0 (kOperandFirst),
// {image, operand} for operand 1, like any narrow row.  kPlaneXform (PTF_PLANES, with or without PTF_PAIR): the operand travels
// RAW and the launch applies its plane's transform.
template <uint32_t ROW_BYTES, bool TAGS, bool OPERAND_FIRST, bool PLANE_XFORM>
struct RowForm {
  static constexpr uint32_t kRowBytes = ROW_BYTES;
  static constexpr bool kTags = TAGS;                   // the LDS block holds 32-bit tags, not keys
  static constexpr bool kOperandFirst = OPERAND_FIRST;  // {operand lo, operand hi, image}, not {image, operand}
  static constexpr bool kPlaneXform = PLANE_XFORM;      // apply the plane's transform to the raw operand
};
typedef RowForm<16u, false, false, false> RowsWide;    // {key, operand}
typedef RowForm<12u, true, false, false> RowsNarrow;   // {image, operand}
typedef RowForm<12u, true, true, false> RowsPair0;     // {operand lo, operand hi, image}
typedef RowForm<12u, true, false, true> RowsNarrowXf;  // {image, raw operand}
typedef RowForm<12u, true, true, true> RowsPair0Xf;    // {raw operand lo, hi, image}
// PTF_ROW8: {image, Float32 bits of the operand} -- 64 contiguous rows per trip, one 8-byte load per lane; the decode widens the bits
// (shadow_widen: the value the 12-byte row would have carried), so parked rows, the atomic and the spill list see narrow's row
typedef RowForm<8u, true, false, false> RowsNarrow8;

// The in-flight rows: kPF slots of four registers, outside the register allocator's reach.  The kernel is compiled for
// kP2Vgprs registers, slot D owns the four that follow: v(kP2Vgprs + 4 D) ... -- v88..v119, which build.py's guard looks for.
constexpr int kPF = 8;
constexpr int kP2Vgprs = 88;
#define DFX_P2_SLOTS(X)                                                                                        \
  X(0, 88, 89, 90, 91) X(1, 92, 93, 94, 95) X(2, 96, 97, 98, 99) X(3, 100, 101, 102, 103) X(4, 104, 105, 106, 107) \
  X(5, 108, 109, 110, 111) X(6, 112, 113, 114, 115) X(7, 116, 117, 118, 119)
#define X(D, A, B, C, E) static_assert(D < kPF && A == kP2Vgprs + 4 * D && B == A + 1 && C == A + 2 && E == A + 3, "slot D = v(kP2Vgprs + 4 D) and the next three");
DFX_P2_SLOTS(X)
#undef X
static_assert(kPF == 8, "eight row slots in the list");
struct Row4 { uint32_t x, y, z, w; };
template <int D, uint32_t ROW_BYTES>
DEV void p2_issue(uint32_t voff, const void* base) {  // slot D <- the lane's 8, 12 or 16 bytes at base + voff
#define X(SLOT, A, B, C, E)                                                                                                                          \
  if constexpr (D == SLOT && ROW_BYTES == 8u) asm volatile("global_load_dwordx2 v[" #A ":" #B "], %0, %1 nt" ::"v"(voff), "s"(base) : "memory", "v" #A, "v" #B); \
  if constexpr (D == SLOT && ROW_BYTES == 12u) asm volatile("global_load_dwordx3 v[" #A ":" #C "], %0, %1 nt" ::"v"(voff), "s"(base) : "memory", "v" #A, "v" #B, "v" #C); \
  if constexpr (D == SLOT && ROW_BYTES == 16u) asm volatile("global_load_dwordx4 v[" #A ":" #E "], %0, %1 nt" ::"v"(voff), "s"(base) : "memory", "v" #A, "v" #B, "v" #C, "v" #E);
  DFX_P2_SLOTS(X)
#undef X
}
template <int D, uint32_t ROW_BYTES, int N>
DEV void p2_take(Row4& r) {  // waits until at most N younger loads are in flight, then copies slot D out
  if constexpr (ROW_BYTES == 12u) r.w = 0;
  if constexpr (ROW_BYTES == 8u) r.z = 0, r.w = 0;
#define X(SLOT, A, B, C, E)                                                                                                          \
  if constexpr (D == SLOT && ROW_BYTES == 8u)                                                                                        \
    asm volatile("s_waitcnt vmcnt(%2)\n\tv_mov_b32 %0, v" #A "\n\tv_mov_b32 %1, v" #B : "=v"(r.x), "=v"(r.y) : "n"(N) : "memory"); \
  if constexpr (D == SLOT && ROW_BYTES == 12u)                                                                                       \
    asm volatile("s_waitcnt vmcnt(%3)\n\tv_mov_b32 %0, v" #A "\n\tv_mov_b32 %1, v" #B "\n\tv_mov_b32 %2, v" #C : "=v"(r.x), "=v"(r.y), "=v"(r.z) : "n"(N) : "memory"); \
  if constexpr (D == SLOT && ROW_BYTES == 16u)                                                                                       \
    asm volatile("s_waitcnt vmcnt(%4)\n\tv_mov_b32 %0, v" #A "\n\tv_mov_b32 %1, v" #B "\n\tv_mov_b32 %2, v" #C "\n\tv_mov_b32 %3, v" #E \
                 : "=v"(r.x), "=v"(r.y), "=v"(r.z), "=v"(r.w) : "n"(N) : "memory");
  DFX_P2_SLOTS(X)
#undef X
}
DEV void p2_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// The general find-or-claim in an LDS block of S slots, over 64-bit keys or 32-bit tags: linear probing from the row's home
// group, FOUR slots per step (the aligned group: two 16-byte LDS reads of keys, one of tags).  Returns the slot, -1: the block is
// full.  k_partition_agg holds the same probe order inline: called from there, this function cost k_partition_agg<1> 58
// instructions and two more spilled SGPRs.
struct Keys4 { ulonglong2 a, b; };
DEV Keys4 p2_load4(const uint64_t* l) { return {*(const ulonglong2*)l, *(const ulonglong2*)(l + 2)}; }
DEV uint4 p2_load4(const uint32_t* l) { return *(const uint4*)l; }
DEV uint32_t p2_eq4(const Keys4& k, uint64_t x) { return (k.a.x == x ? 1u : 0u) | (k.a.y == x ? 2u : 0u) | (k.b.x == x ? 4u : 0u) | (k.b.y == x ? 8u : 0u); }
DEV uint32_t p2_eq4(const uint4& t, uint32_t x) { return (t.x == x ? 1u : 0u) | (t.y == x ? 2u : 0u) | (t.z == x ? 4u : 0u) | (t.w == x ? 8u : 0u); }
DEV uint64_t p2_cas(uint64_t* at, uint64_t expect, uint64_t x) { return atomicCAS((unsigned long long*)at, (unsigned long long)expect, (unsigned long long)x); }
DEV uint32_t p2_cas(uint32_t* at, uint32_t expect, uint32_t x) { return atomicCAS(at, expect, x); }
template <typename W>
DEV int p2_find_or_claim(W* block, uint32_t S, uint32_t slot, W x, W empty, uint32_t& new_keys) {
  uint32_t g = slot >> 2;
  for (uint32_t it = 0; it <= (S >> 2);) {
    const auto four = p2_load4(&block[g * 4]);
    const uint32_t mm = p2_eq4(four, x);
    if (mm) return (int)(g * 4 + (uint32_t)__ffs((int)mm) - 1u);
    const uint32_t em = p2_eq4(four, empty);
    if (em) {
      const uint32_t at = g * 4 + (uint32_t)__ffs((int)em) - 1u;
      const W old = p2_cas(&block[at], empty, x);
      if (old == empty) {
        ++new_keys;
        return (int)at;
      }
      if (old == x) return (int)at;
      continue;  // another key claimed it meanwhile -- look at the same group again
    }
    g = (g + 1) & ((S >> 2) - 1);
    ++it;
  }
  return -1;
}

// branch-free look at ONE aligned group of four slots.  The LDS read and the compare are separate steps so that the
// reads of two rows can be issued together; p2_pin keeps the compiler from sinking a read under the condition its
// result is used in (it would then wait for each read on its own).
struct Group4 {
  uint4 t;           // tags: four of them
  ulonglong2 ka, kb; // keys: four of them
};
template <bool TAGS>
DEV void p2_read_group(const uint32_t* ltags, const uint64_t* lkeys, uint32_t slot4, Group4& g) {
  if (TAGS) {
    g.t = *(const uint4*)&ltags[slot4];
  } else {
    g.ka = *(const ulonglong2*)&lkeys[slot4];
    g.kb = *(const ulonglong2*)&lkeys[slot4 + 2];
  }
}
template <bool TAGS>
DEV void p2_pin(Group4& a, Group4& b) {
  if (TAGS) {
    asm volatile("" : "+v"(a.t.x), "+v"(a.t.y), "+v"(a.t.z), "+v"(a.t.w), "+v"(b.t.x), "+v"(b.t.y), "+v"(b.t.z), "+v"(b.t.w));
  } else {
    asm volatile("" : "+v"(a.ka.x), "+v"(a.ka.y), "+v"(a.kb.x), "+v"(a.kb.y), "+v"(b.ka.x), "+v"(b.ka.y), "+v"(b.kb.x), "+v"(b.kb.y));
  }
}
template <bool TAGS>
DEV int p2_match(const Group4& g, uint32_t img, uint64_t kk) {
  int idx = -1;
  if (TAGS) {
    idx = g.t.w == img ? 3 : idx;
    idx = g.t.z == img ? 2 : idx;
    idx = g.t.y == img ? 1 : idx;
    idx = g.t.x == img ? 0 : idx;
  } else {
    idx = g.kb.y == kk ? 3 : idx;
    idx = g.kb.x == kk ? 2 : idx;
    idx = g.ka.y == kk ? 1 : idx;
    idx = g.ka.x == kk ? 0 : idx;
  }
  return idx;
}

// The two rows' tag compares of look2 as ONE block (narrow rows).  The compiler's form is v_cmp -> vcc, s_nop 1, v_cndmask, four
// times per row and row after row: a VALU read of a lane mask needs two wait states behind the VALU that wrote it, so eight
// s_nop per pair of trips (5 % of the loop's issue slots).  Here the two rows' compares alternate and go to four scalar pairs,
// every select reads a mask written at least three instructions earlier: sixteen instructions, no wait states.
// idx = the first of the group's four tags that equals the row's image, -1 if none.
#ifndef DFX_P2_ASM_MATCH
#define DFX_P2_ASM_MATCH 1
#endif
DEV void p2_match2_narrow(const uint4& a, uint32_t img0, const uint4& b, uint32_t img1, int& i0, int& i1) {
  uint64_t mA, mB, mC, mD;
  int x0, x1;
  asm volatile(
      "v_cmp_eq_u32_e64 %[mA], %[aw], %[g0]\n\t"
      "v_cmp_eq_u32_e64 %[mB], %[bw], %[g1]\n\t"
      "v_cmp_eq_u32_e64 %[mC], %[az], %[g0]\n\t"
      "v_cmp_eq_u32_e64 %[mD], %[bz], %[g1]\n\t"
      "v_cndmask_b32_e64 %[x0], -1, 3, %[mA]\n\t"
      "v_cndmask_b32_e64 %[x1], -1, 3, %[mB]\n\t"
      "v_cmp_eq_u32_e64 %[mA], %[ay], %[g0]\n\t"
      "v_cmp_eq_u32_e64 %[mB], %[by], %[g1]\n\t"
      "v_cndmask_b32_e64 %[x0], %[x0], 2, %[mC]\n\t"
      "v_cndmask_b32_e64 %[x1], %[x1], 2, %[mD]\n\t"
      "v_cmp_eq_u32_e64 %[mC], %[ax], %[g0]\n\t"
      "v_cmp_eq_u32_e64 %[mD], %[bx], %[g1]\n\t"
      "v_cndmask_b32_e64 %[x0], %[x0], 1, %[mA]\n\t"
      "v_cndmask_b32_e64 %[x1], %[x1], 1, %[mB]\n\t"
      "v_cndmask_b32_e64 %[x0], %[x0], 0, %[mC]\n\t"
      "v_cndmask_b32_e64 %[x1], %[x1], 0, %[mD]"
      : [mA] "=&s"(mA), [mB] "=&s"(mB), [mC] "=&s"(mC), [mD] "=&s"(mD), [x0] "=&v"(x0), [x1] "=&v"(x1)
      : [ax] "v"(a.x), [ay] "v"(a.y), [az] "v"(a.z), [aw] "v"(a.w), [bx] "v"(b.x), [by] "v"(b.y), [bz] "v"(b.z), [bw] "v"(b.w),
        [g0] "v"(img0), [g1] "v"(img1));
  i0 = x0;
  i1 = x1;
}

// Pass2Rows::narrow8_pred (SCAN != kP2ScanNone): the regions are a window of a table's ROUTED SHADOW (dfx_routed_shadow.hpp) -- every
// row of 2^27 consecutive table rows, routed once by a dense pass 1, read-only here -- and the query's predicate is evaluated in THIS
// kernel: per trip the operand is widened (shadow_widen) and compared as Float64 with the query's literals, exactly the comparison
// the Val4 scan policies make, and the passing rows are compacted (ballot + mbcnt) into a per-wave LDS ring of kP2StageRows rows.
// Whenever the ring holds 128 rows, two full batches of it take the path below (decode, look2, apply, park); the remainder when
// the wave's regions end.  SCAN: kP2ScanRuntime the operators are read from `pred`; kP2ScanAll no predicate; else the two terms'
// three-way masks as compile-time constants (m0 | m1 << 3, as pass 1's FORM).
template <int M>
DEV bool p2_cmp_ct(double a, double b) {
  if constexpr (M == 1) return a < b;
  else if constexpr (M == 2) return a == b;
  else if constexpr (M == 3) return a <= b;
  else if constexpr (M == 4) return a > b;
  else if constexpr (M == 5) return a < b || a > b;
  else return a >= b;
}
DEV uint64_t p2_cmp_rt(double a, double b, uint32_t m, uint32_t inv) {  // (cmp_mask_by<double> ^ inv: the scan policies' run-time term)
  const uint64_t lt = __ballot(a < b), eq = __ballot(a == b), gt = __ballot(a > b);
  return (((m & 1u) ? lt : 0ull) | ((m & 2u) ? eq : 0ull) | ((m & 4u) ? gt : 0ull)) ^ (inv ? ~0ull : 0ull);
}

// ROWS: the row form (above).  KIND: the accumulator kind (ACC_*).  SHARED_OPERAND (PTF_SHARED; KIND is not read): T.na
// (2..kSharedMaxAggs) aggregates of ONE operand -- the row carries the raw operand, every aggregate applies its own transform
// and atomic to it (kinds and transforms are wave-uniform kernel arguments).
template <typename ROWS, int KIND, bool SHARED_OPERAND = false, int SCAN = kP2ScanNone>
__global__ __launch_bounds__(kABlock) __attribute__((amdgpu_num_vgpr(kP2Vgprs))) void k_partition_agg_lean(const DevTable T, const DevPartition PT,
                                                                                                             const DevRows spill, const DevRowPred pred) {
  extern __shared__ __attribute__((aligned(16))) uint64_t lds[];
  static_assert(!SHARED_OPERAND || ROWS::kTags, "shared-operand rows are narrow rows");
  static_assert(ROWS::kTags ? (ROWS::kRowBytes == 12u || (ROWS::kRowBytes == 8u && !ROWS::kOperandFirst && !ROWS::kPlaneXform && !SHARED_OPERAND))
                            : (ROWS::kRowBytes == 16u && !ROWS::kOperandFirst && !ROWS::kPlaneXform),
                "the six row forms");
  static_assert(SCAN == kP2ScanNone || (ROWS::kRowBytes == 8u && KIND == ACC_ADD_F64), "the scan over a routed shadow reads 8-byte rows and adds");
  const uint32_t NA = SHARED_OPERAND ? (uint32_t)T.na : 1u;
  const uint32_t S = T.block_mask + 1;
  // PTF_PAIR (two aggregates of different operands, 20-byte routed rows): this launch aggregates operand / accumulator plane
  // PT.pair_plane -- the block holds the tags and THAT plane, the row's other operand is not even loaded.  Plane 0's twelve bytes
  // are {operand lo, operand hi, image} (ROWS::kOperandFirst); plane 1 reads {image, operand} like any narrow row.
  // PTF_PLANES (ROWS::kPlaneXform: one launch per accumulator plane): the operand is RAW; this launch applies plane
  // PT.pair_plane's transform to it and aggregates into that plane.
  const bool pair = ROWS::kTags && !SHARED_OPERAND && (PT.flags & PTF_PAIR) != 0;  // (20-byte rows)
  const bool per_plane = pair || ROWS::kPlaneXform;
  const uint32_t plane = per_plane ? PT.pair_plane : 0u;
  const uint32_t last_plane = per_plane ? (uint32_t)T.na - 1u : 0u;
  const uint8_t plane_xf = ROWS::kPlaneXform ? (uint8_t)PT.plane_xf : (uint8_t)VT_RAW;  // (a scalar from the launcher: no kernel-argument array is indexed at run time)
  uint64_t* const t_accs = T.accs + (uint64_t)plane * T.stride;
  // wide: keys[S] accs[S]; narrow: accs[NA][S] tags[S]
  uint64_t* lkeys = lds;
  uint64_t* laccs = ROWS::kTags ? lds : lds + S;
  uint32_t* ltags = (uint32_t*)(lds + (size_t)(ROWS::kTags ? NA : 1u) * S);
  auto apply = [&](uint32_t at, uint64_t val) {  // (ROWS::kPlaneXform: `val` is the RAW operand -- this plane's transform here, so that a row that ends in the spill list still has it raw)
    if constexpr (ROWS::kPlaneXform) val = transform_value(plane_xf, val, true);
    if constexpr (SHARED_OPERAND) {
#pragma unroll
      for (uint32_t a = 0; a < (uint32_t)kSharedMaxAggs; ++a)
        if (a < NA) acc_atomic(T.acc_kind[a], &laccs[(size_t)a * S + at], transform_value(T.val_xform[a], val, true));
    } else {
      acc_atomic((uint8_t)KIND, &laccs[at], val);
    }
  };
  const uint32_t p = blockIdx.x;
  const uint64_t slot0 = (uint64_t)p * S;
  const int lane = lane_id();
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t NP = PT.n_producers;
  // this wave's regions: producer wave + 16 j lives in lane j
  const uint32_t my_prod = wave + (uint32_t)(kABlock / 64) * (uint32_t)lane;
  const uint32_t v_cnt = my_prod < NP ? PT.counts[(uint64_t)p * NP + my_prod] : 0u;
  // table block -> LDS
  for (uint32_t i0 = threadIdx.x * 2; i0 < S; i0 += kABlock * 2) {
    const ulonglong2 kk = *(const ulonglong2*)(T.keys + slot0 + i0);
    for (uint32_t a = 0; a < NA; ++a)
      *(ulonglong2*)(laccs + (size_t)a * S + i0) = *(const ulonglong2*)(t_accs + (uint64_t)a * T.stride + slot0 + i0);
    if (ROWS::kTags) {
      uint32_t tg[2];
      const uint64_t k2[2] = {kk.x, kk.y};
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        uint64_t key1[1] = {k2[j]};
        const uint32_t im = (uint32_t)(hash_keys<1>(key1) >> 32);
        tg[j] = k2[j] == kEmptyKey ? kTagEmpty : (((k2[j] >> 32) != 0 || im >= kTagForeign) ? kTagForeign : im);
      }
      *(uint2*)(ltags + i0) = make_uint2(tg[0], tg[1]);
    } else {
      *(ulonglong2*)(lkeys + i0) = kk;
    }
  }
  p2_drain();  // (the block's loads have landed anyway; from here on vmcnt belongs to the row loads below)
  // wave-uniform cursor: region ordinal, rows left in it, address of the next trip's first row
  const uint8_t* const part_bytes = (const uint8_t*)(PT.rows + (uint64_t)p * PT.part_stride);
  const uint64_t prod_bytes = PT.prod_stride * 8ull;
  const uint64_t win_bytes = PT.win_stride * 8ull;  // from one 64-row trip of a region to the next
  const uint8_t* const safe_ptr = part_bytes + (uint64_t)wave * prod_bytes;  // always a readable trip (>= 64 rows per region)
  const uint32_t n_mine = (NP + (uint32_t)(kABlock / 64) - 1u - wave) / (uint32_t)(kABlock / 64);  // regions of this wave
  uint32_t s_j = 0;
  uint32_t s_rem = (uint32_t)__builtin_amdgcn_readlane((int)v_cnt, 0);
  const uint8_t* s_ptr = safe_ptr;
  // LINE chunks (PTF_CHUNK16 with kNarrowLine, dfx_device.hpp): a trip is six 128-byte lines of ten rows -- lane L < 60 reads row
  // L % 10 of line L / 10 --, else 64 contiguous rows; 768 bytes either way
  // (8-byte rows, PTF_ROW8: sixteen to a line with no padding -- 64 contiguous rows like any other trip)
  const bool line_chunks = ROWS::kTags && ROWS::kRowBytes == 12u && kNarrowLine && (PT.flags & PTF_CHUNK16) != 0;
  const uint32_t trip_rows = line_chunks ? (uint32_t)kNarrowTripRows : 64u;  // (PTF_PAIR: ten lines of six rows = 60 as well)
  static_assert(kPairTripRows == kNarrowTripRows || !kNarrowLine, "one trip length for both line geometries");
  const uint32_t pair_off = (pair && PT.pair_operand != 0u) ? 8u : 0u;  // operand 1's twelve bytes start at the image
  const uint32_t voff = pair ? ((uint32_t)lane / (uint32_t)kPairChunkRows) * 128u + ((uint32_t)lane % (uint32_t)kPairChunkRows) * (4u * kPairRowDwords) + pair_off
                        : line_chunks ? ((uint32_t)lane / 10u) * 128u + ((uint32_t)lane % 10u) * 12u
                                      : (uint32_t)lane * ROWS::kRowBytes;  // (lanes past the trip's rows re-read its first row: measured 11 % over-fetch otherwise)
  uint32_t take[kPF];
  uint64_t s_win = win_bytes;  // (0 once the wave's regions are exhausted: the remaining loads of the pipeline re-read safe_ptr)
  auto advance = [&]() -> uint32_t {  // rows of the next trip (0: exhausted); leaves its address in s_ptr
    if (s_rem == 0) {  // the next region that holds rows -- off the common path
      while (s_rem == 0 && s_j < n_mine) {
        ++s_j;
        if (s_j < n_mine) {
          s_rem = (uint32_t)__builtin_amdgcn_readlane((int)v_cnt, (int)(s_j & 63u));
          s_ptr = part_bytes + (uint64_t)(wave + (uint32_t)(kABlock / 64) * s_j) * prod_bytes;
        }
      }
      if (s_rem == 0) {
        s_ptr = safe_ptr;
        s_win = 0;
      }
    }
    return s_rem < trip_rows ? s_rem : trip_rows;
  };
#define DFX_P2_FETCH(D)                                                   \
  {                                                                       \
    const uint32_t tk = advance();                                        \
    take[D] = tk;                                                         \
    p2_issue<D, ROWS::kRowBytes>((uint32_t)lane < tk ? voff : pair_off, (const void*)s_ptr);                         \
    s_ptr += s_win;                                                       \
    s_rem -= tk;                                                          \
  }
  DFX_P2_FETCH(0) DFX_P2_FETCH(1) DFX_P2_FETCH(2) DFX_P2_FETCH(3) DFX_P2_FETCH(4) DFX_P2_FETCH(5) DFX_P2_FETCH(6) DFX_P2_FETCH(7)
  static_assert(kPF == 8, "eight row slots");
  __syncthreads();  // the block is in LDS
  uint32_t new_keys = 0;
  const int tag_shift = T.shift - 32;                 // narrow: slot = image >> tag_shift (the image is the hash's high half)
  const uint32_t mask4 = T.block_mask & ~3u;          // home slot = base of the aligned group of four
  bool more = true;
  // TWO trips are probed together: their home-group reads (and, when needed, their next-group reads) are in flight at
  // the same time, so a wave exposes one LDS round trip per pair of trips instead of one per trip (with 4 waves per SIMD
  // the probe loop was bound by that latency: 3.9 us per million rows whatever the instruction count).
  struct Probe {
    uint64_t val, kk;
    uint32_t home4, img;
    int j;  // after look2: the row's slot within its home group (0..3), -1: a row whose key is not there (parked), 4: not a row
    bool real;
  };
  auto decode = [&](const Row4& r, uint32_t tk, Probe& q) {
    const bool inb = (uint32_t)lane < tk;
    if (ROWS::kOperandFirst) {  // {operand lo, operand hi, image}
      q.val = ((uint64_t)r.y << 32) | r.x;
      q.img = r.z;
      q.kk = 0;
      q.real = inb && r.z != kTagEmpty;
      q.home4 = (uint32_t)(r.z >> tag_shift) & mask4;
    } else if (ROWS::kRowBytes == 8u) {  // {image, Float32 bits}: exactly the operand's Float64 bits again
      q.val = shadow_widen(r.y);
      q.img = r.x;
      q.kk = 0;
      q.real = inb && r.x != kTagEmpty;
      q.home4 = (uint32_t)(r.x >> tag_shift) & mask4;
    } else if (ROWS::kTags) {
      q.val = ((uint64_t)r.z << 32) | r.y;
      q.img = r.x;
      q.kk = 0;
      q.real = inb && r.x != kTagEmpty;
      q.home4 = (uint32_t)(r.x >> tag_shift) & mask4;
    } else {
      q.kk = ((uint64_t)r.y << 32) | r.x;
      q.val = ((uint64_t)r.w << 32) | r.z;
      q.img = 0;
      q.real = inb && q.kk != kEmptyKey;
      uint64_t key1[1] = {q.kk};
      q.home4 = (uint32_t)(hash_keys<1>(key1) >> T.shift) & mask4;
    }
    q.j = 4;
  };
  auto look2 = [&](Probe& q0, uint32_t g0, Probe& q1, uint32_t g1) {  // both rows' groups: two LDS reads in flight, then the compares
    Group4 a, b;
    p2_read_group<ROWS::kTags>(ltags, lkeys, g0, a);
    p2_read_group<ROWS::kTags>(ltags, lkeys, g1, b);
    int i0, i1;
    if constexpr (ROWS::kTags && DFX_P2_ASM_MATCH != 0) {
      p2_match2_narrow(a.t, q0.img, b.t, q1.img, i0, i1);  // (also pins both reads in front of the compares)
    } else {
      p2_pin<ROWS::kTags>(a, b);
      i0 = p2_match<ROWS::kTags>(a, q0.img, q0.kk);
      i1 = p2_match<ROWS::kTags>(b, q1.img, q1.kk);
    }
    // hit and miss are then ONE compare each on j (a bool that is the AND of two lane masks costs a v_cndmask + v_cmp to ballot)
    q0.j = q0.real ? i0 : 4;
    q1.j = q1.real ? i1 : 4;
  };
  // Rows whose home group does not hold their key (4 % at load 0.5, every row of a block's first batch) are parked in a
  // per-wave LDS queue and go through the general find-or-claim up to 64 at a time.  Handling them in place costs the
  // WHOLE wave a second group look on 99.5 % of the trip pairs (1 - 0.96^128) and the divergent general path on a third
  // of them: more than half of the kernel's vector instructions for 4 % of the rows (pass 2: -20 %).
  constexpr uint32_t kRQ = ROWS::kTags ? (uint32_t)kP2RetryRows : (uint32_t)kP2RetryRowsWide;  // rows per wave
  constexpr uint32_t kRW = ROWS::kTags ? 3u : 4u;  // words per parked row: {image | key lo, key hi} + {operand lo, operand hi}
  uint32_t* const rq = (ROWS::kTags ? (uint32_t*)(ltags + S) : (uint32_t*)(lds + 2 * (size_t)S)) + (size_t)wave * kRQ * kRW;
  uint32_t rqn = 0;  // queued rows (wave-uniform)
  auto retry = [&](bool active, uint32_t at) {  // one queued row per active lane
    uint32_t img = 0;
    uint64_t kk = 0, val = 0;
    if (active) {
      if (ROWS::kTags) {
        img = rq[at * kRW];
      } else {
        kk = ((uint64_t)rq[at * kRW + 1] << 32) | rq[at * kRW];
      }
      val = ((uint64_t)rq[at * kRW + kRW - 1] << 32) | rq[at * kRW + kRW - 2];
    }
    bool todo = active;
    if (active) {
      int found;
      if (ROWS::kTags) {
        found = p2_find_or_claim<uint32_t>(ltags, S, (uint32_t)(img >> tag_shift) & mask4, img, kTagEmpty, new_keys);
      } else {
        uint64_t key1[1] = {kk};
        found = p2_find_or_claim<uint64_t>(lkeys, S, (uint32_t)(hash_keys<1>(key1) >> T.shift) & mask4, kk, kEmptyKey, new_keys);
      }
      if (found >= 0) {
        apply((uint32_t)found, val);
        todo = false;
      }
    }
    if (__ballot(todo) != 0 && (!per_plane || PT.plane_spills != 0u)) {  // block full: grow-and-replay takes the row (as a key again)
      // one launch per plane: only the LAST plane of an operand spills -- the block is as full for every plane, so the others fail on
      // exactly these rows -- and it writes every accumulator of its operand (raw operand: each one's transform; the pair of two
      // aggregates: the one value the scan transformed), the other operand's accumulators get their identity (adding it is a no-op)
      uint64_t key[1] = {ROWS::kTags ? (uint64_t)unhash_word32(img) : kk};
      uint64_t sv[kMaxAggs];
#pragma unroll
      for (int j = 0; j < kMaxAggs; ++j) {
        if (SHARED_OPERAND) {
          sv[j] = (uint32_t)j < NA ? transform_value(T.val_xform[j], val, true) : 0ull;
        } else if (per_plane) {
          const bool mine = pair ? ((PT.pair_ops >> j) & 1u) == PT.pair_operand : true;  // (planes of a shared operand: every accumulator)
          sv[j] = j >= T.na ? 0ull : !mine ? T.acc_init[j] : ROWS::kPlaneXform ? transform_value(T.val_xform[j], val, true) : val;
        } else {
          sv[j] = j == 0 ? val : 0ull;
        }
      }
      spill_row<1>(T, spill, todo, key, sv);
    }
  };
  auto park = [&](const Probe& q) {
    const uint64_t m = __ballot(q.j < 0);
    if (m != 0) {
      if (q.j < 0) {
        const uint32_t at = rqn + mbcnt64(m);
        if (ROWS::kTags) {
          rq[at * kRW] = q.img;
        } else {
          rq[at * kRW] = (uint32_t)q.kk;
          rq[at * kRW + 1] = (uint32_t)(q.kk >> 32);
        }
        rq[at * kRW + kRW - 2] = (uint32_t)q.val;
        rq[at * kRW + kRW - 1] = (uint32_t)(q.val >> 32);
      }
      rqn += (uint32_t)__popcll(m);
      // at most kRQ - 64 rows may stay queued: the next trip parks up to 64 more
      while (rqn > kRQ - 64u) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const uint32_t take_n = rqn < 64u ? rqn : 64u;
        rqn -= take_n;
        retry((uint32_t)lane < take_n, rqn + (uint32_t)lane);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      }
    }
  };
  auto process2 = [&](const Row4& r0, uint32_t tk0, const Row4& r1, uint32_t tk1) {
    Probe q0, q1;
    decode(r0, tk0, q0);
    decode(r1, tk1, q1);
    look2(q0, q0.home4, q1, q1.home4);
    if ((uint32_t)q0.j < 4u) apply(q0.home4 + (uint32_t)q0.j, q0.val);
    if ((uint32_t)q1.j < 4u) apply(q1.home4 + (uint32_t)q1.j, q1.val);
    park(q0);
    park(q1);
  };
  // the scan's stage: a ring of kP2StageRows rows {image, Float32 bits} per wave, behind the parked-row queues
  uint32_t* const stage = (uint32_t*)(ltags + S) + (size_t)kP2Waves * kRQ * kRW + (size_t)wave * (uint32_t)kP2StageRows * 2u;
  uint32_t st_head = 0, st_n = 0;  // (wave-uniform)
  uint64_t passed = 0;
  auto stage_at = [&](uint32_t i) -> uint32_t* {  // row i behind the ring's head
    uint32_t at = st_head + i;
    at = at >= (uint32_t)kP2StageRows ? at - (uint32_t)kP2StageRows : at;
    return stage + at * 2u;
  };
  auto drain2 = [&](uint32_t tk0, uint32_t tk1) __attribute__((always_inline)) {  // the ring's first rows as two batches (lanes past tk read rows nobody uses)
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    const uint2 a = *(const uint2*)stage_at((uint32_t)lane);
    const uint2 b = *(const uint2*)stage_at(64u + (uint32_t)lane);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    const uint32_t took = tk0 + tk1;
    st_head += took;
    st_head = st_head >= (uint32_t)kP2StageRows ? st_head - (uint32_t)kP2StageRows : st_head;
    st_n -= took;
    const Row4 r0 = {a.x, a.y, 0u, 0u}, r1 = {b.x, b.y, 0u, 0u};
    process2(r0, tk0, r1, tk1);
  };
  auto scan1 = [&](const Row4& r, uint32_t tk) __attribute__((always_inline)) {
    uint64_t pm = __ballot((uint32_t)lane < tk && r.x != kTagEmpty);
    if constexpr (SCAN == kP2ScanRuntime) {
      const double x = as_f64(shadow_widen(r.y));
      if (pred.np > 0u) pm &= p2_cmp_rt(x, as_f64(pred.imm[0]), pred.m[0], pred.inv[0]);
      if (pred.np > 1u) pm &= p2_cmp_rt(x, as_f64(pred.imm[1]), pred.m[1], pred.inv[1]);
    } else if constexpr (SCAN != kP2ScanAll) {
      const double x = as_f64(shadow_widen(r.y));
      pm &= __ballot(p2_cmp_ct<(SCAN & 7)>(x, as_f64(pred.imm[0])));
      pm &= __ballot(p2_cmp_ct<((SCAN >> 3) & 7)>(x, as_f64(pred.imm[1])));
    }
    if (pm != 0) {
      if (lane_of_mask(pm)) *(uint2*)stage_at(st_n + mbcnt64(pm)) = make_uint2(r.x, r.y);
      const uint32_t c = (uint32_t)__popcll(pm);
      st_n += c;
      passed += c;
      if (st_n >= 128u) drain2(64u, 64u);
    }
  };
#define DFX_P2_PAIR(D0, D1)                                                                                       \
  if (more) {                                                                                                     \
    const uint32_t tk0 = take[D0], tk1 = take[D1];                                                                \
    if (tk0 == 0) {                                                                                               \
      more = false;                                                                                               \
    } else {                                                                                                      \
      Row4 r0, r1;                                                                                                \
      p2_take<D0, ROWS::kRowBytes, kPF - 1>(r0);                                                                           \
      p2_take<D1, ROWS::kRowBytes, kPF - 2>(r1);                                                                           \
      DFX_P2_FETCH(D0)                                                                                            \
      DFX_P2_FETCH(D1)                                                                                            \
      process2(r0, tk0, r1, tk1);                                                                                 \
      if (tk1 == 0) more = false;                                                                                 \
    }                                                                                                             \
  }
  if constexpr (SCAN == kP2ScanNone) {
    while (more) {
      DFX_P2_PAIR(0, 1) DFX_P2_PAIR(2, 3) DFX_P2_PAIR(4, 5) DFX_P2_PAIR(6, 7)
    }
  } else {
    // The scan: the four slot pairs are the cases of ONE loop body (a scalar switch per pair of trips), so the stage, and behind it
    // process2 with its parked-row path, exist once per trip of the pair and not once per slot: unrolled over the eight slots the
    // kernel was eight copies of all of it.
    uint32_t phase = 0;
    while (more) {
      Row4 r0 = {0u, 0u, 0u, 0u}, r1 = {0u, 0u, 0u, 0u};
      uint32_t tk0 = 0, tk1 = 0;
#define DFX_P2_TAKE2(D0, D1)                        \
  {                                                 \
    tk0 = take[D0], tk1 = take[D1];                 \
    if (tk0 != 0) {                                 \
      p2_take<D0, ROWS::kRowBytes, kPF - 1>(r0);    \
      p2_take<D1, ROWS::kRowBytes, kPF - 2>(r1);    \
      DFX_P2_FETCH(D0)                              \
      DFX_P2_FETCH(D1)                              \
    }                                               \
  }
      switch (phase) {
        case 0: DFX_P2_TAKE2(0, 1) break;
        case 1: DFX_P2_TAKE2(2, 3) break;
        case 2: DFX_P2_TAKE2(4, 5) break;
        default: DFX_P2_TAKE2(6, 7) break;
      }
#undef DFX_P2_TAKE2
      phase = (phase + 1u) & 3u;
      if (tk0 == 0) {
        more = false;
      } else {
        scan1(r0, tk0);
        scan1(r1, tk1);
        if (tk1 == 0) more = false;
      }
    }
  }
#undef DFX_P2_PAIR
#undef DFX_P2_FETCH
  if constexpr (SCAN != kP2ScanNone) {
    if (st_n != 0) drain2(st_n < 64u ? st_n : 64u, st_n > 64u ? st_n - 64u : 0u);  // the ring's last rows (fewer than 128)
    if (lane == 0) stat_add(T, STAT_PASSED, passed);                              // (the scanners of pass 1 count them otherwise)
  }
  if (rqn != 0) {  // the wave's last parked rows (at most kRQ - 64 <= 64)
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    retry((uint32_t)lane < rqn, (uint32_t)lane);
  }
  p2_drain();  // loads still in flight own v88..v119 until they land
  // The key plane goes back only if this block claimed a slot: after a table's first window every key is there already, and
  // the narrow form's write-back is 8-byte stores into every other slot (load 0.5) -- partial lines, 8 MB per launch at 10^6 groups.
  const bool claimed = __syncthreads_or(new_keys != 0) != 0;
  for (uint32_t i0 = threadIdx.x * 2; i0 < S; i0 += kABlock * 2) {
    for (uint32_t a = 0; a < NA; ++a)
      *(ulonglong2*)(t_accs + (uint64_t)a * T.stride + slot0 + i0) = *(const ulonglong2*)(laccs + (size_t)a * S + i0);
    if (!claimed) continue;
    if (ROWS::kTags) {
      const uint2 tg = *(const uint2*)(ltags + i0);
      // a tag that is an image is written back as its key (unchanged for slots that held it before, new for claimed
      // ones); empty and foreign slots keep what the table holds
      if (tg.x < kTagForeign) T.keys[slot0 + i0] = (uint64_t)unhash_word32(tg.x);
      if (tg.y < kTagForeign) T.keys[slot0 + i0 + 1] = (uint64_t)unhash_word32(tg.y);
    } else {
      *(ulonglong2*)(T.keys + slot0 + i0) = *(const ulonglong2*)(lkeys + i0);
    }
  }
#pragma unroll
  for (int mm = 32; mm >= 1; mm >>= 1) new_keys += __shfl_xor(new_keys, mm, 64);
  if (lane == 0 && new_keys) atomicAdd(&T.ctrl[CTRL_OCCUPIED], new_keys);
  if (per_plane && plane != last_plane) return;  // (the last plane's launch reads the same regions: it is the one that ends the window)
  // (a routed shadow is read-only: its counts stand, its regions are never "empty again")
  if (SCAN == kP2ScanNone && p == 0 && threadIdx.x == 0) __hip_atomic_store(&T.ctrl[CTRL_MAX_FILL], 0u, RLX_AGENT);  // the regions are empty again
  snapshot_ctrl_if_last(T, PT);
}

template <typename ROWS>
static void launch_agg_lean(const DevTable& T, const DevPartition& PT, const DevRows& spill, size_t lds_bytes, hipStream_t s, int plane) {
#define DFX_LEAN(K) hipLaunchKernelGGL((k_partition_agg_lean<ROWS, K>), dim3(PT.n_parts), dim3(kABlock), lds_bytes, s, T, PT, spill, DevRowPred{})
  switch (T.acc_kind[plane]) {
    case ACC_ADD_F64: DFX_LEAN(ACC_ADD_F64); break;
    case ACC_ADD_F32: DFX_LEAN(ACC_ADD_F32); break;
    case ACC_ADD_U64: DFX_LEAN(ACC_ADD_U64); break;
    case ACC_MIN_S64: DFX_LEAN(ACC_MIN_S64); break;
    case ACC_MAX_S64: DFX_LEAN(ACC_MAX_S64); break;
    case ACC_MIN_U64: DFX_LEAN(ACC_MIN_U64); break;
    default: DFX_LEAN(ACC_MAX_U64); break;
  }
#undef DFX_LEAN
}

hipError_t launch_partition_agg(const DevTable& T, const DevPartition& PT, const DevRows& spill, double algo_bytes,
                                hipStream_t s) {
  Scope sc(KID_PARTITION_AGG, s, algo_bytes);
  const Pass2Choice c = choose_pass2(PT.flags, T.na, T.kw, PT.n_words, T.block_mask + 1, PT.n_producers, PT.pair_ops, kNarrowLine);
  if (c.form == Pass2Form::refused) return hipErrorInvalidValue;
  const dim3 grid(PT.n_parts), block(kABlock);
  for (int a = 0; a < c.n_launches; ++a) {
    const Pass2Launch& l = c.launch[a];
    DevPartition Pa = PT;
    if (pass2_per_plane(c.form)) {  // launch a aggregates accumulator plane a
      Pa.pair_plane = (uint32_t)a;
      Pa.plane_xf = T.val_xform[a];
      Pa.plane_spills = l.plane_spills;
      if (pass2_is_pair(c.form)) Pa.pair_operand = l.operand;
      if (!l.keeps_snap) Pa.snap_host = nullptr;
    }
    if (c.form == Pass2Form::flat_one) {
      hipLaunchKernelGGL(k_partition_agg<1>, grid, block, c.lds_bytes, s, T, Pa, spill);
    } else if (c.form == Pass2Form::flat_any) {
      hipLaunchKernelGGL(k_partition_agg<0>, grid, block, c.lds_bytes, s, T, Pa, spill);
    } else if (c.form == Pass2Form::shared_operand) {
      hipLaunchKernelGGL((k_partition_agg_lean<RowsNarrow, ACC_ADD_F64, true>), grid, block, c.lds_bytes, s, T, Pa, spill, DevRowPred{});
    } else {
      switch (l.rows) {  // x the plane's accumulator kind
        case Pass2Rows::wide: launch_agg_lean<RowsWide>(T, Pa, spill, c.lds_bytes, s, a); break;
        case Pass2Rows::narrow: launch_agg_lean<RowsNarrow>(T, Pa, spill, c.lds_bytes, s, a); break;
        case Pass2Rows::pair0: launch_agg_lean<RowsPair0>(T, Pa, spill, c.lds_bytes, s, a); break;
        case Pass2Rows::narrow_xf: launch_agg_lean<RowsNarrowXf>(T, Pa, spill, c.lds_bytes, s, a); break;
        case Pass2Rows::pair0_xf: launch_agg_lean<RowsPair0Xf>(T, Pa, spill, c.lds_bytes, s, a); break;
        case Pass2Rows::narrow8_pred: return hipErrorInvalidValue;  // (launch_partition_scan's: choose_pass2 never names it)
        case Pass2Rows::narrow8:  // (only the two SUM signatures bind both shadows: one accumulator kind)
          if (T.acc_kind[a] != ACC_ADD_F64) return hipErrorInvalidValue;
          hipLaunchKernelGGL((k_partition_agg_lean<RowsNarrow8, ACC_ADD_F64>), grid, block, c.lds_bytes, s, T, Pa, spill, DevRowPred{});
          break;
      }
    }
  }
  return hipGetLastError();
}

// One window of a routed shadow (dfx_routed_shadow.hpp) through the scan form: PT describes the window's regions and counts, pred
// the query's predicate over the operand.  Which kernel, with how much LDS, is choose_pass2_scan (dfx_pass2_forms.hpp).
hipError_t launch_partition_scan(const DevTable& T, const DevPartition& PT, const DevRows& spill, const DevRowPred& pred, double algo_bytes,
                                 hipStream_t s) {
  Scope sc(KID_PARTITION_AGG, s, algo_bytes);
  const Pass2ScanChoice c = choose_pass2_scan(PT.flags, T.na, T.kw, T.acc_kind[0] == ACC_ADD_F64, T.block_mask + 1, PT.n_producers, kNarrowLine, pred.np, pred.m[0],
                                              pred.inv[0], pred.m[1], pred.inv[1]);
  if (c.rows != Pass2Rows::narrow8_pred) return hipErrorInvalidValue;
  const dim3 grid(PT.n_parts), block(kABlock);
#define DFX_SCAN(SCAN_) hipLaunchKernelGGL((k_partition_agg_lean<RowsNarrow8, ACC_ADD_F64, false, SCAN_>), grid, block, c.lds_bytes, s, T, PT, spill, pred)
  switch (c.scan) {
    case kP2ScanAll: DFX_SCAN(kP2ScanAll); break;
    case 4 | (1 << 3): DFX_SCAN(4 | (1 << 3)); break;  // x >  a AND x <  b
    case 6 | (1 << 3): DFX_SCAN(6 | (1 << 3)); break;  // x >= a AND x <  b
    case 4 | (3 << 3): DFX_SCAN(4 | (3 << 3)); break;  // x >  a AND x <= b
    case 6 | (3 << 3): DFX_SCAN(6 | (3 << 3)); break;  // x >= a AND x <= b
    default: DFX_SCAN(kP2ScanRuntime); break;
  }
#undef DFX_SCAN
  return hipGetLastError();
}

}  // namespace dfx
