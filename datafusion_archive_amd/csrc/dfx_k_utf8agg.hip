// dfx_k_utf8agg.hip -- MIN / MAX of a Utf8 column (deviation D10: the planner types them, sqlplanner.rs:309-322, the executor
// panics on the downcast, aggregate.rs:561-603).
//
// MIN(x) per group is the minimum over the group's DISTINCT values of x, and the distinct set of (group key words, zero padding,
// dictionary id of x) is what COUNT_DISTINCT(x) of a Utf8 column already builds (dfx_distinct.cpp, dfx_k_distinct_inl.hpp).
// Nothing here runs per input row.  At emit
//
//   k_utf8_extrema_fold    walks the set's occupied slots (next to k_distinct_count): finds or creates the key prefix's entry in
//                          the extrema table (the count table's twin: same width, the argument word zeroed, two planes) and folds
//                          the tuple's id into the entry's two words, min id + 1 and max id + 1, 0 = nothing folded yet;
//   k_utf8_extrema_lookup  hands every group the inner aggregate emitted one of its two ids (the twin of k_distinct_lookup), with
//                          the validity bitmap of the column: word 0 = the group has no non-null argument.
//
// Ids are insertion-ordered, so they say nothing about the strings' order: the fold compares the strings themselves, straight
// out of the distinct side's dictionary (DevDict: offset, length, pool), with utf8_three_way (dfx_utf8_match.hpp: Rust `str`
// ordering, what the Lt / Gt string terms and the host use).  The dictionary is complete before the fold starts: plain loads.
#include "dfx_k_distinct_inl.hpp"

namespace dfx {

// Fold dictionary string `id` into *word (id + 1 of the best string so far, 0: none).  better: the three-way outcome that
// replaces the word, 1 (sorts before it: MIN) or 4 (after it: MAX).  The word is loaded plainly; a CAS is tried only when it is
// empty or the candidate is strictly better, and a failed CAS compares again with what it found there.  Every change of the word
// makes it strictly better, so a lane leaves the loop after finitely many trips whichever lane wins; no lane waits for another.
// Equal ids are equal strings (the dictionary holds each once): no bytes are compared.
DEV void utf8_extrema_fold_word(uint64_t* word, uint64_t id, const DevDict& D, uint32_t better) {
  const uint64_t mine = id + 1;
  const uint8_t* str = D.pool + D.str_off[id];
  const uint32_t len = D.str_len[id];
  uint64_t cur = __hip_atomic_load(word, RLX_AGENT);
  for (;;) {
    if (cur == mine) return;
    if (cur != 0ull && utf8_three_way(str, len, D.pool + D.str_off[cur - 1], D.str_len[cur - 1]) != better) return;
    const uint64_t old = atomicCAS((unsigned long long*)word, (unsigned long long)cur, (unsigned long long)mine);
    if (old == cur) return;
    cur = old;
  }
}

// One pass over the set's slots.  Grouped: Ex is keyed by the key prefix like the count table (sized so that it never fills:
// load <= 1/2, probing over the whole table; an insert that fails anyway sets bit 8 of its CTRL_ERROR).  Ungrouped (KW == 1): the
// prefix has no words and Ex is its single entry, accs[0] and accs[Ex.stride].  planes: bit 0 fold the minimum, bit 1 the
// maximum.  A tuple whose argument word is no id of the dictionary (n_ids: the ids it holds) sets bit 9 and is left out.
template <int KW>
__global__ __launch_bounds__(kBlock) void k_utf8_extrema_fold(const DevTable S, const DevTable Ex, const DevDict D, const uint64_t n_ids,
                                                              const uint32_t planes) {
  const int64_t n_slots = (int64_t)S.mask + 2;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n_slots; i += stride) {
    if (!distinct_slot_occupied<KW>(S, (uint64_t)i)) continue;
    // (slot `cap` of a one-word set belongs to the tuple that equals the claim sentinel: never an id)
    const uint64_t id = (KW == 1 && (uint64_t)i == S.mask + 1) ? kEmptyKey : S.keys[(uint64_t)(KW - 1) * S.stride + i];
    if (id >= n_ids) {
      atomicOr(&Ex.ctrl[CTRL_ERROR], 0x200u);
      continue;
    }
    uint64_t slot = 0;
    if (KW > 1) {
      uint64_t key[KW];
#pragma unroll
      for (int k = 0; k < KW - 1; ++k) key[k] = S.keys[(uint64_t)k * S.stride + i];
      key[KW - 1] = 0;
      bool inserted = false;
      if (!table_upsert_slot<KW>(Ex, key, hash_keys<KW>(key), slot, inserted)) {
        atomicOr(&Ex.ctrl[CTRL_ERROR], 0x100u);
        continue;
      }
    }
    if (planes & 1u) utf8_extrema_fold_word(&Ex.accs[slot], id, D, 1u);
    if (planes & 2u) utf8_extrema_fold_word(&Ex.accs[Ex.stride + slot], id, D, 4u);
  }
}

// emitted group keys -> plane `plane` (0 minimum, 1 maximum) of their entry as a dictionary id, and the column's validity: a group
// without an entry, or whose word is 0, is null and gets null_id (the id of the empty string: length 0, no bytes to gather).
// validity: (n + 63) / 64 words, bits past n zero; *nulls += null rows.  Ex is complete and quiescent: plain loads.
template <int KW>
__global__ __launch_bounds__(kBlock) void k_utf8_extrema_lookup(const DevTable Ex, const DevDistinctKeys K, const int kw_out, const int64_t n,
                                                                const int plane, const uint64_t null_id, uint64_t* __restrict__ ids,
                                                                uint64_t* __restrict__ validity, uint64_t* nulls) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  const int64_t n_pad = (n + 63) & ~63ll;  // whole waves: the ballot below is a validity word
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n_pad; i += stride) {
    uint64_t word = 0;
    if (i < n) {
      uint64_t slot = 0;
      bool found = KW == 1;
      if (KW > 1) {
        uint64_t key[KW];
        distinct_prefix_key<KW>(K, kw_out, i, key);
        found = distinct_prefix_find<KW>(Ex, key, slot);
      }
      if (found) word = Ex.accs[(uint64_t)plane * Ex.stride + slot];
      ids[i] = word ? word - 1 : null_id;
    }
    const uint64_t valid = __ballot(word != 0ull);
    if (lane_id() == 0) {
      const int64_t rows = n - i < 64 ? n - i : 64;
      validity[i >> 6] = valid;
      const uint64_t missing = (uint64_t)rows - (uint64_t)__popcll(valid);
      if (missing) atomicAdd((unsigned long long*)nulls, (unsigned long long)missing);
    }
  }
}

#define DFX_UTF8AGG_DISPATCH(kw, CALL)      \
  switch (kw) {                             \
    case 1: CALL(1); break;                 \
    case 2: CALL(2); break;                 \
    case 3: CALL(3); break;                 \
    case 4: CALL(4); break;                 \
    case 8: CALL(8); break;                 \
    default: return hipErrorInvalidValue;   \
  }

hipError_t launch_utf8_extrema_fold(const DevTable& S, const DevTable& Ex, const DevDict& D, uint64_t n_ids, uint32_t planes, hipStream_t s) {
  if (S.kw != Ex.kw || (planes & 3u) == 0u) return hipErrorInvalidValue;
  Scope sc(KID_UTF8_EXTREMA, s, 0);
  const int64_t n = (int64_t)S.mask + 2;
  const int grid = stream_grid((n + kBlock - 1) / kBlock, 8);
#define CALL(KW) hipLaunchKernelGGL(k_utf8_extrema_fold<KW>, dim3(grid), dim3(kBlock), 0, s, S, Ex, D, n_ids, planes)
  DFX_UTF8AGG_DISPATCH(S.kw, CALL)
#undef CALL
  return hipGetLastError();
}

hipError_t launch_utf8_extrema_lookup(const DevTable& Ex, const DevDistinctKeys& K, int kw_out, int64_t n, int plane, uint64_t null_id,
                                      uint64_t* ids, uint64_t* validity, uint64_t* nulls, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  if (plane < 0 || plane > 1 || (Ex.kw == 1 && n != 1)) return hipErrorInvalidValue;
  Scope sc(KID_UTF8_EXTREMA, s, 0);
  const int grid = stream_grid((n + kBlock - 1) / kBlock, 8);
#define CALL(KW) hipLaunchKernelGGL(k_utf8_extrema_lookup<KW>, dim3(grid), dim3(kBlock), 0, s, Ex, K, kw_out, n, plane, null_id, ids, validity, nulls)
  DFX_UTF8AGG_DISPATCH(Ex.kw, CALL)
#undef CALL
  return hipGetLastError();
}

}  // namespace dfx
