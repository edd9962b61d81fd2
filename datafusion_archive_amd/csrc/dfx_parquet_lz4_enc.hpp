// dfx_parquet_lz4_enc.hpp -- the rule by which the Parquet writer's "compression" option (deviation D13) packs a
// page body into one raw LZ4 block (Parquet codec 7, LZ4_RAW; the block format is in dfx_parquet_lz4.hpp, the reader's side), and the
// sequential host encoder of that rule.  ONE source for the kernel (dfx_k_parquet_write_lz4.hip: k_pqw_lz4, which reproduces the host
// encoder byte for byte), the host code (dfx_parquet_write.cpp: sizes only) and the CPU test
// (tests/native/parquet_lz4_write_check.cpp).  Free of HIP.
//
// The rule is shaped for a wave -- 64 positions looked at per step -- and is deterministic.  For a block of n input bytes:
//   bound     lz4_bound(n) = n + n / 255 + 16 bytes hold any block the rule makes
//   short     n < 13: one literal-only sequence (n == 0: the one-byte block {0x00}, a token of no literals: an empty block is not
//             a block to LZ4's own decoder)
//   table     4096 entries of position + 1, 0 = empty; hash = (le32(p) * 2654435761u) >> 20
//   step      anchor = cur = 0; while cur <= n - 12: the positions p_i = cur + i, i in 0 .. 63, p_i <= n - 12, each read their
//             candidate ref_i from the table AS IT STOOD BEFORE THE STEP.  A candidate holds when the entry is not empty, ref_i < p_i,
//             p_i - ref_i <= 65535 and le32(ref_i) == le32(p_i).  The pick is the lowest i whose candidate holds.  The positions up
//             to and including the pick (all of them without one) go into the table, each entry the maximum of its old value and
//             p + 1; the positions behind the pick do not (a later step would match a position against itself), nor do the positions
//             inside a match.  No pick: cur moves past the step.  A pick at s with reference r: the match is 4 bytes and every
//             following equal byte while s + len < n - 5; the sequence {literals [anchor, s), offset s - r, len} goes out and
//             anchor = cur = s + len.
//   end       one literal-only sequence [anchor, n)
// So the last 5 bytes of a block are literals and its last match starts 12 bytes or more before the end: LZ4's end-of-block rules,
// which other decoders enforce.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "dfx_parquet_rle.hpp"

namespace dfx {
namespace pqw {

constexpr int32_t kCodecUncompressed = 0, kCodecLz4Raw = 7;  // Parquet codec ids (pq::codec_name)
constexpr uint32_t kLz4TableEntries = 4096, kLz4HashShift = 20, kLz4HashMul = 2654435761u;
constexpr uint32_t kLz4Step = 64;         // positions looked at per step
constexpr uint32_t kLz4MinInput = 13;     // a shorter block is literals only
constexpr uint32_t kLz4LastMatch = 12;    // a match starts at n - 12 or before ...
constexpr uint32_t kLz4LastLiterals = 5;  // ... and ends at n - 5 or before
constexpr uint32_t kLz4MaxOffset = 65535;

DFX_PQ_HD bool compression_ok(int64_t codec) { return codec == kCodecUncompressed || codec == kCodecLz4Raw; }
DFX_PQ_HD uint64_t lz4_bound(uint64_t n) { return n + n / 255 + 16; }
// the i32 rule of a compressed page: the header holds the compressed size in an i32, and the block's bound must fit it
DFX_PQ_HD bool lz4_body_fits(uint64_t n) { return n <= 0x7FFFFFFFull && lz4_bound(n) <= 0x7FFFFFFFull; }
DFX_PQ_HD uint32_t lz4_hash(uint32_t word) { return (word * kLz4HashMul) >> kLz4HashShift; }
DFX_PQ_HD uint32_t lz4_le32(const uint8_t* p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
// does the table entry `entry` (position + 1; 0: empty) hold as the candidate of position p of `bytes`?
DFX_PQ_HD bool lz4_candidate_ok(uint64_t p, uint32_t entry, const uint8_t* bytes) {
  if (entry == 0) return false;
  const uint64_t ref = (uint64_t)entry - 1;
  return ref < p && p - ref <= kLz4MaxOffset && lz4_le32(bytes + ref) == lz4_le32(bytes + p);
}
// extension bytes of a length whose nibble is 15: each adds its value, a byte below 255 ends the chain
DFX_PQ_HD uint32_t lz4_ext_bytes(uint64_t len_minus_base) { return len_minus_base < 15 ? 0u : (uint32_t)((len_minus_base - 15) / 255 + 1); }
// byte k of the chain of lz4_ext_bytes(v) bytes
DFX_PQ_HD uint8_t lz4_ext_byte(uint64_t v, uint32_t k) { return k + 1 < lz4_ext_bytes(v) ? (uint8_t)255 : (uint8_t)((v - 15) % 255); }
// bytes of a sequence: token, literal extension, literals and, for a match (match_len >= 4), offset and match extension
DFX_PQ_HD uint64_t lz4_sequence_bytes(uint64_t lit, uint64_t match_len) {
  return 1 + lz4_ext_bytes(lit) + lit + (match_len ? 2 + lz4_ext_bytes(match_len - 4) : 0);
}

struct Lz4EncStats {  // (beside Lz4Stats, the decoder's)
  uint64_t sequences = 0, lit_extensions = 0, match_extensions = 0;
  uint64_t steps_without_pick = 0;
};

// one sequence at out[pos ...]; match_len 0: the last, literals only.  Returns the bytes stored (lz4_sequence_bytes).
inline uint64_t lz4_put_sequence(uint8_t* out, const uint8_t* lits, uint64_t lit, uint32_t offset, uint64_t match_len, Lz4EncStats* stats) {
  const uint64_t ml = match_len ? match_len - 4 : 0;
  uint64_t o = 0;
  out[o++] = (uint8_t)((lit < 15 ? lit : 15) << 4 | (ml < 15 ? ml : 15));
  for (uint32_t k = 0; k < lz4_ext_bytes(lit); ++k) out[o++] = lz4_ext_byte(lit, k);
  if (lit) memcpy(out + o, lits, (size_t)lit);
  o += lit;
  if (match_len) {
    out[o++] = (uint8_t)(offset & 0xFF);
    out[o++] = (uint8_t)(offset >> 8);
    for (uint32_t k = 0; k < lz4_ext_bytes(ml); ++k) out[o++] = lz4_ext_byte(ml, k);
  }
  if (stats) {
    ++stats->sequences;
    stats->lit_extensions += lz4_ext_bytes(lit);
    stats->match_extensions += match_len ? lz4_ext_bytes(ml) : 0;
  }
  return o;
}

// the sequential encoder: [src, src + n) -> one block at dst, which has room for lz4_bound(n) bytes; returns the block's length
inline uint64_t lz4_encode_block(const uint8_t* src, uint64_t n, uint8_t* dst, Lz4EncStats* stats = nullptr) {
  uint64_t anchor = 0, op = 0;
  if (n >= kLz4MinInput) {
    std::vector<uint32_t> table(kLz4TableEntries, 0u);
    const uint64_t last = n - kLz4LastMatch;  // the last position a match may start at
    uint64_t cur = 0;
    while (cur <= last) {
      const uint64_t left = last - cur + 1;
      const uint32_t count = (uint32_t)(left < kLz4Step ? left : kLz4Step);
      uint32_t pick = count;
      for (uint32_t i = 0; i < count && pick == count; ++i)
        if (lz4_candidate_ok(cur + i, table[lz4_hash(lz4_le32(src + cur + i))], src)) pick = i;
      const uint64_t ref = pick < count ? (uint64_t)table[lz4_hash(lz4_le32(src + cur + pick))] - 1 : 0;  // (read before the step's inserts)
      for (uint32_t i = 0; i < count && i <= pick; ++i) {
        uint32_t& e = table[lz4_hash(lz4_le32(src + cur + i))];
        if (e < (uint32_t)(cur + i + 1)) e = (uint32_t)(cur + i + 1);
      }
      if (pick == count) {
        cur += count;
        if (stats) ++stats->steps_without_pick;
        continue;
      }
      const uint64_t s = cur + pick;
      uint64_t len = 4;
      while (s + len < n - kLz4LastLiterals && src[ref + len] == src[s + len]) ++len;
      op += lz4_put_sequence(dst + op, src + anchor, s - anchor, (uint32_t)(s - ref), len, stats);
      anchor = cur = s + len;
    }
  }
  op += lz4_put_sequence(dst + op, src + anchor, n - anchor, 0, 0, stats);
  return op;
}

}  // namespace pqw
}  // namespace dfx
