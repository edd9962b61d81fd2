// dfx_parquet_lz4.hpp -- the inflate stage of the Parquet source (deviation D12): the table the host hands the device, one entry
// per page of a compressed column chunk, and the parser of a raw LZ4 block (Parquet codec 7, LZ4_RAW: one block per page body, no
// frame, no length prefix, no checksum).  ONE source for the kernel (dfx_k_parquet.hip: k_pq_inflate), the sequential host decoder
// below (what tests/native/parquet_lz4_check.cpp holds against pyarrow) and the relation (dfx_parquet.cpp).  Free of HIP.
//
//   block    := sequence* last
//   sequence := token lit-ext* literals offset match-ext*      last := token lit-ext* literals
//   token: high nibble = literal length, low nibble = match length - 4; a nibble of 15 is continued by bytes that each add their
//   value, a byte below 255 ending the chain.  offset: 2 bytes little-endian, 1 .. 65535, back from the match's first output byte;
//   a match may overlap its own output (offset < length): byte i of it is byte (i mod offset) of the `offset` bytes before it.
//
// Bounds rules (the same on both sides; every one is checked by lz4_next_sequence BEFORE a byte of the sequence moves): a length
// chain or literals past the block, an offset of 0 or beyond the bytes produced so far, literals or a match past the page's
// uncompressed size, a block that ends before that size is reached, input left over after it.  A failure is PQ_ERR_INFLATE.
//
// The stage is codec-independent but for the sequence parser: a page is {an uncompressed prefix, a compressed or stored rest};
// another codec adds a parser that yields the same (literals, offset, match length) and a value of PqInflatePage::codec.
#pragma once
#include <stdint.h>

#include "dfx_parquet_rle.hpp"

namespace dfx {

enum : uint32_t {
  PQ_INFLATE_COMPRESSED = 1u,        // the rest after the prefix is a compressed block (clear: stored, a plain copy)
  PQ_INFLATE_PROBE_AFTER_LEVELS = 2u // V1 page of an optional column: the probe offset is 4 + the LE32 at body offset 0
};

// One page of a compressed chunk as the inflate kernel sees it.  The host's header pass (dfx_parquet_meta.hpp: walk_headers) has
// checked [src_off, src_off + src_len) against the chunk, [dst_off, dst_off + dst_len) against the inflated image, prefix_len
// against both, and for a stored page that the two rests are equally long.
struct PqInflatePage {
  uint32_t src_off;     // the page's body in the chunk (prefix first)
  uint32_t src_len;     // PageHeader::compressed_size
  uint32_t dst_off;     // the page's body in the inflated image, 8-byte aligned
  uint32_t dst_len;     // PageHeader::uncompressed_size
  uint32_t prefix_len;  // V2: the repetition and definition levels, never compressed; 0 otherwise
  uint32_t flags;       // PQ_INFLATE_*
  uint32_t probe_off;   // body offset of the second word of the page's prologue (ignored with PQ_INFLATE_PROBE_AFTER_LEVELS)
  uint32_t codec;       // the Parquet codec id of the compressed rest (7)
};

// What the body pass needs of an inflated page of fixed-width or Boolean values, stored by the kernel after it inflated the page:
// the LE32 at body offset 0 (a V1 optional page: the length of its definition levels) and the LE32 at the probe offset (the index
// width byte of a dictionary-encoded page, the length of a Boolean page's RLE values).  Bytes past the page's end read as 0.
struct PqPrologue {
  uint32_t word0, probe;
};
DFX_PQ_HD uint32_t pq_le32_or_zero(const uint8_t* body, uint64_t len, uint64_t off) {
  uint32_t v = 0;
  for (uint32_t k = 0; k < 4; ++k)
    if (off + k < len) v |= (uint32_t)body[off + k] << (8 * k);
  return v;
}
DFX_PQ_HD uint64_t pq_probe_offset(const PqInflatePage& pg, uint32_t word0) {
  return (pg.flags & PQ_INFLATE_PROBE_AFTER_LEVELS) ? 4ull + word0 : (uint64_t)pg.probe_off;
}

struct Lz4Seq {
  uint64_t lit_pos;    // the literals in the block
  uint32_t lit_len;
  uint32_t offset;     // the match: 1 .. 65535, <= the bytes produced once the literals are out (0 in the last sequence)
  uint32_t match_len;  // >= 4 (0 in the last sequence)
  uint32_t last;       // 1: literals only, the block ends behind them and the output is complete
  uint32_t lit_ext, match_ext;  // extension bytes of the two lengths
  uint64_t next;       // the next sequence's token
};

// parses the sequence whose token is at `pos` of block [src, src + src_len), `out_pos` of `out_len` bytes having been produced.
// false: malformed (the rules above).  Reads [pos, next) of the block only, and nothing once it returns false.
DFX_PQ_HD bool lz4_next_sequence(const uint8_t* src, uint64_t src_len, uint64_t pos, uint64_t out_pos, uint64_t out_len, Lz4Seq* q) {
  if (pos >= src_len || out_pos > out_len) return false;
  const uint32_t token = src[pos++];
  uint64_t lit = token >> 4;
  q->lit_ext = 0;
  q->match_ext = 0;
  if (lit == 15) {
    for (;;) {
      if (pos >= src_len) return false;
      const uint32_t b = src[pos++];
      lit += b;
      ++q->lit_ext;
      if (b != 255) break;
    }
  }
  if (lit > src_len - pos || lit > out_len - out_pos) return false;
  q->lit_pos = pos;
  q->lit_len = (uint32_t)lit;
  pos += lit;
  out_pos += lit;
  if (pos == src_len) {  // the last sequence: literals only
    if (out_pos != out_len) return false;
    q->offset = 0;
    q->match_len = 0;
    q->last = 1;
    q->next = pos;
    return true;
  }
  if (src_len - pos < 2) return false;
  const uint32_t offset = (uint32_t)src[pos] | (uint32_t)src[pos + 1] << 8;
  pos += 2;
  if (offset == 0 || offset > out_pos) return false;
  uint64_t len = (token & 15u) + 4;
  if ((token & 15u) == 15) {
    for (;;) {
      if (pos >= src_len) return false;
      const uint32_t b = src[pos++];
      len += b;
      ++q->match_ext;
      if (b != 255) break;
    }
  }
  if (len > out_len - out_pos) return false;
  q->offset = offset;
  q->match_len = (uint32_t)len;
  q->last = 0;
  q->next = pos;  // (a block that ends here has no last sequence: the next call finds pos == src_len and fails)
  return true;
}

struct Lz4Stats {
  uint64_t sequences = 0, lit_extensions = 0, match_extensions = 0;
  uint64_t offset_1 = 0, offset_lt8 = 0, offset_ge64 = 0, offset_ge32768 = 0;  // matches by offset
  uint64_t overlapping = 0;   // matches with offset < length
  uint64_t stored_pages = 0;  // pages copied, not inflated (counted by the caller that copies them)
};

// the sequential decoder: block [src, src + src_len) -> exactly out_len bytes at dst.  false: malformed; dst holds what the
// sequences before the bad one produced.  An empty block is the block of an empty page.
inline bool lz4_decode_block(const uint8_t* src, uint64_t src_len, uint8_t* dst, uint64_t out_len, Lz4Stats* stats = nullptr) {
  if (src_len == 0 && out_len == 0) return true;
  uint64_t pos = 0, out = 0;
  for (;;) {
    Lz4Seq q;
    if (!lz4_next_sequence(src, src_len, pos, out, out_len, &q)) return false;
    for (uint32_t i = 0; i < q.lit_len; ++i) dst[out + i] = src[q.lit_pos + i];
    out += q.lit_len;
    if (stats) {
      ++stats->sequences;
      stats->lit_extensions += q.lit_ext;
      stats->match_extensions += q.match_ext;
    }
    if (q.last) return true;
    for (uint32_t i = 0; i < q.match_len; ++i) dst[out + i] = dst[out + i - q.offset];
    out += q.match_len;
    pos = q.next;
    if (stats) {
      stats->offset_1 += q.offset == 1;
      stats->offset_lt8 += q.offset < 8;
      stats->offset_ge64 += q.offset >= 64;
      stats->offset_ge32768 += q.offset >= 32768;
      stats->overlapping += q.offset < q.match_len;
    }
  }
}

}  // namespace dfx
