// dfx_parquet_rle.hpp -- the RLE / bit-packed hybrid of Parquet levels, dictionary indices and RLE Booleans, and the page table
// the host hands the device: ONE source for the kernels (dfx_k_parquet.hip), the sequential host decoder (dfx_parquet_meta.hpp,
// what tests/native/parquet_check.cpp holds against pyarrow) and the relation (dfx_parquet.cpp).  Free of HIP.
//
//   hybrid  := run*                      run := header-varint payload
//   header & 1 == 1: bit-packed, groups = header >> 1, values = 8 * groups, payload = groups * width bytes, value i of the run
//                    is bits [i * width, (i + 1) * width) of the payload, LSB first
//   header & 1 == 0: RLE, count = header >> 1, payload = ceil(width / 8) bytes, one little-endian value repeated count times
//   width 0: every value is 0 and no payload byte is read.  0 <= width <= 32.
//
// Bounds rules (the same on both sides): a header varint of more than 5 bytes or past the end, a payload past the end, a width
// above 32 are PQ_ERR_RUN; a walk stops after `want` values, whatever the last run still holds (the writer pads the last group).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DFX_PQ_HD __host__ __device__ inline
#else
#define DFX_PQ_HD inline
#endif

namespace dfx {

// error bits of the device control block's CTRL_ERROR word (error_from_ctrl: DFX_PARSER_ERROR) and of the host decoder
enum : uint32_t {
  PQ_ERR_RUN = 1u << 16,         // a run of a hybrid stream overruns its page (or its header is malformed)
  PQ_ERR_DICT_INDEX = 1u << 17,  // a dictionary index >= the dictionary's size
  PQ_ERR_VALUE = 1u << 18,       // a page holds fewer values than its levels say are non-null
  PQ_ERR_INFLATE = 1u << 19,     // a compressed page's block is malformed (dfx_parquet_lz4.hpp: the bounds rules)
  PQ_ERR_ALL = PQ_ERR_RUN | PQ_ERR_DICT_INDEX | PQ_ERR_VALUE | PQ_ERR_INFLATE
};

enum : uint32_t { PQ_ENC_PLAIN = 0, PQ_ENC_DICT = 1, PQ_ENC_RLE_BOOL = 2 };

// One data page as the kernels see it.  Every offset is relative to the chunk's first byte on the device and has been checked
// by the host against the chunk's extent (dfx_parquet_meta.hpp: walk_chunk): [lev_off, lev_off + lev_len) and [val_off, val_off + val_len) lie inside.
struct PqPage {
  uint32_t enc;         // PQ_ENC_*
  uint32_t bit_width;   // PQ_ENC_DICT: width of the indices
  uint32_t lev_off;     // definition levels: hybrid at width 1 (lev_len == 0 and required: none)
  uint32_t lev_len;
  uint32_t val_off;     // PLAIN: the values; DICT / RLE_BOOL: the hybrid stream (after the width byte / the length prefix)
  uint32_t val_len;
  uint32_t num_values;  // rows of the page (nulls included)
  uint32_t first_row;   // of the page within the row group
  uint32_t dense_base;  // the page's first slot in the dense buffers (decoded indices, expanded Boolean bits): rows before it
  uint32_t rank_base;   // the page's first entry in the word-rank buffer
  uint32_t str_base;    // PLAIN Utf8: the page's first entry in the string-offset buffer (`pad` + 1 entries per page)
  uint32_t pad;         // PLAIN Utf8: the strings the page holds (its entries from str_base on, plus an end); 0 otherwise
};

struct PqRun {
  uint32_t packed;   // 1: bit-packed
  uint32_t count;    // values of the run (8 * groups, or the repeat count)
  uint32_t value;    // RLE: the value
  uint64_t payload;  // bit-packed: offset of the payload in the stream
  uint64_t next;     // offset of the next header
};

// reads the run whose header starts at `pos` of stream [p, p + len); false: malformed (PQ_ERR_RUN)
DFX_PQ_HD bool pq_read_run(const uint8_t* p, uint64_t len, uint64_t pos, uint32_t width, PqRun* r) {
  if (width > 32) return false;
  uint64_t h = 0;
  int shift = 0;
  for (;;) {
    if (pos >= len || shift > 28) return false;
    const uint8_t b = p[pos++];
    h |= (uint64_t)(b & 0x7F) << shift;
    shift += 7;
    if (!(b & 0x80)) break;
  }
  if (h >> 32) return false;
  if (h & 1) {
    const uint64_t groups = h >> 1;
    const uint64_t bytes = groups * width;
    if (groups > (1ull << 28) || bytes > len - pos) return false;
    r->packed = 1;
    r->count = (uint32_t)(groups * 8);
    r->value = 0;
    r->payload = pos;
    r->next = pos + bytes;
    return true;
  }
  const uint32_t vb = (width + 7) / 8;
  if (vb > len - pos) return false;
  uint32_t v = 0;
  for (uint32_t i = 0; i < vb; ++i) v |= (uint32_t)p[pos + i] << (8 * i);
  r->packed = 0;
  r->count = (uint32_t)(h >> 1);
  r->value = width < 32 ? (v & ((1u << width) - 1u)) : v;
  r->payload = pos;
  r->next = pos + vb;
  return true;
}

// value i of a bit-packed payload at `width` (1 .. 32): byte loads only, at most 5 bytes, all inside the payload the run's
// geometry was checked for (i < 8 * groups)
DFX_PQ_HD uint32_t pq_unpack(const uint8_t* payload, uint64_t i, uint32_t width) {
  if (width == 0) return 0;
  const uint64_t bit = i * width;
  const uint64_t byte = bit >> 3;
  const uint32_t sh = (uint32_t)(bit & 7);
  const uint32_t nbytes = (sh + width + 7) / 8;
  uint64_t v = 0;
  for (uint32_t k = 0; k < nbytes; ++k) v |= (uint64_t)payload[byte + k] << (8 * k);
  v >>= sh;
  return width < 32 ? (uint32_t)(v & ((1ull << width) - 1ull)) : (uint32_t)v;
}

// sequential decode of up to `want` values (the host side; out may be null: count only).  Returns the values decoded, sets *err.
// A stream that ends early just gives fewer values: the caller knows how many it needs.
inline uint64_t pq_decode_hybrid(const uint8_t* p, uint64_t len, uint32_t width, uint64_t want, uint32_t* out, uint32_t* err,
                                 uint64_t* rle_runs = nullptr, uint64_t* packed_runs = nullptr) {
  uint64_t pos = 0, got = 0;
  while (got < want && pos < len) {
    PqRun r;
    if (!pq_read_run(p, len, pos, width, &r)) {
      *err |= PQ_ERR_RUN;
      return got;
    }
    const uint64_t n = (uint64_t)r.count < want - got ? (uint64_t)r.count : want - got;
    if (out) {
      if (r.packed)
        for (uint64_t i = 0; i < n; ++i) out[got + i] = pq_unpack(p + r.payload, i, width);
      else
        for (uint64_t i = 0; i < n; ++i) out[got + i] = r.value;
    }
    if (r.packed && packed_runs) ++*packed_runs;
    if (!r.packed && rle_runs) ++*rle_runs;
    got += n;
    pos = r.next;
  }
  return got;
}

}  // namespace dfx
