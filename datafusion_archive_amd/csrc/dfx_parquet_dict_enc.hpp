// dfx_parquet_dict_enc.hpp -- the rules of the Parquet writer's "dictionary" option (deviation D13): what its
// kernels (dfx_k_parquet_write_dict.hip), its host code (dfx_parquet_write.cpp) and its CPU test
// (tests/native/parquet_dict_write_check.cpp) share on top of dfx_parquet_enc.hpp.  Free of HIP.
//
//   dictionary  one per column chunk (row group and column), keyed on the STORED bit pattern: a fixed-width value after pqw::widen in
//               stored_width bytes (NaN payloads are entries of their own, -0.0 and +0.0 are two), a Utf8 value's bytes.  Null slots
//               contribute nothing.  Ids in order of first occurrence in the chunk's row order.  Boolean columns have none.
//   its page    the chunk's first page: the entries in id order, PLAIN (stored width each; LE32 length + bytes for Utf8)
//   data page   V1, RLE_DICTIONARY: the level block as in a PLAIN page, one byte w, then ONE run over the page's nn non-null values:
//               nothing when nn == 0; an RLE run when all its indices are equal: varint(nn << 1), the index in ceil(w / 8) bytes;
//               else one bit-packed run: varint(ceil(nn / 8) << 1 | 1) and ceil(nn / 8) * w bytes, LSB first, padding bits zero
//   w           max(1, bits(max(E, 1) - 1)), E the chunk's entries after the launch that holds the page
//   decision    per LAUNCH (the rows ParquetSink::encode_rows takes at once): a chunk in dictionary mode that would gain e_new
//               entries of b_new body bytes stays in it iff E + e_new <= N and the body still obeys the i32 rule; else it is PLAIN from
//               this launch to its end, E and the body as they were.  A chunk that falls back in its first launch has no dictionary
//               page: it is byte for byte the chunk written without the option.
//
// DictChunk / dict_encode_launch are the sequential restatement the kernels are held against (whole files, byte for byte).  They know
// no hash: a chunk the device gives up for a hash collision of two Utf8 values is the one place where the two may differ.
#pragma once
#include <unordered_map>

#include "dfx_parquet_enc.hpp"

namespace dfx {
namespace pqw {

constexpr int64_t kMaxDictionary = 1 << 20;
enum : uint32_t { DICT_RUN_NONE = 0, DICT_RUN_RLE = 1, DICT_RUN_PACKED = 2 };

// ---- options -----------------------------------------------------------------------------------------------------------------------
DFX_PQ_HD bool dictionary_ok(int64_t n) { return n >= 0 && n <= kMaxDictionary; }  // 0: no dictionaries
DFX_PQ_HD bool dictionary_hash_bits_ok(int64_t bits) { return bits >= 1 && bits <= 64; }
DFX_PQ_HD bool dictionary_dtype(int dtype) { return dtype_ok(dtype) && dtype != DFX_BOOLEAN; }

// ---- sizes -------------------------------------------------------------------------------------------------------------------------
DFX_PQ_HD uint32_t bits_of(uint64_t v) {
  uint32_t n = 0;
  while (v) {
    v >>= 1;
    ++n;
  }
  return n;
}
DFX_PQ_HD uint32_t dict_index_width(uint64_t entries) {
  const uint32_t b = bits_of((entries ? entries : 1) - 1);
  return b ? b : 1;
}
DFX_PQ_HD uint32_t dict_run_kind(uint64_t nn, bool all_equal) { return nn == 0 ? DICT_RUN_NONE : all_equal ? DICT_RUN_RLE : DICT_RUN_PACKED; }
DFX_PQ_HD uint64_t dict_run_header(uint32_t run, uint64_t nn) { return run == DICT_RUN_PACKED ? ((nn + 7) / 8) << 1 | 1 : nn << 1; }
// bytes of the run: header + the index (RLE) or the groups (bit-packed)
DFX_PQ_HD uint64_t dict_run_bytes(uint32_t run, uint32_t w, uint64_t nn) {
  if (run == DICT_RUN_NONE) return 0;
  return varint_len(dict_run_header(run, nn)) + (run == DICT_RUN_RLE ? (uint64_t)((w + 7) / 8) : (nn + 7) / 8 * w);
}
// bytes of a dictionary data page's value block: the width byte and the run
DFX_PQ_HD uint64_t dict_value_bytes(uint32_t run, uint32_t w, uint64_t nn) { return 1 + dict_run_bytes(run, w, nn); }
// bytes of one entry in the dictionary page's body
DFX_PQ_HD uint64_t dict_entry_bytes(int dtype, uint64_t utf8_len) { return dtype == DFX_UTF8 ? 4 + utf8_len : stored_width(dtype); }
// the decision of a launch: E entries of B body bytes so far, e_new / b_new what the launch would add, N the option
DFX_PQ_HD bool dict_stays(uint64_t entries, uint64_t e_new, uint64_t body_bytes, uint64_t b_new, uint64_t limit) {
  const uint64_t b = body_bytes + b_new;
  return entries + e_new <= limit && b >= body_bytes && body_fits(0, b);
}
// slots of a chunk's device table: twice the next power of two of the entries it can come to hold (at most N, at most the row group's rows)
DFX_PQ_HD uint64_t dict_table_slots(uint64_t limit, uint64_t row_group_rows) {
  const uint64_t most = limit < row_group_rows ? limit : row_group_rows;
  uint64_t p = 1;
  while (p < most) p <<= 1;
  return 2 * p;
}

// ---- the sequential encoder of a dictionary chunk ----------------------------------------------------------------------------------
struct DictChunk {  // one column chunk under the option; a new row group starts with a new one
  bool plain = false;     // fell back: PLAIN pages from that launch on
  int64_t launches = 0;   // launches held in dictionary mode: > 0, the chunk has a dictionary page
  uint64_t entries = 0;
  std::vector<uint8_t> body;  // the dictionary page's body
  std::unordered_map<std::string, uint32_t> ids;  // stored bytes -> id
};
struct DictPage {
  EncodedPage info;  // val_bytes: the width byte and the run
  uint32_t run = DICT_RUN_NONE, width = 1;
  std::vector<uint8_t> body;  // exactly the page's body
};
inline std::string dict_key(const SourceColumn& c, int64_t r) {
  if (c.dtype == DFX_UTF8) return std::string((const char*)c.data + c.offsets[r], (size_t)(c.offsets[r + 1] - c.offsets[r]));
  const uint32_t sw = stored_width(c.dtype), rw = source_width(c.dtype);
  uint64_t raw = 0;
  memcpy(&raw, (const uint8_t*)c.values + (size_t)r * rw, rw);
  const uint64_t w = widen(c.dtype, raw);
  return std::string((const char*)&w, sw);
}
// one page of dictionary indices: rows [row0, row0 + n) of the column, `idx` the ids of its non-null rows in row order.
// false: the i32 rule refuses the page.
inline bool dict_encode_page(const SourceColumn& c, int64_t row0, int64_t n, const std::vector<uint32_t>& idx, uint32_t w, DictPage* pg) {
  const uint64_t nn = idx.size();
  bool all_equal = true;
  for (uint32_t v : idx) all_equal = all_equal && v == idx[0];
  pg->run = dict_run_kind(nn, all_equal);
  pg->width = w;
  pg->info.num_values = n;
  pg->info.non_null = (int64_t)nn;
  pg->info.kind = level_kind(c.optional, (uint64_t)n, nn);
  pg->info.level_bytes = level_block_bytes(pg->info.kind, (uint64_t)n);
  pg->info.val_bytes = dict_value_bytes(pg->run, w, nn);
  if (!body_fits(pg->info.level_bytes, pg->info.val_bytes)) return false;
  pg->body.assign((size_t)(pg->info.level_bytes + pg->info.val_bytes), 0);
  uint8_t* p = pg->body.data();
  if (pg->info.kind != LEVELS_NONE) {
    uint64_t lo = 0, hi = 0;
    const uint32_t len = level_block_prefix(pg->info.kind, (uint64_t)n, &lo, &hi);
    for (uint32_t k = 0; k < len; ++k) p[k] = (uint8_t)((k < 8 ? lo >> (8 * k) : hi >> (8 * (k - 8))) & 0xFF);
    if (pg->info.kind == LEVELS_MIXED)
      for (int64_t i = 0; i < n; ++i)
        if (source_valid(c, row0 + i)) p[len + (i >> 3)] |= (uint8_t)(1u << (i & 7));
  }
  uint8_t* v = p + pg->info.level_bytes;
  *v++ = (uint8_t)w;
  if (pg->run == DICT_RUN_NONE) return true;
  for (uint64_t h = dict_run_header(pg->run, nn);; h >>= 7) {
    *v++ = (uint8_t)(h >= 0x80 ? (h & 0x7F) | 0x80 : h);
    if (h < 0x80) break;
  }
  if (pg->run == DICT_RUN_RLE) {
    for (uint32_t k = 0; k < (w + 7) / 8; ++k) v[k] = (uint8_t)(idx[0] >> (8 * k));
  } else {
    for (uint64_t i = 0; i < nn; ++i)
      for (uint32_t b = 0; b < w; ++b)
        if (idx[i] >> b & 1) v[(i * w + b) >> 3] |= (uint8_t)(1u << ((i * w + b) & 7));
  }
  return true;
}
// One launch -- rows [row0, row0 + n) of the column, pages of page_rows rows -- of a chunk in dictionary mode under limit N.
// 1: the launch stayed in dictionary mode, *pages holds its pages; 0: the chunk fell back (k->plain; the caller encodes the launch's
// and every later page with encode_page); -1: the i32 rule refuses a page.
inline int dict_encode_launch(const SourceColumn& c, int64_t row0, int64_t n, int64_t page_rows, uint64_t limit, DictChunk* k, std::vector<DictPage>* pages) {
  std::unordered_map<std::string, uint32_t> fresh;
  std::vector<const std::string*> order;
  uint64_t b_new = 0;
  for (int64_t r = row0; r < row0 + n; ++r) {
    if (!source_valid(c, r)) continue;
    const std::string key = dict_key(c, r);
    if (k->ids.count(key)) continue;
    auto ins = fresh.emplace(key, (uint32_t)fresh.size());
    if (!ins.second) continue;
    order.push_back(&ins.first->first);
    b_new += dict_entry_bytes(c.dtype, key.size());
  }
  if (!dict_stays(k->entries, fresh.size(), k->body.size(), b_new, limit)) {
    k->plain = true;
    return 0;
  }
  for (const std::string* key : order) {
    if (c.dtype == DFX_UTF8)
      for (int b = 0; b < 4; ++b) k->body.push_back((uint8_t)((uint32_t)key->size() >> (8 * b)));
    k->body.insert(k->body.end(), key->begin(), key->end());
    k->ids.emplace(*key, (uint32_t)k->entries++);
  }
  ++k->launches;
  const uint32_t w = dict_index_width(k->entries);
  for (int64_t p0 = 0; p0 < n; p0 += page_rows) {
    const int64_t pn = page_rows < n - p0 ? page_rows : n - p0;
    std::vector<uint32_t> idx;
    for (int64_t r = row0 + p0; r < row0 + p0 + pn; ++r)
      if (source_valid(c, r)) idx.push_back(k->ids.find(dict_key(c, r))->second);
    pages->emplace_back();
    if (!dict_encode_page(c, row0 + p0, pn, idx, w, &pages->back())) return -1;
  }
  return 1;
}

}  // namespace pqw
}  // namespace dfx
