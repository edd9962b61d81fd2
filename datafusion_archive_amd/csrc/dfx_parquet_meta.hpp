// dfx_parquet_meta.hpp -- the host side of the Parquet source (deviation D12), free of HIP: a bounds-checked reader of thrift's
// compact protocol, FileMetaData / PageHeader, the supported subset, the walk over a column chunk's pages that fills the page
// table (dfx_parquet_rle.hpp: PqPage) and the length chains of PLAIN byte arrays, and a sequential decoder of a whole chunk.  For a
// compressed chunk (codec 7, LZ4_RAW) the walk is split: a header pass over the file's bytes (walk_headers: the inflate table and
// the layout of the inflated image), the inflate stage (dfx_parquet_lz4.hpp; on the device k_pq_inflate), a body pass over the image
// or over the pages' prologues (walk_bodies).  dfx_parquet.cpp uses everything but the decoders; tests/native/parquet_check.cpp and
// tests/native/parquet_lz4_check.cpp hold all of it against pyarrow on the CPU.
//
// Nothing here trusts a count from the file: lists are read element by element after their size has been checked against the
// bytes that remain (an element takes at least one), extents are checked before they are used, and every failure is a
// Err{DFX_PARSER_ERROR | DFX_NOT_IMPLEMENTED, what and where} (one exception: a Utf8 column beyond Arrow's 32-bit offsets is the
// DFX_EXECUTION_ERROR the CSV source gives, utf8_total_error).
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/dfx.h"
#include "dfx_parquet_lz4.hpp"
#include "dfx_parquet_rle.hpp"
#include "dfx_scan_rules.hpp"

namespace dfx {
namespace pq {

struct Err {
  int32_t code = DFX_OK;
  std::string msg;
  bool ok() const { return code == DFX_OK; }
};
inline Err parser_error(const std::string& m) { return Err{DFX_PARSER_ERROR, "Parquet: " + m}; }
inline Err not_implemented(const std::string& m) { return Err{DFX_NOT_IMPLEMENTED, "Parquet: " + m}; }
inline std::string num(long long v) {
  char b[32];
  snprintf(b, sizeof(b), "%lld", v);
  return b;
}

// ---- thrift compact protocol ------------------------------------------------------------------------------------------------
enum : int { T_STOP = 0, T_TRUE = 1, T_FALSE = 2, T_BYTE = 3, T_I16 = 4, T_I32 = 5, T_I64 = 6, T_DOUBLE = 7, T_BINARY = 8, T_LIST = 9,
             T_SET = 10, T_MAP = 11, T_STRUCT = 12 };

class Thrift {
 public:
  Thrift(const uint8_t* p, size_t n) : p_(p), n_(n) {}
  bool bad() const { return bad_; }
  size_t pos() const { return pos_; }
  size_t left() const { return n_ - pos_; }
  uint64_t varint() {
    uint64_t v = 0;
    for (int shift = 0; shift < 70; shift += 7) {
      if (pos_ >= n_) return fail();
      const uint8_t b = p_[pos_++];
      if (shift < 64) v |= (uint64_t)(b & 0x7F) << shift;
      if (!(b & 0x80)) return v;
    }
    return fail();
  }
  int64_t zigzag() {
    const uint64_t v = varint();
    return (int64_t)(v >> 1) ^ -(int64_t)(v & 1);
  }
  int32_t i32() {
    const int64_t v = zigzag();
    if (v < INT32_MIN || v > INT32_MAX) fail();
    return (int32_t)v;
  }
  // next field of the struct being read; *last carries the previous field id.  false: STOP (or damage: bad())
  bool field(int* last, int* id, int* type) {
    if (bad_ || pos_ >= n_) return fail() != 0;
    const uint8_t b = p_[pos_++];
    if (b == 0) return false;
    *type = b & 0x0F;
    const int delta = b >> 4;
    if (delta)
      *id = *last + delta;
    else
      *id = (int)zigzag();
    *last = *id;
    if (*id <= 0) return fail() != 0;  // field ids are positive
    return !bad_;
  }
  bool list(int* etype, uint32_t* size) {
    if (pos_ >= n_) return fail() != 0;
    const uint8_t b = p_[pos_++];
    *etype = b & 0x0F;
    uint64_t s = b >> 4;
    if (s == 15) s = varint();
    if (bad_ || s > left()) return fail() != 0;  // every element takes at least one byte
    *size = (uint32_t)s;
    return true;
  }
  bool binary(std::string* out) {
    const uint64_t len = varint();
    if (bad_ || len > left()) return fail() != 0;
    if (out) out->assign((const char*)p_ + pos_, (size_t)len);
    pos_ += (size_t)len;
    return true;
  }
  bool boolean(int type) const { return type == T_TRUE; }
  void skip(int type, bool in_list = false, int depth = 0) {
    if (bad_) return;
    if (depth > 24) {
      fail();
      return;
    }
    switch (type) {
      case T_TRUE:
      case T_FALSE:
        if (in_list) advance(1);
        break;
      case T_BYTE: advance(1); break;
      case T_I16:
      case T_I32:
      case T_I64: (void)varint(); break;
      case T_DOUBLE: advance(8); break;
      case T_BINARY: (void)binary(nullptr); break;
      case T_LIST:
      case T_SET: {
        int et = 0;
        uint32_t n = 0;
        if (!list(&et, &n)) return;
        for (uint32_t i = 0; i < n && !bad_; ++i) skip(et, true, depth + 1);
        break;
      }
      case T_MAP: {
        const uint64_t n = varint();
        if (bad_ || n > left()) {
          fail();
          return;
        }
        if (n == 0) break;
        if (pos_ >= n_) {
          fail();
          return;
        }
        const uint8_t kv = p_[pos_++];
        for (uint64_t i = 0; i < n && !bad_; ++i) {
          skip(kv >> 4, true, depth + 1);
          skip(kv & 0x0F, true, depth + 1);
        }
        break;
      }
      case T_STRUCT: {
        int last = 0, id = 0, ty = 0;
        while (field(&last, &id, &ty)) skip(ty, false, depth + 1);
        break;
      }
      default: fail();
    }
  }
  uint8_t byte() {
    if (pos_ >= n_) return (uint8_t)fail();
    return p_[pos_++];
  }

 private:
  uint64_t fail() {
    bad_ = true;
    pos_ = n_;
    return 0;
  }
  void advance(size_t k) {
    if (k > left())
      fail();
    else
      pos_ += k;
  }
  const uint8_t* p_;
  size_t n_, pos_ = 0;
  bool bad_ = false;
};

// ---- FileMetaData -----------------------------------------------------------------------------------------------------------
enum : int { PT_BOOLEAN = 0, PT_INT32 = 1, PT_INT64 = 2, PT_INT96 = 3, PT_FLOAT = 4, PT_DOUBLE = 5, PT_BYTE_ARRAY = 6, PT_FIXED = 7 };
inline const char* physical_name(int t) {
  static const char* n[] = {"BOOLEAN", "INT32", "INT64", "INT96", "FLOAT", "DOUBLE", "BYTE_ARRAY", "FIXED_LEN_BYTE_ARRAY"};
  return t >= 0 && t < 8 ? n[t] : "?";
}
inline const char* codec_name(int c) {
  static const char* n[] = {"UNCOMPRESSED", "SNAPPY", "GZIP", "LZO", "BROTLI", "LZ4", "ZSTD", "LZ4_RAW"};
  return c >= 0 && c < 8 ? n[c] : "?";
}
inline const char* encoding_name(int e) {
  static const char* n[] = {"PLAIN", "?", "PLAIN_DICTIONARY", "RLE", "BIT_PACKED", "DELTA_BINARY_PACKED", "DELTA_LENGTH_BYTE_ARRAY",
                            "DELTA_BYTE_ARRAY", "RLE_DICTIONARY", "BYTE_STREAM_SPLIT"};
  return e >= 0 && e < 10 ? n[e] : "?";
}
inline const char* logical_name(int l) {
  static const char* n[] = {"?", "STRING", "MAP", "LIST", "ENUM", "DECIMAL", "DATE", "TIME", "TIMESTAMP", "?", "INTEGER", "UNKNOWN",
                            "JSON", "BSON", "UUID", "FLOAT16"};
  return l >= 0 && l < 16 ? n[l] : "?";
}
inline const char* converted_name(int c) {
  static const char* n[] = {"UTF8", "MAP", "MAP_KEY_VALUE", "LIST", "ENUM", "DECIMAL", "DATE", "TIME_MILLIS", "TIME_MICROS",
                            "TIMESTAMP_MILLIS", "TIMESTAMP_MICROS", "UINT_8", "UINT_16", "UINT_32", "UINT_64", "INT_8", "INT_16",
                            "INT_32", "INT_64", "JSON", "BSON", "INTERVAL"};
  return c >= 0 && c < 22 ? n[c] : "?";
}

struct SchemaElement {
  int32_t type = -1;        // physical type; -1: a group
  int32_t repetition = -1;  // 0 required, 1 optional, 2 repeated
  std::string name;
  int32_t num_children = 0;
  int32_t converted = -1;
  int32_t logical = -1;  // field id of the LogicalType union
  int32_t int_width = 0;
  bool int_signed = true;
};
struct ChunkMeta {
  bool has_meta = false;
  int32_t type = -1;
  std::vector<int32_t> encodings;
  std::vector<std::string> path;  // path_in_schema
  int32_t codec = 0;
  int64_t num_values = 0, total_uncompressed_size = 0, total_compressed_size = 0;
  int64_t data_page_offset = 0, dictionary_page_offset = 0;
  bool has_dictionary_offset = false;
  // where the chunk's bytes are: the dictionary page comes first when there is one
  int64_t start() const {
    // (a chunk without rows has a dictionary page and no data page: data_page_offset is 0)
    return has_dictionary_offset && dictionary_page_offset > 0 && (data_page_offset <= 0 || dictionary_page_offset < data_page_offset)
               ? dictionary_page_offset
               : data_page_offset;
  }
};
struct RowGroupMeta {
  std::vector<ChunkMeta> columns;
  int64_t num_rows = 0;
  bool complete = false;  // both required fields were there
};
struct FileMeta {
  int32_t version = 0;
  std::vector<SchemaElement> schema;
  int64_t num_rows = 0;
  std::vector<RowGroupMeta> row_groups;
};
struct Column {  // one leaf of a flat schema, as the stream serves it
  std::string name;
  int dtype = DFX_TYPE_NONE;
  bool optional = false;
  int physical = -1;
};

inline void read_logical(Thrift& t, SchemaElement* e) {
  int last = 0, id = 0, ty = 0;
  while (t.field(&last, &id, &ty)) {
    e->logical = id;
    if (id == 10 && ty == T_STRUCT) {  // IntType { 1: i8 bitWidth, 2: bool isSigned }
      int l2 = 0, id2 = 0, ty2 = 0;
      while (t.field(&l2, &id2, &ty2)) {
        if (id2 == 1 && ty2 == T_BYTE)
          e->int_width = (int8_t)t.byte();
        else if (id2 == 2 && (ty2 == T_TRUE || ty2 == T_FALSE))
          e->int_signed = t.boolean(ty2);
        else
          t.skip(ty2);
      }
    } else {
      t.skip(ty);
    }
  }
}
inline void read_schema_element(Thrift& t, SchemaElement* e) {
  int last = 0, id = 0, ty = 0;
  while (t.field(&last, &id, &ty)) {
    if (id == 1 && ty == T_I32) e->type = t.i32();
    else if (id == 3 && ty == T_I32) e->repetition = t.i32();
    else if (id == 4 && ty == T_BINARY) t.binary(&e->name);
    else if (id == 5 && ty == T_I32) e->num_children = t.i32();
    else if (id == 6 && ty == T_I32) e->converted = t.i32();
    else if (id == 10 && ty == T_STRUCT) read_logical(t, e);
    else t.skip(ty);
  }
}
inline void read_column_meta(Thrift& t, ChunkMeta* c) {
  int last = 0, id = 0, ty = 0;
  uint32_t seen = 0;  // required: type, codec, num_values, total_compressed_size, data_page_offset
  while (t.field(&last, &id, &ty)) {
    if (((id == 1 || id == 4) && ty == T_I32) || ((id == 5 || id == 7 || id == 9) && ty == T_I64)) seen |= 1u << id;
    c->has_meta = seen == ((1u << 1) | (1u << 4) | (1u << 5) | (1u << 7) | (1u << 9));
    if (id == 1 && ty == T_I32) c->type = t.i32();
    else if (id == 2 && ty == T_LIST) {
      int et = 0;
      uint32_t n = 0;
      if (!t.list(&et, &n)) return;
      for (uint32_t i = 0; i < n && !t.bad(); ++i) {
        if (et == T_I32) c->encodings.push_back(t.i32());
        else t.skip(et, true);
      }
    } else if (id == 3 && ty == T_LIST) {
      int et = 0;
      uint32_t n = 0;
      if (!t.list(&et, &n)) return;
      for (uint32_t i = 0; i < n && !t.bad(); ++i) {
        if (et == T_BINARY) {
          c->path.emplace_back();
          t.binary(&c->path.back());
        } else t.skip(et, true);
      }
    } else if (id == 4 && ty == T_I32) c->codec = t.i32();
    else if (id == 5 && ty == T_I64) c->num_values = t.zigzag();
    else if (id == 6 && ty == T_I64) c->total_uncompressed_size = t.zigzag();
    else if (id == 7 && ty == T_I64) c->total_compressed_size = t.zigzag();
    else if (id == 9 && ty == T_I64) c->data_page_offset = t.zigzag();
    else if (id == 11 && ty == T_I64) {
      c->dictionary_page_offset = t.zigzag();
      c->has_dictionary_offset = true;
    } else t.skip(ty);  // path_in_schema, key-value metadata, statistics, index offsets ...: never interpreted
  }
}
inline void read_row_group(Thrift& t, RowGroupMeta* g) {
  int last = 0, id = 0, ty = 0;
  uint32_t seen = 0;
  while (t.field(&last, &id, &ty)) {
    if ((id == 1 && ty == T_LIST) || (id == 3 && ty == T_I64)) seen |= 1u << id;
    g->complete = seen == 0xAu;
    if (id == 1 && ty == T_LIST) {
      int et = 0;
      uint32_t n = 0;
      if (!t.list(&et, &n)) return;
      for (uint32_t i = 0; i < n && !t.bad(); ++i) {
        if (et != T_STRUCT) {
          t.skip(et, true);
          continue;
        }
        g->columns.emplace_back();
        int l2 = 0, id2 = 0, ty2 = 0;
        while (t.field(&l2, &id2, &ty2)) {
          if (id2 == 3 && ty2 == T_STRUCT) read_column_meta(t, &g->columns.back());
          else t.skip(ty2);
        }
      }
    } else if (id == 3 && ty == T_I64) g->num_rows = t.zigzag();
    else t.skip(ty);
  }
}
// the footer's thrift (the bytes between the last row group and the 8-byte tail)
inline Err parse_file_meta(const uint8_t* p, size_t n, FileMeta* m) {
  Thrift t(p, n);
  int last = 0, id = 0, ty = 0;
  uint32_t seen = 0;  // the struct's required fields 1 .. 4, each with its own wire type
  while (t.field(&last, &id, &ty)) {
    if (id >= 1 && id <= 4 && ty == (id == 1 ? T_I32 : id == 3 ? T_I64 : T_LIST)) seen |= 1u << id;
    if (id == 1 && ty == T_I32) m->version = t.i32();
    else if (id == 2 && ty == T_LIST) {
      int et = 0;
      uint32_t k = 0;
      if (!t.list(&et, &k)) break;
      for (uint32_t i = 0; i < k && !t.bad(); ++i) {
        if (et != T_STRUCT) {
          t.skip(et, true);
          continue;
        }
        m->schema.emplace_back();
        read_schema_element(t, &m->schema.back());
      }
    } else if (id == 3 && ty == T_I64) m->num_rows = t.zigzag();
    else if (id == 4 && ty == T_LIST) {
      int et = 0;
      uint32_t k = 0;
      if (!t.list(&et, &k)) break;
      for (uint32_t i = 0; i < k && !t.bad(); ++i) {
        if (et != T_STRUCT) {
          t.skip(et, true);
          continue;
        }
        m->row_groups.emplace_back();
        read_row_group(t, &m->row_groups.back());
      }
    } else t.skip(ty);  // key-value metadata (pyarrow's ARROW:schema blob), created_by, column orders ...
  }
  if (t.bad()) return parser_error("the footer's thrift overruns its " + num((long long)n) + " bytes");
  if (seen != 0x1Eu) return parser_error("the footer lacks a required field of FileMetaData (version, schema, num_rows, row_groups)");
  if (t.pos() != n) return parser_error("the footer's thrift ends after " + num((long long)t.pos()) + " of its " + num((long long)n) + " bytes");
  for (const RowGroupMeta& g : m->row_groups)
    if (!g.complete) return parser_error("a row group lacks a required field (columns, num_rows)");
  return Err();
}

// the 8-byte tail {u32 footer length, "PAR1"} of a file of file_size bytes
inline Err check_tail(const uint8_t tail[8], uint64_t file_size, uint32_t* footer_len) {
  if (memcmp(tail + 4, "PAR1", 4) != 0) return parser_error("the file does not end with the magic PAR1");
  const uint32_t len = (uint32_t)tail[0] | (uint32_t)tail[1] << 8 | (uint32_t)tail[2] << 16 | (uint32_t)tail[3] << 24;
  if ((uint64_t)len + 12 > file_size) return parser_error("footer length " + num(len) + " is beyond the file's " + num((long long)file_size) + " bytes");
  *footer_len = len;
  return Err();
}

// an Arrow field name is a NUL-terminated UTF-8 string
inline bool name_is_utf8(const std::string& s) {
  for (size_t i = 0; i < s.size();) {
    const unsigned char c = (unsigned char)s[i];
    const int more = c < 0x80 ? 0 : (c >> 5) == 6 ? 1 : (c >> 4) == 14 ? 2 : (c >> 3) == 30 ? 3 : -1;
    if (c == 0 || more < 0 || i + (size_t)more >= s.size() + (more ? 0 : 1)) return false;
    for (int k = 1; k <= more; ++k)
      if (((unsigned char)s[i + (size_t)k] >> 6) != 2) return false;
    i += (size_t)more + 1;
  }
  return true;
}

// the flat schema, the Arrow types and the subset: schema, types, codec, encodings, chunk extents, row counts
inline Err resolve(const FileMeta& m, uint64_t file_size, uint32_t footer_len, std::vector<Column>* cols) {
  if (m.schema.empty()) return parser_error("the footer has no schema");
  const SchemaElement& root = m.schema[0];
  cols->clear();
  for (size_t i = 1; i < m.schema.size(); ++i) {
    const SchemaElement& e = m.schema[i];
    if (!name_is_utf8(e.name)) return parser_error("the name of column " + num((long long)i - 1) + " is not UTF-8 text");
    const std::string where = "column '" + e.name + "'";
    if (e.num_children > 0 || e.type < 0) return not_implemented(where + " is a group: nested schemas are not read (flat schemas only)");
    if (e.repetition == 2) return not_implemented(where + " is repeated: only required and optional fields are read");
    if (e.repetition != 0 && e.repetition != 1) return parser_error(where + " has repetition type " + num(e.repetition));
    Column c;
    c.name = e.name;
    c.optional = e.repetition == 1;
    c.physical = e.type;
    const bool annotated = e.logical >= 0 || e.converted >= 0;
    const std::string ann = e.logical >= 0 ? std::string("logical type ") + logical_name(e.logical) : std::string("converted type ") + converted_name(e.converted);
    int iw = 0;  // integer annotation: width, sign
    bool isg = true;
    if (e.logical == 10) {
      iw = e.int_width;
      isg = e.int_signed;
    } else if (e.logical < 0 && e.converted >= 11 && e.converted <= 18) {
      static const int w[] = {8, 16, 32, 64, 8, 16, 32, 64};
      iw = w[e.converted - 11];
      isg = e.converted >= 15;
    }
    switch (e.type) {
      case PT_BOOLEAN:
        if (annotated) return not_implemented(where + ": BOOLEAN with " + ann);
        c.dtype = DFX_BOOLEAN;
        break;
      case PT_INT32:
        if (!annotated) c.dtype = DFX_INT32;
        else if (iw == 8) c.dtype = isg ? DFX_INT8 : DFX_UINT8;
        else if (iw == 16) c.dtype = isg ? DFX_INT16 : DFX_UINT16;
        else if (iw == 32) c.dtype = isg ? DFX_INT32 : DFX_UINT32;
        else return not_implemented(where + ": INT32 with " + ann);
        break;
      case PT_INT64:
        if (!annotated) c.dtype = DFX_INT64;
        else if (iw == 64) c.dtype = isg ? DFX_INT64 : DFX_UINT64;
        else return not_implemented(where + ": INT64 with " + ann);
        break;
      case PT_FLOAT:
        if (annotated) return not_implemented(where + ": FLOAT with " + ann);
        c.dtype = DFX_FLOAT32;
        break;
      case PT_DOUBLE:
        if (annotated) return not_implemented(where + ": DOUBLE with " + ann);
        c.dtype = DFX_FLOAT64;
        break;
      case PT_BYTE_ARRAY:
        if (e.logical == 1 || (e.logical < 0 && e.converted == 0)) c.dtype = DFX_UTF8;
        else if (!annotated) return not_implemented(where + ": BYTE_ARRAY without the String annotation");
        else return not_implemented(where + ": BYTE_ARRAY with " + ann);
        break;
      default: return not_implemented(where + ": physical type " + physical_name(e.type));
    }
    cols->push_back(c);
  }
  if ((int64_t)cols->size() != (int64_t)root.num_children) return parser_error("the root names " + num(root.num_children) + " children, the schema has " + num((long long)cols->size()) + " leaves");
  const uint64_t data_end = file_size - 8 - footer_len;
  int64_t rows = 0;
  for (size_t g = 0; g < m.row_groups.size(); ++g) {
    const RowGroupMeta& rg = m.row_groups[g];
    const std::string rgw = "row group " + num((long long)g);
    if (rg.columns.size() != cols->size()) return parser_error(rgw + " has " + num((long long)rg.columns.size()) + " column chunks for " + num((long long)cols->size()) + " columns");
    if (rg.num_rows < 0 || rg.num_rows > (int64_t)0x7FFFFFFF) return parser_error(rgw + " claims " + num(rg.num_rows) + " rows");
    rows += rg.num_rows;
    for (size_t c = 0; c < rg.columns.size(); ++c) {
      const ChunkMeta& k = rg.columns[c];
      const std::string where = "column '" + (*cols)[c].name + "', " + rgw;
      if (!k.has_meta) return parser_error(where + ": the chunk's metadata lacks a required field");
      if (k.type != (*cols)[c].physical) return parser_error(where + ": the chunk is of type " + std::string(physical_name(k.type)) + ", the schema says " + physical_name((*cols)[c].physical));
      if (k.path.size() != 1 || k.path[0] != (*cols)[c].name) return parser_error(where + ": the chunk's path in the schema is not the column's name");
      if (k.codec != 0 && k.codec != 7)
        return not_implemented(where + ": codec " + codec_name(k.codec) + " (only UNCOMPRESSED and LZ4_RAW chunks are read: the device has no other decompressor)");
      for (int32_t e : k.encodings)
        if (e != 0 && e != 2 && e != 3 && e != 4 && e != 8) return not_implemented(where + ": encoding " + std::string(encoding_name(e)) + " (" + num(e) + ")");
      if (k.codec == 0 && k.total_uncompressed_size != k.total_compressed_size) return parser_error(where + ": sizes " + num(k.total_uncompressed_size) + " / " + num(k.total_compressed_size) + " differ in an UNCOMPRESSED chunk");
      if (k.num_values != rg.num_rows) return parser_error(where + ": " + num(k.num_values) + " values in a row group of " + num(rg.num_rows) + " rows");
      if (k.dictionary_page_offset < 0 || k.data_page_offset < 0) return parser_error(where + ": a negative page offset");
      const int64_t s = k.start();
      if (rg.num_rows == 0 && k.total_compressed_size == 0) continue;  // a chunk without pages: nothing is ever read
      if (s < 4 || k.total_compressed_size < 0 || (uint64_t)s > data_end || (uint64_t)k.total_compressed_size > data_end - (uint64_t)s)
        return parser_error(where + ": the chunk's extent [" + num(s) + ", +" + num(k.total_compressed_size) + ") is beyond the file's data");
      if (k.total_compressed_size >= (int64_t)0x7FFFFFFF) return not_implemented(where + ": a column chunk of 2 GB or more");
      // (offsets into the inflated image of a compressed chunk are 32-bit as well: PqPage, PqInflatePage)
      if (k.codec == 7 && (k.total_uncompressed_size < 0 || k.total_uncompressed_size >= (int64_t)0x7FFFFFFF))
        return not_implemented(where + ": a column chunk of 2 GB or more");
    }
  }
  if (rows != m.num_rows) return parser_error("the row groups hold " + num(rows) + " rows, the file says " + num(m.num_rows));
  return Err();
}

// ---- PageHeader -------------------------------------------------------------------------------------------------------------
struct PageHeader {
  int32_t type = -1;  // 0 data page V1, 1 index page, 2 dictionary page, 3 data page V2
  int32_t uncompressed_size = -1, compressed_size = -1;
  int32_t num_values = -1, encoding = -1, def_encoding = -1;
  int32_t def_len = 0, rep_len = 0;  // V2
  bool is_compressed = true;         // V2: the bytes after the levels are compressed (a chunk with a codec; the levels never are)
  size_t header_len = 0;
};
inline void read_sub_header(Thrift& t, int kind, PageHeader* h) {
  int last = 0, id = 0, ty = 0;
  while (t.field(&last, &id, &ty)) {
    if (id == 1 && ty == T_I32) h->num_values = t.i32();
    else if (kind != 3 && id == 2 && ty == T_I32) h->encoding = t.i32();
    else if (kind == 0 && id == 3 && ty == T_I32) h->def_encoding = t.i32();
    else if (kind == 3 && id == 4 && ty == T_I32) h->encoding = t.i32();
    else if (kind == 3 && id == 5 && ty == T_I32) h->def_len = t.i32();
    else if (kind == 3 && id == 6 && ty == T_I32) h->rep_len = t.i32();
    else if (kind == 3 && id == 7 && (ty == T_TRUE || ty == T_FALSE)) h->is_compressed = t.boolean(ty);
    else t.skip(ty);  // statistics, is_sorted, num_nulls, num_rows
  }
}
inline bool parse_page_header(const uint8_t* p, size_t n, PageHeader* h) {
  Thrift t(p, n);
  int last = 0, id = 0, ty = 0;
  while (t.field(&last, &id, &ty)) {
    if (id == 1 && ty == T_I32) h->type = t.i32();
    else if (id == 2 && ty == T_I32) h->uncompressed_size = t.i32();
    else if (id == 3 && ty == T_I32) h->compressed_size = t.i32();
    else if (id == 5 && ty == T_STRUCT) read_sub_header(t, 0, h);
    else if (id == 7 && ty == T_STRUCT) read_sub_header(t, 2, h);
    else if (id == 8 && ty == T_STRUCT) read_sub_header(t, 3, h);
    else t.skip(ty);
  }
  h->header_len = t.pos();
  return !t.bad() && h->type >= 0;
}

// ---- one column chunk: its pages -------------------------------------------------------------------------------------------
struct PageInfo {  // what the tests compare with pyarrow's view of the file
  int kind = 0, encoding = 0;
  int64_t num_values = 0;
};
struct WalkedChunk {
  std::vector<PqPage> pages;  // data pages, in row order
  std::vector<PageInfo> infos;  // every page, the dictionary page included
  bool has_dict = false;
  uint32_t dict_off = 0, dict_len = 0, dict_n = 0;  // the dictionary's PLAIN values
  std::vector<uint32_t> dict_str;  // Utf8: offset of every entry's length prefix, plus the end (dict_n + 1)
  std::vector<uint32_t> str_offs;  // PLAIN Utf8 data pages: the same per page, pages back to back (PqPage::str_base)
  uint32_t dense_total = 0, rank_total = 0;
  long long dict_pages = 0, dict_data_pages = 0, plain_pages = 0, walked_strings = 0;  // dictionary pages; data pages of indices / PLAIN values
  uint32_t encodings_seen = 0;  // bit per PQ_ENC_*
};
inline int physical_width(int pt) { return pt == PT_INT32 || pt == PT_FLOAT ? 4 : pt == PT_INT64 || pt == PT_DOUBLE ? 8 : 0; }

// offsets of the 4-byte length prefixes of the strings in [off, off + len) of the chunk, at most max_n of them, plus the end
inline bool walk_length_chain(const uint8_t* chunk, uint32_t off, uint32_t len, uint64_t max_n, bool to_end, std::vector<uint32_t>* out, uint32_t* n_out) {
  uint64_t pos = off, end = (uint64_t)off + len, n = 0;
  while (n < max_n && (to_end ? pos < end : true)) {
    if (end - pos < 4) return false;
    const uint32_t l = (uint32_t)chunk[pos] | (uint32_t)chunk[pos + 1] << 8 | (uint32_t)chunk[pos + 2] << 16 | (uint32_t)chunk[pos + 3] << 24;
    if (l > end - pos - 4) return false;
    out->push_back((uint32_t)pos);
    pos += 4 + (uint64_t)l;
    ++n;
  }
  out->push_back((uint32_t)pos);
  *n_out = (uint32_t)n;
  return true;
}

// The bytes a page's body is read from.  The body pass reads little of a body: the 4-byte length of a V1 page's definition levels,
// the index width byte, the 4-byte length of RLE Booleans, and the length chains of BYTE_ARRAY values.  For an uncompressed chunk
// `base` is the chunk; for a compressed one it is the inflated image where the host has it (BYTE_ARRAY chunks), and null where
// only the page's prologue came back from the device (dfx_parquet_lz4.hpp: PqPrologue), which holds the first three.
struct PageBytes {
  const uint8_t* base = nullptr;
  uint32_t body = 0;  // the page's body within `base`
  PqPrologue pro{0, 0};
  uint64_t probe_off = 0;  // body offset of pro.probe
  bool le32(uint32_t off, uint32_t* v) const {
    if (base) *v = (uint32_t)base[off] | (uint32_t)base[off + 1] << 8 | (uint32_t)base[off + 2] << 16 | (uint32_t)base[off + 3] << 24;
    else if (off == body) *v = pro.word0;
    else if ((uint64_t)off == (uint64_t)body + probe_off) *v = pro.probe;
    else return false;
    return true;
  }
};
inline std::string page_where(const std::string& where, int page_no, size_t pos) {
  return where + ", page " + num(page_no) + " at byte " + num((long long)pos) + " of the chunk";
}

// The body pass of one page: the page's entry in the page table, its offsets relative to b.base's first byte.  [body, body + size)
// is the page's uncompressed body and lies inside what b.base points to.  rows: the rows of the pages before it, updated.
inline Err walk_page(const PageHeader& h, const std::string& pw, const PageBytes& b, uint32_t body, uint32_t size, const Column& col, int64_t rg_rows,
                     int64_t* rows_io, WalkedChunk* w) {
  const int width = physical_width(col.physical);
  const int64_t rows = *rows_io;
  auto unread = [&] { return parser_error(pw + ": the body pass asks for bytes of the page that were not read back"); };
  if (h.type == 1) return Err();  // index page: skipped, never interpreted
  if (h.type != 0 && h.type != 2 && h.type != 3) return parser_error(pw + ": page type " + num(h.type));
  if (h.num_values < 0) return parser_error(pw + ": " + num(h.num_values) + " values");
  PageInfo info;
  info.kind = h.type;
  info.encoding = h.encoding;
  info.num_values = h.num_values;
  w->infos.push_back(info);
  if (h.type == 2) {
    if (w->has_dict || !w->pages.empty()) return parser_error(pw + ": a dictionary page that is not the chunk's first page");
    if (h.encoding != 0 && h.encoding != 2) return not_implemented(pw + ": dictionary page encoded " + std::string(encoding_name(h.encoding)));
    if (col.physical == PT_BOOLEAN) return parser_error(pw + ": a dictionary page in a BOOLEAN chunk");
    w->has_dict = true;
    w->dict_off = body;
    w->dict_len = size;
    w->dict_n = (uint32_t)h.num_values;
    if (col.physical == PT_BYTE_ARRAY) {
      uint32_t n = 0;
      if (!b.base) return unread();
      if (!walk_length_chain(b.base, body, size, (uint64_t)h.num_values, false, &w->dict_str, &n))
        return parser_error(pw + ": a string length of the dictionary overruns its page");
      w->walked_strings += n;
    } else if ((uint64_t)h.num_values * (uint64_t)width > size) {
      return parser_error(pw + ": " + num(h.num_values) + " dictionary values overrun the page's " + num(size) + " bytes");
    }
    ++w->dict_pages;
    return Err();
  }
  if ((int64_t)h.num_values > rg_rows - rows) return parser_error(pw + ": page value counts exceed the row group's " + num(rg_rows) + " rows");
  PqPage p;
  memset(&p, 0, sizeof(p));
  p.num_values = (uint32_t)h.num_values;
  p.first_row = (uint32_t)rows;
  p.dense_base = w->dense_total;
  p.rank_base = w->rank_total;
  uint32_t voff = body, vlen = size;
  if (h.type == 0) {
    if (col.optional) {
      if (h.def_encoding != 3) return not_implemented(pw + ": definition levels encoded " + std::string(encoding_name(h.def_encoding)));
      if (vlen < 4) return parser_error(pw + ": no room for the length of the definition levels");
      uint32_t l = 0;
      if (!b.le32(voff, &l)) return unread();
      if (l > vlen - 4) return parser_error(pw + ": the definition levels' " + num(l) + " bytes overrun the page");
      p.lev_off = voff + 4;
      p.lev_len = l;
      voff += 4 + l;
      vlen -= 4 + l;
    }
  } else {
    if (h.rep_len != 0) return not_implemented(pw + ": repetition levels in a flat column");
    if (h.def_len < 0 || (uint32_t)h.def_len > vlen) return parser_error(pw + ": the definition levels' " + num(h.def_len) + " bytes overrun the page");
    if (col.optional) {
      p.lev_off = voff;
      p.lev_len = (uint32_t)h.def_len;
    }
    voff += (uint32_t)h.def_len;
    vlen -= (uint32_t)h.def_len;
  }
  if (h.encoding == 0) {
    p.enc = PQ_ENC_PLAIN;
    if (col.physical == PT_BYTE_ARRAY) {
      p.str_base = (uint32_t)w->str_offs.size();
      uint32_t n = 0;
      if (!b.base) return unread();
      if (!walk_length_chain(b.base, voff, vlen, (uint64_t)h.num_values, true, &w->str_offs, &n))
        return parser_error(pw + ": a string length overruns its page");
      p.pad = n;  // strings the page holds
      w->walked_strings += n;
    }
    ++w->plain_pages;
  } else if (h.encoding == 2 || h.encoding == 8) {
    if (!w->has_dict) return parser_error(pw + ": dictionary-encoded values without a dictionary page");
    if (vlen < 1) return parser_error(pw + ": no room for the bit width of the dictionary indices");
    p.enc = PQ_ENC_DICT;
    ++w->dict_data_pages;
    uint32_t first = 0;  // (the width byte is the low byte of the word at voff; a page that ends inside the word is read to its end)
    if (b.base) first = b.base[voff];
    else if (!b.le32(voff, &first)) return unread();
    p.bit_width = first & 0xFFu;
    if (p.bit_width > 32) return parser_error(pw + ": dictionary indices of " + num(p.bit_width) + " bits");
    voff += 1;
    vlen -= 1;
  } else if (h.encoding == 3 && col.physical == PT_BOOLEAN) {
    if (vlen < 4) return parser_error(pw + ": no room for the length of the RLE values");
    uint32_t l = 0;
    if (!b.le32(voff, &l)) return unread();
    if (l > vlen - 4) return parser_error(pw + ": the RLE values' " + num(l) + " bytes overrun the page");
    p.enc = PQ_ENC_RLE_BOOL;
    voff += 4;
    vlen = l;
  } else {
    return not_implemented(pw + ": values encoded " + std::string(encoding_name(h.encoding)) + " (" + num(h.encoding) + ")");
  }
  p.val_off = voff;
  p.val_len = vlen;
  w->encodings_seen |= 1u << p.enc;
  *rows_io = rows + h.num_values;
  w->dense_total += p.num_values;
  w->rank_total += (uint32_t)(((uint64_t)p.first_row + p.num_values + 63) / 64 - p.first_row / 64) + 1;
  w->pages.push_back(p);
  return Err();
}
inline Err rows_error(int64_t rows, int64_t rg_rows, const std::string& where) {
  if (rows != rg_rows) return parser_error(where + ": the pages hold " + num(rows) + " values, the row group has " + num(rg_rows) + " rows");
  return Err();
}

// An UNCOMPRESSED chunk: header and body of every page in one walk over the chunk's bytes, which are the bytes the page table points
// into.  chunk: the chunk's len bytes (len < 2^31).  where: "column 'x', row group g" for the messages.
inline Err walk_chunk(const uint8_t* chunk, size_t len, const Column& col, int64_t rg_rows, const std::string& where, WalkedChunk* w) {
  size_t pos = 0;
  int64_t rows = 0;
  int page_no = 0;
  while (pos < len) {
    const std::string pw = page_where(where, page_no, pos);
    PageHeader h;
    if (!parse_page_header(chunk + pos, len - pos, &h)) return parser_error(pw + ": the page header's thrift overruns the chunk");
    if (h.compressed_size < 0 || (size_t)h.compressed_size > len - pos - h.header_len)
      return parser_error(pw + ": the page's " + num(h.compressed_size) + " bytes are beyond the chunk's extent");
    if (h.uncompressed_size != h.compressed_size) return parser_error(pw + ": sizes " + num(h.uncompressed_size) + " / " + num(h.compressed_size) + " differ in an UNCOMPRESSED chunk");
    const uint32_t body = (uint32_t)(pos + h.header_len), size = (uint32_t)h.compressed_size;
    pos += h.header_len + size;
    ++page_no;
    PageBytes b;
    b.base = chunk;
    b.body = body;
    const Err e = walk_page(h, pw, b, body, size, col, rg_rows, &rows, w);
    if (!e.ok()) return e;
  }
  return rows_error(rows, rg_rows, where);
}

// ---- a compressed chunk: the header pass, the inflated image, the body pass -----------------------------------------------------
// The header pass needs the file's bytes only.  Per page (index pages are skipped) it keeps the parsed header and gives the page's
// entry of the inflate table: where the body lies in the chunk, how much of it is V2's uncompressed level prefix, and where the body
// goes in the INFLATED IMAGE, in which the bodies sit back to back, 8-byte aligned, the dictionary page first (it is the chunk's
// first page).  Nothing is sized by a number from the file that has not been checked: an uncompressed size beyond what a block of
// the compressed size can hold (an extension byte adds at most 255 bytes of output, so no valid LZ4 block exceeds 255 x its size
// + 64) is refused here, before the image is allocated.
struct HeaderPage {
  PageHeader h;
  int page_no = 0;
  size_t pos = 0;  // of the header in the chunk
  PqInflatePage ip;
};
struct ChunkHeaders {
  std::vector<HeaderPage> pages;
  uint64_t image_len = 0;
  long long inflated_pages = 0, stored_pages = 0, inflated_bytes = 0;  // inflated_bytes: of image produced (V2 prefixes are copies)
  long long oversized_v1_pages = 0;  // pages whose block is larger than what it inflates to (legal: the writer compresses anyway)
  std::vector<PqInflatePage> table() const {
    std::vector<PqInflatePage> t;
    for (const HeaderPage& p : pages) t.push_back(p.ip);
    return t;
  }
};
inline Err walk_headers(const uint8_t* chunk, size_t len, int32_t codec, const Column& col, const std::string& where, ChunkHeaders* out) {
  size_t pos = 0;
  int page_no = 0;
  while (pos < len) {
    const std::string pw = page_where(where, page_no, pos);
    HeaderPage hp;
    PageHeader& h = hp.h;
    if (!parse_page_header(chunk + pos, len - pos, &h)) return parser_error(pw + ": the page header's thrift overruns the chunk");
    if (h.compressed_size < 0 || (size_t)h.compressed_size > len - pos - h.header_len)
      return parser_error(pw + ": the page's " + num(h.compressed_size) + " bytes are beyond the chunk's extent");
    hp.page_no = page_no;
    hp.pos = pos;
    const uint32_t body = (uint32_t)(pos + h.header_len);
    pos += h.header_len + (size_t)h.compressed_size;
    ++page_no;
    if (h.type == 1) continue;  // index page: skipped, never interpreted, never inflated
    if (h.type != 0 && h.type != 2 && h.type != 3) return parser_error(pw + ": page type " + num(h.type));
    int64_t prefix = 0;
    if (h.type == 3) {
      if (h.rep_len < 0 || h.def_len < 0 || (int64_t)h.rep_len + h.def_len > (int64_t)h.compressed_size)
        return parser_error(pw + ": the levels' " + num(h.rep_len) + " + " + num(h.def_len) + " bytes overrun the page");
      prefix = (int64_t)h.rep_len + h.def_len;
    }
    if (h.uncompressed_size < 0 || (int64_t)h.uncompressed_size < prefix)
      return parser_error(pw + ": an uncompressed size of " + num(h.uncompressed_size) + " bytes is below the levels' " + num(prefix));
    const bool compressed = h.type != 3 || h.is_compressed;
    if (compressed && (int64_t)h.uncompressed_size > 255ll * h.compressed_size + 64)
      return parser_error(pw + ": an uncompressed size of " + num(h.uncompressed_size) + " bytes is more than a block of " + num(h.compressed_size) + " bytes can hold");
    if (!compressed && h.uncompressed_size != h.compressed_size)
      return parser_error(pw + ": sizes " + num(h.uncompressed_size) + " / " + num(h.compressed_size) + " differ in a page that is not compressed");
    const uint64_t dst = (out->image_len + 7) & ~7ull;
    if (dst + (uint64_t)h.uncompressed_size >= 0x7FFFFFFFull) return not_implemented(pw + ": the chunk's pages inflate to 2 GB or more");
    memset(&hp.ip, 0, sizeof(hp.ip));
    hp.ip.src_off = body;
    hp.ip.src_len = (uint32_t)h.compressed_size;
    hp.ip.dst_off = (uint32_t)dst;
    hp.ip.dst_len = (uint32_t)h.uncompressed_size;
    hp.ip.prefix_len = (uint32_t)prefix;
    hp.ip.flags = compressed ? PQ_INFLATE_COMPRESSED : 0u;
    hp.ip.codec = (uint32_t)codec;
    if (h.type == 0 && col.optional) hp.ip.flags |= PQ_INFLATE_PROBE_AFTER_LEVELS;  // the values follow the level block
    if (h.type == 3) hp.ip.probe_off = (uint32_t)h.def_len;                          // ... the (uncompressed) levels
    out->image_len = dst + (uint64_t)h.uncompressed_size;
    if (compressed) ++out->inflated_pages; else ++out->stored_pages;
    out->inflated_bytes += (long long)h.uncompressed_size - prefix;
    if (h.type != 3 && h.compressed_size > h.uncompressed_size) ++out->oversized_v1_pages;
    out->pages.push_back(hp);
  }
  return Err();
}

// the inflate stage on the host, page by page as the kernel does it: prefix and stored pages are copies.  image: image_len bytes,
// zeroed.  false: the page's block is malformed (PQ_ERR_INFLATE).
inline bool inflate_page(const uint8_t* chunk, const PqInflatePage& ip, uint8_t* image, Lz4Stats* stats) {
  memcpy(image + ip.dst_off, chunk + ip.src_off, ip.prefix_len);
  const uint8_t* src = chunk + ip.src_off + ip.prefix_len;
  uint8_t* dst = image + ip.dst_off + ip.prefix_len;
  const uint32_t src_len = ip.src_len - ip.prefix_len, dst_len = ip.dst_len - ip.prefix_len;
  if (!(ip.flags & PQ_INFLATE_COMPRESSED)) {
    memcpy(dst, src, dst_len);  // (== src_len: walk_headers)
    if (stats) ++stats->stored_pages;
    return true;
  }
  return lz4_decode_block(src, src_len, dst, dst_len, stats);
}
inline PqPrologue page_prologue(const uint8_t* image, const PqInflatePage& ip) {
  PqPrologue p;
  p.word0 = pq_le32_or_zero(image + ip.dst_off, ip.dst_len, 0);
  p.probe = pq_le32_or_zero(image + ip.dst_off, ip.dst_len, pq_probe_offset(ip, p.word0));
  return p;
}

// The body pass: the same page table, checks and messages as walk_chunk's, the offsets pointing into the inflated image.  image:
// the image's bytes, or null where only the prologues (one per page of hd) are known: enough for fixed-width and Boolean chunks.
inline Err walk_bodies(const ChunkHeaders& hd, const uint8_t* image, const PqPrologue* prologues, const Column& col, int64_t rg_rows, const std::string& where,
                       WalkedChunk* w) {
  int64_t rows = 0;
  for (size_t i = 0; i < hd.pages.size(); ++i) {
    const HeaderPage& hp = hd.pages[i];
    PageBytes b;
    b.base = image;
    b.body = hp.ip.dst_off;
    b.pro = prologues[i];
    b.probe_off = pq_probe_offset(hp.ip, b.pro.word0);
    const Err e = walk_page(hp.h, page_where(where, hp.page_no, hp.pos), b, hp.ip.dst_off, hp.ip.dst_len, col, rg_rows, &rows, w);
    if (!e.ok()) return e;
  }
  return rows_error(rows, rg_rows, where);
}

// The bytes of a Utf8 column of one row group must fit Arrow's 32-bit offsets.  The sum is NOT bounded by the chunk: the rows of a
// dictionary-encoded page take their lengths from the dictionary, so one long entry referenced by many rows sums past 2^31 from a
// small file.  Both sides sum in 64 bits and ask this before anything is sized by the total.  (The comparison is the library's one
// rule, dfx_scan_rules.hpp: the sort, the resident table, the CSV source and the filter ask it of their scan's 64-bit total.)
inline Err utf8_total_error(uint64_t total_bytes, const std::string& where) {
  if (utf8_total_exceeds_offsets(total_bytes))
    return Err{DFX_EXECUTION_ERROR, "Utf8 column of a Parquet row group exceeds 2 GB (Arrow Utf8 offsets are 32-bit): " + where + " holds " +
                                        num((long long)total_bytes) + " bytes"};
  return Err();
}

// ---- the sequential decoder (CPU tests; the kernels compute the same from the same page table) --------------------------------
struct DecodedColumn {
  std::vector<uint8_t> valid;      // one byte per row
  std::vector<uint64_t> bits;      // fixed width / Boolean: the value's bit pattern in the Arrow type's width (0 in null slots)
  std::vector<std::string> strs;   // Utf8
  uint64_t rle_runs = 0, packed_runs = 0;
};
inline uint64_t narrow_bits(int dtype, uint64_t raw) {
  switch (dtype) {
    case DFX_INT8:
    case DFX_UINT8: return raw & 0xFFull;
    case DFX_INT16:
    case DFX_UINT16: return raw & 0xFFFFull;
    case DFX_INT32:
    case DFX_UINT32:
    case DFX_FLOAT32: return raw & 0xFFFFFFFFull;
    default: return raw;
  }
}
inline Err decode_chunk(const uint8_t* chunk, const Column& col, const WalkedChunk& w, int64_t rg_rows, const std::string& where, DecodedColumn* d) {
  const int width = physical_width(col.physical);
  const bool utf8 = col.physical == PT_BYTE_ARRAY;
  d->valid.assign((size_t)rg_rows, 1);
  if (utf8) d->strs.assign((size_t)rg_rows, std::string());
  else d->bits.assign((size_t)rg_rows, 0);
  auto fixed_at = [&](uint32_t off) {
    uint64_t v = 0;
    for (int k = 0; k < width; ++k) v |= (uint64_t)chunk[off + k] << (8 * k);
    return narrow_bits(col.dtype, v);
  };
  auto str_at = [&](const std::vector<uint32_t>& offs, uint32_t i) { return std::string((const char*)chunk + offs[i] + 4, offs[i + 1] - offs[i] - 4); };
  auto len_at = [&](const std::vector<uint32_t>& offs, uint32_t i) { return (uint64_t)(offs[i + 1] - offs[i] - 4); };
  std::vector<uint32_t> lev, idx;
  uint64_t total_bytes = 0;
  // a Utf8 column is walked twice: first only its bytes are summed (utf8_total_error: nothing is materialised for a column that
  // Arrow's offsets cannot hold), then the strings are made
  for (int pass = utf8 ? 0 : 1; pass < 2; ++pass) {
  const bool measure = pass == 0;
  uint64_t* rle_runs = measure ? nullptr : &d->rle_runs;
  uint64_t* packed_runs = measure ? nullptr : &d->packed_runs;
  for (size_t pi = 0; pi < w.pages.size(); ++pi) {
    const PqPage& p = w.pages[pi];
    const std::string pw = where + ", data page " + num((long long)pi);
    uint32_t err = 0;
    uint64_t nonnull = p.num_values;
    if (col.optional && p.lev_len > 0) {
      lev.assign(p.num_values, 0);
      const uint64_t got = pq_decode_hybrid(chunk + p.lev_off, p.lev_len, 1, p.num_values, lev.data(), &err, rle_runs, packed_runs);
      if (err) return parser_error(pw + ": a run of the definition levels overruns the page");
      if (got != p.num_values) return parser_error(pw + ": " + num((long long)got) + " definition levels for " + num(p.num_values) + " values");
      nonnull = 0;
      for (uint32_t i = 0; i < p.num_values; ++i) {
        d->valid[p.first_row + i] = (uint8_t)lev[i];
        nonnull += lev[i];
      }
    }
    if (p.enc != PQ_ENC_PLAIN) {
      idx.assign((size_t)nonnull, 0);
      const uint64_t got = pq_decode_hybrid(chunk + p.val_off, p.val_len, p.enc == PQ_ENC_DICT ? p.bit_width : 1, nonnull, idx.data(), &err, rle_runs, packed_runs);
      if (err) return parser_error(pw + ": a run of the values overruns the page");
      if (got != nonnull) return parser_error(pw + ": " + num((long long)got) + " values for " + num((long long)nonnull) + " non-null rows");
    }
    uint64_t j = 0;
    for (uint32_t i = 0; i < p.num_values; ++i) {
      const size_t r = (size_t)p.first_row + i;
      if (!d->valid[r]) continue;
      if (p.enc == PQ_ENC_PLAIN) {
        if (utf8) {
          if (j >= p.pad) return parser_error(pw + ": " + num(p.pad) + " strings for more non-null rows");
          if (measure) total_bytes += len_at(w.str_offs, p.str_base + (uint32_t)j);
          else d->strs[r] = str_at(w.str_offs, p.str_base + (uint32_t)j);
        } else if (col.physical == PT_BOOLEAN) {
          if (j >= (uint64_t)p.val_len * 8) return parser_error(pw + ": the values overrun the page");
          d->bits[r] = (chunk[p.val_off + (j >> 3)] >> (j & 7)) & 1;
        } else {
          if ((j + 1) * (uint64_t)width > p.val_len) return parser_error(pw + ": the values overrun the page");
          d->bits[r] = fixed_at(p.val_off + (uint32_t)j * (uint32_t)width);
        }
      } else if (p.enc == PQ_ENC_RLE_BOOL) {
        d->bits[r] = idx[(size_t)j];
      } else {
        const uint32_t k = idx[(size_t)j];
        if (k >= w.dict_n) return parser_error(pw + ": dictionary index " + num(k) + " is beyond the dictionary's " + num(w.dict_n) + " entries");
        if (utf8 && measure) total_bytes += len_at(w.dict_str, k);
        else if (utf8) d->strs[r] = str_at(w.dict_str, k);
        else d->bits[r] = fixed_at(w.dict_off + k * (uint32_t)width);
      }
      ++j;
    }
  }
  if (measure) {
    const Err e = utf8_total_error(total_bytes, where);
    if (!e.ok()) return e;
  }
  }
  return Err();
}

}  // namespace pq
}  // namespace dfx
