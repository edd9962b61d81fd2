// dfx_parquet_thrift_write.hpp -- the writing side of thrift's compact protocol and, on top of it, the Parquet structures the
// writer (deviation D13: dfx_parquet_write.cpp) puts into a file: PageHeader / DataPageHeader, SchemaElement with its logical type,
// ColumnMetaData, ColumnChunk, RowGroup, FileMetaData; DictionaryPageHeader for the chunks written under the sink's "dictionary" option.  Free of HIP.  It is the mirror of the reader in dfx_parquet_meta.hpp: what
// is written here, that reader parses back (tests/native/parquet_write_check.cpp holds the two against each other without pyarrow).
//
//   varint    7 bits per byte, least significant first, the high bit set on every byte but the last
//   zigzag    (v << 1) ^ (v >> 63): i16 / i32 / i64 values and long-form field ids
//   field     one byte {id delta << 4 | type} when 0 < delta <= 15, else {type} followed by the zigzag id; a Boolean field carries
//             its value in the type nibble (1 true, 2 false); a struct ends with a 0 byte and field ids restart inside it
//   list      {size << 4 | element type} for size < 15, else {0xF0 | element type} followed by the varint size
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

namespace dfx {
namespace pqw {

enum : int { TW_TRUE = 1, TW_FALSE = 2, TW_BYTE = 3, TW_I16 = 4, TW_I32 = 5, TW_I64 = 6, TW_BINARY = 8, TW_LIST = 9, TW_STRUCT = 12 };

class ThriftWriter {
 public:
  explicit ThriftWriter(std::vector<uint8_t>* out) : out_(out) {}
  void varint(uint64_t v) {
    while (v >= 0x80) {
      out_->push_back((uint8_t)(v | 0x80));
      v >>= 7;
    }
    out_->push_back((uint8_t)v);
  }
  void zigzag(int64_t v) { varint(((uint64_t)v << 1) ^ (uint64_t)(v >> 63)); }
  void field(int id, int type) {
    const int delta = id - last_;
    if (delta > 0 && delta <= 15) {
      out_->push_back((uint8_t)(delta << 4 | type));
    } else {
      out_->push_back((uint8_t)type);
      zigzag(id);
    }
    last_ = id;
  }
  void i32(int id, int32_t v) {
    field(id, TW_I32);
    zigzag(v);
  }
  void i64(int id, int64_t v) {
    field(id, TW_I64);
    zigzag(v);
  }
  void byte(int id, int8_t v) {
    field(id, TW_BYTE);
    out_->push_back((uint8_t)v);
  }
  void boolean(int id, bool v) { field(id, v ? TW_TRUE : TW_FALSE); }
  void binary_value(const std::string& s) {
    varint(s.size());
    out_->insert(out_->end(), s.begin(), s.end());
  }
  void binary(int id, const std::string& s) {
    field(id, TW_BINARY);
    binary_value(s);
  }
  void list(int id, int etype, size_t n) {
    field(id, TW_LIST);
    if (n < 15) {
      out_->push_back((uint8_t)(n << 4 | (size_t)etype));
    } else {
      out_->push_back((uint8_t)(0xF0 | etype));
      varint(n);
    }
  }
  // a struct as a field (id > 0) or as a list element / the top level (id == 0): field ids restart inside, end_struct restores them
  void begin_struct(int id) {
    if (id > 0) field(id, TW_STRUCT);
    stack_.push_back(last_);
    last_ = 0;
  }
  void end_struct() {
    out_->push_back(0);
    last_ = stack_.back();
    stack_.pop_back();
  }

 private:
  std::vector<uint8_t>* out_;
  std::vector<int> stack_;
  int last_ = 0;
};

// ---- the Parquet structures (parquet.thrift; only the fields this writer sets) ---------------------------------------------------
enum : int { PHYS_BOOLEAN = 0, PHYS_INT32 = 1, PHYS_INT64 = 2, PHYS_FLOAT = 4, PHYS_DOUBLE = 5, PHYS_BYTE_ARRAY = 6 };
enum : int { ENCODING_PLAIN = 0, ENCODING_RLE = 3, ENCODING_RLE_DICTIONARY = 8 };
enum : int { REP_REQUIRED = 0, REP_OPTIONAL = 1 };
enum : int { CONV_NONE = -1, CONV_UTF8 = 0, CONV_UINT_8 = 11, CONV_UINT_16 = 12, CONV_UINT_32 = 13, CONV_UINT_64 = 14, CONV_INT_8 = 15, CONV_INT_16 = 16,
             CONV_INT_32 = 17 };
enum : int { LOGICAL_NONE = 0, LOGICAL_STRING = 1, LOGICAL_INTEGER = 10 };  // field ids of the LogicalType union

struct LeafSchema {
  std::string name;
  int physical = PHYS_INT32;
  int repetition = REP_OPTIONAL;
  int converted = CONV_NONE;
  int logical = LOGICAL_NONE;
  int int_bits = 0;  // LOGICAL_INTEGER
  bool int_signed = true;
};

// PageHeader { 1 type = DATA_PAGE, 2 uncompressed_page_size, 3 compressed_page_size, 5 DataPageHeader { 1 num_values, 2 encoding = PLAIN,
// 3 definition_level_encoding = RLE, 4 repetition_level_encoding = RLE } }: a V1 data page, no CRC, no statistics;
// encoding: PLAIN, or RLE_DICTIONARY for a page of dictionary indices; body_bytes: of the body as the file holds it;
// uncompressed_bytes: of what it inflates to in a compressed chunk (below 0: the same, an UNCOMPRESSED chunk)
inline void write_page_header(int32_t body_bytes, int32_t num_values, std::vector<uint8_t>* out, int encoding = ENCODING_PLAIN, int32_t uncompressed_bytes = -1) {
  ThriftWriter t(out);
  t.begin_struct(0);
  t.i32(1, 0);
  t.i32(2, uncompressed_bytes < 0 ? body_bytes : uncompressed_bytes);
  t.i32(3, body_bytes);
  t.begin_struct(5);
  t.i32(1, num_values);
  t.i32(2, encoding);
  t.i32(3, ENCODING_RLE);
  t.i32(4, ENCODING_RLE);
  t.end_struct();
  t.end_struct();
}
// PageHeader { 1 type = DICTIONARY_PAGE, 2 uncompressed_page_size, 3 compressed_page_size, 7 DictionaryPageHeader { 1 num_values,
// 2 encoding = PLAIN } }: the first page of a dictionary-encoded chunk
inline void write_dictionary_page_header(int32_t body_bytes, int32_t num_values, std::vector<uint8_t>* out, int32_t uncompressed_bytes = -1) {
  ThriftWriter t(out);
  t.begin_struct(0);
  t.i32(1, 2);
  t.i32(2, uncompressed_bytes < 0 ? body_bytes : uncompressed_bytes);
  t.i32(3, body_bytes);
  t.begin_struct(7);
  t.i32(1, num_values);
  t.i32(2, ENCODING_PLAIN);
  t.end_struct();
  t.end_struct();
}

inline void write_schema_root(ThriftWriter& t, int32_t n_children) {
  t.begin_struct(0);
  t.binary(4, "schema");
  t.i32(5, n_children);
  t.end_struct();
}
inline void write_schema_leaf(ThriftWriter& t, const LeafSchema& e) {
  t.begin_struct(0);
  t.i32(1, e.physical);
  t.i32(3, e.repetition);
  t.binary(4, e.name);
  if (e.converted != CONV_NONE) t.i32(6, e.converted);
  if (e.logical != LOGICAL_NONE) {
    t.begin_struct(10);  // LogicalType: a union, one member set
    t.begin_struct(e.logical);
    if (e.logical == LOGICAL_INTEGER) {
      t.byte(1, (int8_t)e.int_bits);
      t.boolean(2, e.int_signed);
    }
    t.end_struct();
    t.end_struct();
  }
  t.end_struct();
}

struct ChunkInfo {  // one column chunk of a row group, as the footer records it
  int physical = PHYS_INT32;
  bool optional = true;  // encodings: PLAIN, and RLE for the definition levels of an OPTIONAL column
  std::string name;
  int64_t num_values = 0, null_count = 0;
  int64_t total_size = 0;  // headers + bodies of its pages as the file holds them (UNCOMPRESSED: both sizes)
  int codec = 0;           // the Parquet codec id of its pages: 0 UNCOMPRESSED, 7 LZ4_RAW
  int64_t total_uncompressed_size = -1;  // headers + what the bodies inflate to (below 0: total_size, an UNCOMPRESSED chunk)
  int64_t data_page_offset = 0;
  bool has_dictionary = false;  // the chunk starts with a dictionary page: encodings PLAIN, RLE, RLE_DICTIONARY; total_size counts it
  int64_t dictionary_page_offset = 0;
};
// ColumnChunk { 2 file_offset, 3 ColumnMetaData { 1 type, 2 encodings, 3 path_in_schema, 4 codec, 5 num_values,
// 6 total_uncompressed_size, 7 total_compressed_size, 9 data_page_offset, 11 dictionary_page_offset (a chunk with a dictionary page),
// 12 Statistics { 3 null_count } } }
inline void write_column_chunk(ThriftWriter& t, const ChunkInfo& c) {
  t.begin_struct(0);
  t.i64(2, c.data_page_offset);
  t.begin_struct(3);
  t.i32(1, c.physical);
  t.list(2, TW_I32, c.has_dictionary ? 3 : c.optional ? 2 : 1);
  t.zigzag(ENCODING_PLAIN);
  if (c.optional || c.has_dictionary) t.zigzag(ENCODING_RLE);
  if (c.has_dictionary) t.zigzag(ENCODING_RLE_DICTIONARY);
  t.list(3, TW_BINARY, 1);
  t.binary_value(c.name);
  t.i32(4, c.codec);
  t.i64(5, c.num_values);
  t.i64(6, c.total_uncompressed_size < 0 ? c.total_size : c.total_uncompressed_size);
  t.i64(7, c.total_size);
  t.i64(9, c.data_page_offset);
  if (c.has_dictionary) t.i64(11, c.dictionary_page_offset);
  t.begin_struct(12);
  t.i64(3, c.null_count);
  t.end_struct();
  t.end_struct();
  t.end_struct();
}
struct RowGroupInfo {
  std::vector<ChunkInfo> chunks;
  int64_t num_rows = 0;
};
// RowGroup { 1 columns, 2 total_byte_size, 3 num_rows }
inline void write_row_group(ThriftWriter& t, const RowGroupInfo& g) {
  t.begin_struct(0);
  t.list(1, TW_STRUCT, g.chunks.size());
  int64_t total = 0;
  for (const ChunkInfo& c : g.chunks) {
    write_column_chunk(t, c);
    total += c.total_uncompressed_size < 0 ? c.total_size : c.total_uncompressed_size;  // (of the uncompressed column data)
  }
  t.i64(2, total);
  t.i64(3, g.num_rows);
  t.end_struct();
}
// FileMetaData { 1 version, 2 schema (the root, then the leaves), 3 num_rows, 4 row_groups, 6 created_by, 7 column_orders (every
// column TypeDefinedOrder: what a reader needs to trust the chunk statistics) }
inline void write_file_meta(const std::vector<LeafSchema>& leaves, const std::vector<RowGroupInfo>& groups, int64_t num_rows, const std::string& created_by,
                            std::vector<uint8_t>* out) {
  ThriftWriter t(out);
  t.begin_struct(0);
  t.i32(1, 2);
  t.list(2, TW_STRUCT, leaves.size() + 1);
  write_schema_root(t, (int32_t)leaves.size());
  for (const LeafSchema& e : leaves) write_schema_leaf(t, e);
  t.i64(3, num_rows);
  t.list(4, TW_STRUCT, groups.size());
  for (const RowGroupInfo& g : groups) write_row_group(t, g);
  t.binary(6, created_by);
  t.list(7, TW_STRUCT, leaves.size());
  for (size_t i = 0; i < leaves.size(); ++i) {
    t.begin_struct(0);  // ColumnOrder: a union
    t.begin_struct(1);  // TypeDefinedOrder {}
    t.end_struct();
    t.end_struct();
  }
  t.end_struct();
}

}  // namespace pqw
}  // namespace dfx
