// parquet_write_check.cpp -- the Parquet writer's two HIP-free headers (csrc/dfx_parquet_thrift_write.hpp, csrc/dfx_parquet_enc.hpp) as
// a stand-alone program (tests/test_parquet_write_host.py builds it plain and under the host sanitizers; tests/test_gpu_parquet_write.py
// takes the expected bytes of every file from it):
//   write DESC OUT   the columns described in DESC written as a whole Parquet file by the sequential host encoder, then OUT read
//                    again, parsed and decoded by the READER's headers (csrc/dfx_parquet_meta.hpp) and compared with the source, value
//                    by value; the footer, the pages with the run kind read from their level bytes, and the verdict as JSON
//   fits L V ...     the i32 size rule on pairs of made-up {level bytes, value bytes}: one 0 / 1 per pair
//   damage FILE      FILE truncated at every length and every byte of its footer set to 0x00, 0x7f, 0xff one at a time: a truncation
//                    must be an error, a byte change an error or a file that still parses; nothing may read out of bounds
// Every buffer the encoder reads is an exact-size heap copy, every page is encoded into a vector of exactly its size, and the file is
// parsed from an exact-size copy, so a read or a write past an end is the sanitizer's to see.
//
// DESC (little-endian): "PQWD", u64 row_group_rows, u64 page_rows, u32 columns, per column {u32 name bytes, name, u32 dtype, u32 nullable},
// u32 batches, per batch {u64 rows, per column {u64 offset (rows AND bits before row 0 in every buffer), then four buffers, each
// u64 bytes + the bytes: validity (0 bytes: none), values, offsets, data}}.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../datafusion_archive_amd/csrc/dfx_parquet_enc.hpp"
#include "../../datafusion_archive_amd/csrc/dfx_parquet_meta.hpp"

using namespace dfx;

struct Heap {  // an exact-size heap copy
  uint8_t* p = nullptr;
  size_t n = 0;
  Heap() {}
  Heap(const Heap&) = delete;
  Heap& operator=(const Heap&) = delete;
  Heap(Heap&& o) : p(o.p), n(o.n) { o.p = nullptr; }
  ~Heap() { free(p); }
  void take(const uint8_t* src, size_t len) {
    p = (uint8_t*)malloc(len ? len : 1);
    n = len;
    if (len) memcpy(p, src, len);
  }
};
struct BatchColumn {
  uint64_t offset = 0;
  Heap validity, values, offsets, data;
};
struct Batch {
  uint64_t rows = 0;
  std::vector<BatchColumn> cols;
};
struct Desc {
  uint64_t row_group_rows = 0, page_rows = 0;
  std::vector<pqw::ColumnSpec> cols;
  std::vector<Batch> batches;
};

static bool read_file(const char* path, std::vector<uint8_t>* out) {
  FILE* fp = !strcmp(path, "-") ? stdin : fopen(path, "rb");
  if (!fp) return false;
  uint8_t buf[65536];
  size_t got;
  while ((got = fread(buf, 1, sizeof(buf), fp)) > 0) out->insert(out->end(), buf, buf + got);
  if (fp != stdin) fclose(fp);
  return true;
}

struct Cursor {
  const uint8_t* p;
  size_t n, pos = 0;
  bool bad = false;
  bool need(size_t k) {
    if (bad || k > n - pos) bad = true;
    return !bad;
  }
  uint32_t u32() {
    if (!need(4)) return 0;
    uint32_t v;
    memcpy(&v, p + pos, 4);
    pos += 4;
    return v;
  }
  uint64_t u64() {
    if (!need(8)) return 0;
    uint64_t v;
    memcpy(&v, p + pos, 8);
    pos += 8;
    return v;
  }
  void heap(Heap* h) {
    const uint64_t len = u64();
    if (!need((size_t)len)) return;
    h->take(p + pos, (size_t)len);
    pos += (size_t)len;
  }
};

static bool parse_desc(const std::vector<uint8_t>& raw, Desc* d) {
  Cursor c{raw.data(), raw.size()};
  if (!c.need(4) || memcmp(raw.data(), "PQWD", 4) != 0) return false;
  c.pos = 4;
  d->row_group_rows = c.u64();
  d->page_rows = c.u64();
  const uint32_t n_cols = c.u32();
  for (uint32_t i = 0; i < n_cols && !c.bad; ++i) {
    pqw::ColumnSpec s;
    const uint32_t len = c.u32();
    if (!c.need(len)) break;
    s.name.assign((const char*)raw.data() + c.pos, len);
    c.pos += len;
    s.dtype = (int)c.u32();
    s.nullable = c.u32() != 0;
    d->cols.push_back(s);
  }
  const uint32_t n_batches = c.u32();
  for (uint32_t b = 0; b < n_batches && !c.bad; ++b) {
    d->batches.emplace_back();
    Batch& bt = d->batches.back();
    bt.rows = c.u64();
    bt.cols.resize(n_cols);
    for (uint32_t i = 0; i < n_cols && !c.bad; ++i) {
      bt.cols[i].offset = c.u64();
      c.heap(&bt.cols[i].validity);
      c.heap(&bt.cols[i].values);
      c.heap(&bt.cols[i].offsets);
      c.heap(&bt.cols[i].data);
    }
  }
  return !c.bad && c.pos == raw.size();
}

static pqw::SourceColumn source_of(const pqw::ColumnSpec& s, const BatchColumn& bc) {
  pqw::SourceColumn c;
  c.dtype = s.dtype;
  c.optional = s.nullable;
  c.validity = bc.validity.n ? bc.validity.p : nullptr;
  c.bit_offset = (int64_t)bc.offset;
  if (s.dtype == DFX_UTF8) {
    c.offsets = (const int32_t*)bc.offsets.p + bc.offset;
    c.data = bc.data.p;
  } else if (s.dtype == DFX_BOOLEAN) {
    c.values = bc.values.p;
  } else {
    c.values = bc.values.p + (size_t)bc.offset * pqw::source_width(s.dtype);
  }
  return c;
}

struct Page {
  int64_t num_values = 0, non_null = 0;
  std::vector<uint8_t> body;  // exactly the body
};

static bool put_file(void* fp, const void* p, size_t n) { return fwrite(p, 1, n, (FILE*)fp) == n; }

// the writer: the same cuts as dfx_parquet_write.cpp (groups, pieces, pages), pages held per column until their group closes
static int write_file(const Desc& d, const char* out_path, std::string* error) {
  for (const pqw::ColumnSpec& s : d.cols)
    if (!pqw::dtype_ok(s.dtype)) return *error = "column '" + s.name + "' of an unsupported type", DFX_NOT_IMPLEMENTED;
  if (!pqw::page_rows_ok((int64_t)d.page_rows) || !pqw::row_group_rows_ok((int64_t)d.row_group_rows)) return *error = "bad options", DFX_GENERAL;
  FILE* fp = fopen(out_path, "wb");
  if (!fp) return *error = "cannot create the file", DFX_IO_ERROR;
  pqw::FileWriter w(d.cols, put_file, fp);
  std::vector<std::vector<Page>> held(d.cols.size());
  int64_t group_rows = 0;
  int code = DFX_OK;
  bool ok = w.begin();
  auto close_group = [&]() {
    w.begin_row_group();
    for (size_t c = 0; c < held.size(); ++c) {
      w.begin_chunk(c);
      for (const Page& p : held[c]) ok = ok && w.add_page(p.num_values, p.non_null, p.body.data(), p.body.size());
      held[c].clear();
    }
    w.end_row_group(group_rows);
    group_rows = 0;
  };
  for (const Batch& b : d.batches) {
    for (int64_t r0 = 0; r0 < (int64_t)b.rows && code == DFX_OK;) {
      const int64_t piece = pqw::piece_rows(group_rows, (int64_t)b.rows - r0, (int64_t)d.row_group_rows);
      for (size_t c = 0; c < d.cols.size() && code == DFX_OK; ++c) {
        const pqw::SourceColumn src = source_of(d.cols[c], b.cols[c]);
        for (int64_t p0 = 0; p0 < piece; p0 += (int64_t)d.page_rows) {
          const int64_t n = std::min<int64_t>((int64_t)d.page_rows, piece - p0);
          held[c].emplace_back();
          Page& pg = held[c].back();
          pqw::EncodedPage info;
          if (!pqw::encode_page(src, r0 + p0, n, &pg.body, &info)) {
            *error = "a page of column '" + d.cols[c].name + "' is refused by the i32 size rule";
            code = DFX_EXECUTION_ERROR;
            break;
          }
          if (!d.cols[c].nullable && info.non_null != n) {
            *error = "column '" + d.cols[c].name + "' is REQUIRED and holds nulls";
            code = DFX_EXECUTION_ERROR;
            break;
          }
          pg.num_values = n;
          pg.non_null = info.non_null;
        }
      }
      r0 += piece;
      group_rows += piece;
      if (code == DFX_OK && group_rows == (int64_t)d.row_group_rows) close_group();
    }
    if (code != DFX_OK) break;
  }
  if (code == DFX_OK) {
    if (group_rows > 0) close_group();
    ok = ok && w.finish();
  }
  if (fclose(fp) != 0) ok = false;
  if (code == DFX_OK && !ok) {
    *error = "writing the file failed";
    code = DFX_IO_ERROR;
  }
  if (code != DFX_OK) remove(out_path);
  return code;
}

// ---- the way back: the reader's headers over an exact-size copy of the file --------------------------------------------------------
struct Chunk {
  pq::ChunkMeta meta;
  pq::WalkedChunk walked;
  pq::DecodedColumn decoded;
};
struct Parsed {
  std::vector<pq::Column> cols;
  pq::FileMeta meta;
  std::vector<std::vector<Chunk>> rgs;
};
static pq::Err parse_file(const uint8_t* f, size_t n, Parsed* out) {
  if (n < 12) return pq::parser_error("a file of " + pq::num((long long)n) + " bytes is too short");
  if (memcmp(f, "PAR1", 4) != 0) return pq::parser_error("the file does not start with the magic PAR1");
  uint32_t flen = 0;
  pq::Err e = pq::check_tail(f + n - 8, n, &flen);
  if (!e.ok()) return e;
  e = pq::parse_file_meta(f + n - 8 - flen, flen, &out->meta);
  if (!e.ok()) return e;
  e = pq::resolve(out->meta, n, flen, &out->cols);
  if (!e.ok()) return e;
  for (size_t g = 0; g < out->meta.row_groups.size(); ++g) {
    const pq::RowGroupMeta& rg = out->meta.row_groups[g];
    out->rgs.emplace_back(rg.columns.size());
    for (size_t c = 0; c < rg.columns.size(); ++c) {
      Chunk& k = out->rgs.back()[c];
      k.meta = rg.columns[c];
      const std::string where = "column '" + out->cols[c].name + "', row group " + pq::num((long long)g);
      const uint8_t* chunk = f + k.meta.start();
      e = pq::walk_chunk(chunk, (size_t)k.meta.total_compressed_size, out->cols[c], rg.num_rows, where, &k.walked);
      if (!e.ok()) return e;
      e = pq::decode_chunk(chunk, out->cols[c], k.walked, rg.num_rows, where, &k.decoded);
      if (!e.ok()) return e;
    }
  }
  return pq::Err();
}
static pq::Err parse_copy(const uint8_t* f, size_t n, Parsed* out) {
  Heap copy;
  copy.take(f, n);
  return parse_file(copy.p, n, out);
}

static void put_str(const std::string& s) {
  putchar('"');
  for (unsigned char c : s) {
    if (c == '"' || c == '\\') printf("\\%c", c);
    else if (c < 0x20) printf("\\u%04x", c);
    else putchar(c);
  }
  putchar('"');
}

// the decoded file against the source, row by row; "" when equal
static std::string compare(const Desc& d, const Parsed& p) {
  if (p.cols.size() != d.cols.size()) return "column count";
  for (size_t c = 0; c < d.cols.size(); ++c)
    if (p.cols[c].name != d.cols[c].name || p.cols[c].dtype != d.cols[c].dtype || p.cols[c].optional != d.cols[c].nullable) return "schema of column " + d.cols[c].name;
  size_t g = 0;
  int64_t in_group = 0;
  for (const Batch& b : d.batches)
    for (int64_t r = 0; r < (int64_t)b.rows; ++r) {
      if (g >= p.rgs.size()) return "more source rows than the file holds";
      for (size_t c = 0; c < d.cols.size(); ++c) {
        const pqw::SourceColumn src = source_of(d.cols[c], b.cols[c]);
        const pq::DecodedColumn& dec = p.rgs[g][c].decoded;
        const std::string where = "column " + d.cols[c].name + ", row group " + pq::num((long long)g) + ", row " + pq::num(in_group);
        const bool valid = pqw::source_valid(src, r);
        if ((dec.valid[(size_t)in_group] != 0) != valid) return "validity of " + where;
        if (!valid) continue;
        if (d.cols[c].dtype == DFX_UTF8) {
          const std::string want((const char*)src.data + src.offsets[r], (size_t)(src.offsets[r + 1] - src.offsets[r]));
          if (dec.strs[(size_t)in_group] != want) return "value of " + where;
        } else if (d.cols[c].dtype == DFX_BOOLEAN) {
          if (dec.bits[(size_t)in_group] != (pqw::source_bit((const uint8_t*)src.values, src.bit_offset + r) ? 1u : 0u)) return "value of " + where;
        } else {
          const uint32_t rw = pqw::source_width(d.cols[c].dtype);
          uint64_t raw = 0;
          memcpy(&raw, (const uint8_t*)src.values + (size_t)r * rw, rw);
          if (dec.bits[(size_t)in_group] != raw) return "value of " + where;
        }
      }
      if (++in_group == p.meta.row_groups[g].num_rows) {
        ++g;
        in_group = 0;
      }
    }
  if (g != p.rgs.size() || in_group != 0) return "the file holds more rows than the source";
  return "";
}

static int cmd_write(const char* desc_path, const char* out_path) {
  std::vector<uint8_t> raw;
  Desc d;
  if (!read_file(desc_path, &raw) || !parse_desc(raw, &d)) {
    fprintf(stderr, "cannot read the description\n");
    return 2;
  }
  std::string error;
  const int code = write_file(d, out_path, &error);
  if (code != DFX_OK) {
    printf("{\"code\": %d, \"error\": ", code);
    put_str(error);
    printf("}\n");
    return 0;
  }
  std::vector<uint8_t> f;
  if (!read_file(out_path, &f)) return 2;
  Parsed p;
  const pq::Err e = parse_copy(f.data(), f.size(), &p);
  if (!e.ok()) {
    printf("{\"code\": 0, \"bytes\": %zu, \"reader_code\": %d, \"reader_error\": ", f.size(), e.code);
    put_str(e.msg);
    printf("}\n");
    return 0;
  }
  printf("{\"code\": 0, \"bytes\": %zu, \"reader_code\": 0, \"num_rows\": %lld, \"mismatch\": ", f.size(), (long long)p.meta.num_rows);
  put_str(compare(d, p));
  printf(", \"columns\": [");
  for (size_t c = 0; c < p.cols.size(); ++c) {
    printf("%s{\"name\": ", c ? ", " : "");
    put_str(p.cols[c].name);
    printf(", \"dtype\": %d, \"optional\": %s, \"physical\": \"%s\"}", p.cols[c].dtype, p.cols[c].optional ? "true" : "false", pq::physical_name(p.cols[c].physical));
  }
  printf("], \"row_groups\": [");
  for (size_t g = 0; g < p.rgs.size(); ++g) {
    printf("%s{\"num_rows\": %lld, \"chunks\": [", g ? ", " : "", (long long)p.meta.row_groups[g].num_rows);
    for (size_t c = 0; c < p.rgs[g].size(); ++c) {
      const Chunk& k = p.rgs[g][c];
      printf("%s{\"start\": %lld, \"total_size\": %lld, \"num_values\": %lld, \"pages\": [", c ? ", " : "", (long long)k.meta.start(),
             (long long)k.meta.total_compressed_size, (long long)k.meta.num_values);
      for (size_t i = 0; i < k.walked.pages.size(); ++i) {
        const PqPage& pg = k.walked.pages[i];
        // the run kind from the level bytes themselves: the run's header is the block's first byte(s); bit 0 set: bit-packed
        const char* run = "none";
        if (pg.lev_len > 0) {
          const uint8_t* lev = f.data() + k.meta.start() + pg.lev_off;
          run = (lev[0] & 1) ? "packed" : lev[pg.lev_len - 1] ? "rle1" : "rle0";
        }
        printf("%s{\"num_values\": %u, \"run\": \"%s\", \"lev_len\": %u, \"val_len\": %u}", i ? ", " : "", pg.num_values, run, pg.lev_len, pg.val_len);
      }
      printf("]}");
    }
    printf("]}");
  }
  printf("]}\n");
  return 0;
}

static int cmd_fits(int argc, char** argv) {
  printf("[");
  for (int i = 2; i + 1 < argc; i += 2)
    printf("%s%d", i > 2 ? ", " : "", pqw::body_fits(strtoull(argv[i], nullptr, 10), strtoull(argv[i + 1], nullptr, 10)) ? 1 : 0);
  printf("]\n");
  return 0;
}

static int cmd_damage(const char* path) {
  std::vector<uint8_t> f;
  if (!read_file(path, &f)) return 2;
  {
    Parsed p;
    const pq::Err e = parse_copy(f.data(), f.size(), &p);
    if (!e.ok()) {
      fprintf(stderr, "the undamaged file does not parse: %s\n", e.msg.c_str());
      return 2;
    }
  }
  long long truncations = 0, flips = 0, errors = 0;
  for (size_t n = 0; n < f.size(); ++n) {
    Parsed p;
    const pq::Err e = parse_copy(f.data(), n, &p);
    if (e.ok() || e.msg.empty()) {
      fprintf(stderr, "truncation at %zu of %zu parses\n", n, f.size());
      return 1;
    }
    ++truncations;
  }
  uint32_t flen = 0;
  (void)pq::check_tail(f.data() + f.size() - 8, f.size(), &flen);
  for (size_t pos = f.size() - 8 - flen; pos < f.size(); ++pos) {
    static const uint8_t vals[3] = {0x00, 0x7f, 0xff};
    for (uint8_t v : vals) {
      if (f[pos] == v) continue;
      const uint8_t keep = f[pos];
      f[pos] = v;
      Parsed p;
      const pq::Err e = parse_copy(f.data(), f.size(), &p);
      f[pos] = keep;
      ++flips;
      if (!e.ok()) {
        if (e.msg.empty()) return 1;
        ++errors;
      }
    }
  }
  printf("{\"truncations\": %lld, \"flips\": %lld, \"errors\": %lld}\n", truncations, flips, errors);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "write")) return cmd_write(argv[2], argv[3]);
  if (argc >= 4 && argc % 2 == 0 && !strcmp(argv[1], "fits")) return cmd_fits(argc, argv);
  if (argc == 3 && !strcmp(argv[1], "damage")) return cmd_damage(argv[2]);
  fprintf(stderr, "usage: parquet_write_check write DESC|- OUT | fits LEVEL_BYTES VALUE_BYTES ... | damage FILE\n");
  return 2;
}
