// parquet_lz4_check.cpp -- the Parquet source's HIP-free headers with the inflate stage (csrc/dfx_parquet_lz4.hpp, and the header
// pass / body pass of csrc/dfx_parquet_meta.hpp) as a stand-alone program (tests/test_parquet_lz4_host.py builds it plain and under
// the host sanitizers).  A compressed chunk goes the way the device takes it: header pass -> every page inflated into the image
// (lz4_decode_block) -> the pages' prologues -> body pass (from the prologues alone unless the column is a BYTE_ARRAY) ->
// pq::decode_chunk over the image.
//   dump FILE     what parquet_check dumps, plus the LZ4 statistics summed over the file
//   damage FILE   FILE's first compressed page damaged in the ways listed below, one at a time; the code and message of each as JSON
// Every parse runs over an exact-size heap copy of the file, every block is inflated from an exact-size heap copy into an exact-size
// image, so a read or a store past an end is the sanitizer's to see.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../datafusion_archive_amd/csrc/dfx_parquet_meta.hpp"

using namespace dfx;
using namespace dfx::pq;

struct Chunk {
  ChunkMeta meta;
  ChunkHeaders headers;
  WalkedChunk walked;
  DecodedColumn decoded;
};
struct Parsed {
  std::vector<Column> cols;
  FileMeta meta;
  std::vector<std::vector<Chunk>> rgs;
  Lz4Stats lz4;
  long long inflated_pages = 0, inflated_bytes = 0, oversized_v1_pages = 0, prologue_only_chunks = 0;
};

static Err inflate_and_decode(const uint8_t* chunk, size_t len, const Column& col, int64_t rg_rows, const std::string& where, Chunk* k, Parsed* out) {
  Err e = walk_headers(chunk, len, k->meta.codec, col, where, &k->headers);
  if (!e.ok()) return e;
  const ChunkHeaders& hd = k->headers;
  uint8_t* image = (uint8_t*)calloc(hd.image_len ? hd.image_len : 1, 1);
  std::vector<PqPrologue> prologues;
  for (const HeaderPage& hp : hd.pages) {
    // the compressed part alone, in a heap block of its own size
    uint8_t* body = (uint8_t*)malloc(hp.ip.src_len ? hp.ip.src_len : 1);
    memcpy(body, chunk + hp.ip.src_off, hp.ip.src_len);
    PqInflatePage ip = hp.ip;
    ip.src_off = 0;
    const bool ok = inflate_page(body, ip, image, &out->lz4);
    free(body);
    if (!ok) {
      free(image);
      return parser_error(page_where(where, hp.page_no, hp.pos) + ": the compressed block is malformed");
    }
    prologues.push_back(page_prologue(image, hp.ip));
  }
  out->inflated_pages += hd.inflated_pages;
  out->inflated_bytes += hd.inflated_bytes;
  out->oversized_v1_pages += hd.oversized_v1_pages;
  const bool chains = col.physical == PT_BYTE_ARRAY;  // the only bodies the host reads beyond the prologue
  if (!chains) ++out->prologue_only_chunks;
  e = walk_bodies(hd, chains ? image : nullptr, prologues.data(), col, rg_rows, where, &k->walked);
  if (e.ok()) e = decode_chunk(image, col, k->walked, rg_rows, where, &k->decoded);
  free(image);
  return e;
}

static Err parse_file(const uint8_t* f, size_t n, Parsed* out) {
  if (n < 12) return parser_error("a file of " + num((long long)n) + " bytes is too short");
  if (memcmp(f, "PAR1", 4) != 0) return parser_error("the file does not start with the magic PAR1");
  uint32_t flen = 0;
  Err e = check_tail(f + n - 8, n, &flen);
  if (!e.ok()) return e;
  e = parse_file_meta(f + n - 8 - flen, flen, &out->meta);
  if (!e.ok()) return e;
  e = resolve(out->meta, n, flen, &out->cols);
  if (!e.ok()) return e;
  for (size_t g = 0; g < out->meta.row_groups.size(); ++g) {
    const RowGroupMeta& rg = out->meta.row_groups[g];
    out->rgs.emplace_back(rg.columns.size());
    for (size_t c = 0; c < rg.columns.size(); ++c) {
      Chunk& k = out->rgs.back()[c];
      k.meta = rg.columns[c];
      const std::string where = "column '" + out->cols[c].name + "', row group " + num((long long)g);
      const uint8_t* chunk = f + k.meta.start();
      const size_t len = (size_t)k.meta.total_compressed_size;
      if (k.meta.codec == 0) {
        e = walk_chunk(chunk, len, out->cols[c], rg.num_rows, where, &k.walked);
        if (e.ok()) e = decode_chunk(chunk, out->cols[c], k.walked, rg.num_rows, where, &k.decoded);
      } else {
        e = inflate_and_decode(chunk, len, out->cols[c], rg.num_rows, where, &k, out);
      }
      if (!e.ok()) return e;
    }
  }
  return Err();
}

static Err parse_copy(const uint8_t* f, size_t n, Parsed* out) {
  uint8_t* copy = (uint8_t*)malloc(n ? n : 1);
  if (n) memcpy(copy, f, n);
  Err e = parse_file(copy, n, out);
  free(copy);
  return e;
}

static bool read_file(const char* path, std::vector<uint8_t>* out) {
  FILE* fp = fopen(path, "rb");
  if (!fp) return false;
  uint8_t buf[65536];
  size_t got;
  while ((got = fread(buf, 1, sizeof(buf), fp)) > 0) out->insert(out->end(), buf, buf + got);
  fclose(fp);
  return true;
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
static void put_hex(const std::string& s) {
  putchar('"');
  for (unsigned char c : s) printf("%02x", c);
  putchar('"');
}
static void put_err(const Err& e) {
  printf("{\"code\": %d, \"error\": ", e.code);
  put_str(e.msg);
  printf("}");
}
// pyarrow's name of a codec (ColumnChunkMetaData.compression): LZ4_RAW is reported as LZ4
static const char* pyarrow_codec_name(int c) { return c == 7 ? "LZ4" : codec_name(c); }

static int dump(const char* path) {
  std::vector<uint8_t> f;
  if (!read_file(path, &f)) {
    printf("{\"error\": \"cannot read\", \"code\": %d}\n", DFX_IO_ERROR);
    return 3;
  }
  Parsed p;
  Err e = parse_copy(f.data(), f.size(), &p);
  if (!e.ok()) {
    put_err(e);
    printf("\n");
    return 3;
  }
  printf("{\"code\": 0, \"num_rows\": %lld, \"lz4\": {\"sequences\": %llu, \"lit_extensions\": %llu, \"match_extensions\": %llu, \"offset_1\": %llu, "
         "\"offset_lt8\": %llu, \"offset_ge64\": %llu, \"offset_ge32768\": %llu, \"overlapping\": %llu, \"stored_pages\": %llu, \"inflated_pages\": %lld, "
         "\"inflated_bytes\": %lld, \"oversized_v1_pages\": %lld, \"prologue_only_chunks\": %lld}, \"columns\": [",
         (long long)p.meta.num_rows, (unsigned long long)p.lz4.sequences, (unsigned long long)p.lz4.lit_extensions, (unsigned long long)p.lz4.match_extensions,
         (unsigned long long)p.lz4.offset_1, (unsigned long long)p.lz4.offset_lt8, (unsigned long long)p.lz4.offset_ge64,
         (unsigned long long)p.lz4.offset_ge32768, (unsigned long long)p.lz4.overlapping, (unsigned long long)p.lz4.stored_pages, p.inflated_pages,
         p.inflated_bytes, p.oversized_v1_pages, p.prologue_only_chunks);
  for (size_t c = 0; c < p.cols.size(); ++c) {
    printf("%s{\"name\": ", c ? ", " : "");
    put_str(p.cols[c].name);
    printf(", \"dtype\": %d, \"optional\": %s, \"physical\": \"%s\"}", p.cols[c].dtype, p.cols[c].optional ? "true" : "false", physical_name(p.cols[c].physical));
  }
  printf("], \"row_groups\": [");
  for (size_t g = 0; g < p.rgs.size(); ++g) {
    printf("%s{\"num_rows\": %lld, \"chunks\": [", g ? ", " : "", (long long)p.meta.row_groups[g].num_rows);
    for (size_t c = 0; c < p.rgs[g].size(); ++c) {
      const Chunk& k = p.rgs[g][c];
      printf("%s{\"start\": %lld, \"total_compressed_size\": %lld, \"num_values\": %lld, \"codec\": \"%s\", \"codec_id\": %d, \"data_page_offset\": %lld, "
             "\"dictionary_page_offset\": %lld, \"dict_pages\": %lld, \"plain_pages\": %lld, \"rle_runs\": %llu, \"packed_runs\": %llu, \"image_len\": %llu, \"pages\": [",
             c ? ", " : "", (long long)k.meta.start(), (long long)k.meta.total_compressed_size, (long long)k.meta.num_values, pyarrow_codec_name(k.meta.codec),
             k.meta.codec, (long long)k.meta.data_page_offset, (long long)(k.meta.has_dictionary_offset ? k.meta.dictionary_page_offset : -1), k.walked.dict_pages,
             k.walked.plain_pages, (unsigned long long)k.decoded.rle_runs, (unsigned long long)k.decoded.packed_runs, (unsigned long long)k.headers.image_len);
      for (size_t i = 0; i < k.walked.infos.size(); ++i)
        printf("%s{\"kind\": %d, \"encoding\": \"%s\", \"num_values\": %lld}", i ? ", " : "", k.walked.infos[i].kind, encoding_name(k.walked.infos[i].encoding),
               (long long)k.walked.infos[i].num_values);
      printf("], \"inflate\": [");  // the inflate table: file offsets of the bodies, image offsets of what they inflate to
      for (size_t i = 0; i < k.headers.pages.size(); ++i) {
        const HeaderPage& hp = k.headers.pages[i];
        printf("%s{\"kind\": %d, \"header_at\": %lld, \"src_off\": %lld, \"src_len\": %u, \"dst_off\": %u, \"dst_len\": %u, \"prefix_len\": %u, \"flags\": %u}", i ? ", " : "",
               hp.h.type, (long long)k.meta.start() + (long long)hp.pos, (long long)k.meta.start() + hp.ip.src_off, hp.ip.src_len, hp.ip.dst_off, hp.ip.dst_len,
               hp.ip.prefix_len, hp.ip.flags);
      }
      printf("], \"data_pages\": [");  // (offsets into the inflated image where the chunk is compressed)
      for (size_t i = 0; i < k.walked.pages.size(); ++i) {
        const PqPage& pg = k.walked.pages[i];
        printf("%s{\"enc\": %u, \"bit_width\": %u, \"lev_off\": %u, \"lev_len\": %u, \"val_off\": %u, \"val_len\": %u, \"num_values\": %u, \"first_row\": %u}",
               i ? ", " : "", pg.enc, pg.bit_width, pg.lev_off, pg.lev_len, pg.val_off, pg.val_len, pg.num_values, pg.first_row);
      }
      printf("], \"valid\": \"");
      for (uint8_t v : k.decoded.valid) putchar(v ? '1' : '0');
      printf("\", ");
      if (p.cols[c].dtype == DFX_UTF8) {
        printf("\"strs\": [");
        for (size_t i = 0; i < k.decoded.strs.size(); ++i) {
          if (i) putchar(',');
          put_hex(k.decoded.strs[i]);
        }
      } else {
        printf("\"bits\": [");
        for (size_t i = 0; i < k.decoded.bits.size(); ++i) printf("%s%llu", i ? "," : "", (unsigned long long)k.decoded.bits[i]);
      }
      printf("]}");
    }
    printf("]}");
  }
  printf("]}\n");
  return 0;
}

// ---- damage ---------------------------------------------------------------------------------------------------------------------
// the varint at f[at ...] (a zigzag i32 of a page header): its length
static size_t varint_len(const std::vector<uint8_t>& f, size_t at) {
  size_t n = 1;
  while (at + n - 1 < f.size() && (f[at + n - 1] & 0x80)) ++n;
  return n;
}
static uint64_t varint_get(const std::vector<uint8_t>& f, size_t at, size_t n) {
  uint64_t v = 0;
  for (size_t i = 0; i < n; ++i) v |= (uint64_t)(f[at + i] & 0x7F) << (7 * i);
  return v;
}
// stores v in the n bytes of the varint at f[at]; false: v does not fit n bytes (or would take fewer)
static bool varint_put(std::vector<uint8_t>* f, size_t at, size_t n, uint64_t v) {
  if ((n < 10 && (v >> (7 * n)) != 0) || (n > 1 && (v >> (7 * (n - 1))) == 0)) return false;
  for (size_t i = 0; i < n; ++i) (*f)[at + i] = (uint8_t)(((v >> (7 * i)) & 0x7F) | (i + 1 < n ? 0x80 : 0));
  return true;
}

static bool first_case = true;
static void report(const char* name, const std::vector<uint8_t>& f) {
  Parsed p;
  const Err e = parse_copy(f.data(), f.size(), &p);
  printf("%s{\"name\": \"%s\", \"result\": ", first_case ? "" : ", ", name);
  put_err(e);
  printf("}");
  first_case = false;
}
static void report_skipped(const char* name, const char* why) {
  printf("%s{\"name\": \"%s\", \"skipped\": \"%s\"}", first_case ? "" : ", ", name, why);
  first_case = false;
}

static int damage(const char* path) {
  std::vector<uint8_t> f;
  if (!read_file(path, &f)) return 2;
  Parsed p;
  {
    Err e = parse_copy(f.data(), f.size(), &p);
    if (!e.ok()) {
      fprintf(stderr, "the undamaged file does not parse: %s\n", e.msg.c_str());
      return 2;
    }
  }
  // the first compressed page with a match in it
  const Chunk* chunk = nullptr;
  const HeaderPage* page = nullptr;
  for (const auto& rg : p.rgs)
    for (const Chunk& k : rg)
      for (const HeaderPage& hp : k.headers.pages)
        if (!page && (hp.ip.flags & PQ_INFLATE_COMPRESSED) && hp.ip.src_len - hp.ip.prefix_len > 16) {
          chunk = &k;
          page = &hp;
        }
  if (!page) {
    fprintf(stderr, "no compressed page\n");
    return 2;
  }
  const size_t header_at = (size_t)chunk->meta.start() + page->pos;
  const size_t block_at = (size_t)chunk->meta.start() + page->ip.src_off + page->ip.prefix_len;
  const size_t block_len = page->ip.src_len - page->ip.prefix_len, out_len = page->ip.dst_len - page->ip.prefix_len;
  printf("{\"block_len\": %zu, \"out_len\": %zu, ", block_len, out_len);
  // 1. every truncation of the block, each in a heap block of its own size, into an image of the page's size
  size_t truncations = 0, survived = 0;
  for (size_t n = 0; n < block_len; ++n) {
    uint8_t* src = (uint8_t*)malloc(n ? n : 1);
    memcpy(src, f.data() + block_at, n);
    uint8_t* dst = (uint8_t*)calloc(out_len ? out_len : 1, 1);
    if (lz4_decode_block(src, n, dst, out_len)) ++survived;
    free(dst);
    free(src);
    ++truncations;
  }
  printf("\"truncations\": %zu, \"truncations_accepted\": %zu, \"cases\": [", truncations, survived);
  // the first match of the block: where its offset is
  Lz4Seq q;
  const bool has_match = lz4_next_sequence(f.data() + block_at, block_len, 0, 0, out_len, &q) && !q.last;
  const size_t offset_at = block_at + (size_t)q.lit_pos + q.lit_len;
  if (has_match) {
    std::vector<uint8_t> d = f;
    d[offset_at] = 0;
    d[offset_at + 1] = 0;
    report("offset_zero", d);
    d[offset_at] = 0xFF;  // 65535 bytes back, of q.lit_len produced
    d[offset_at + 1] = 0xFF;
    if (q.lit_len < 65535) report("offset_beyond_output", d);
    else report_skipped("offset_beyond_output", "the first literals are 65535 bytes or more");
  } else {
    report_skipped("offset_zero", "the block's first sequence has no match");
    report_skipped("offset_beyond_output", "the block's first sequence has no match");
  }
  {
    std::vector<uint8_t> d = f;  // a token of 15 literals whose extension never ends
    for (size_t i = 0; i < block_len; ++i) d[block_at + i] = 0xFF;
    report("length_chain_to_the_end", d);
  }
  // the page header starts {0x15 type, 0x15 uncompressed_size, 0x15 compressed_size}: i32 fields 1, 2, 3, delta-encoded ids
  const size_t usize_at = header_at + 3;
  const bool shape = f[header_at] == 0x15 && f[header_at + 2] == 0x15 && !(f[header_at + 1] & 0x80);
  const size_t vn = varint_len(f, usize_at);
  const uint64_t zz = varint_get(f, usize_at, vn);  // zigzag: 2 * size
  struct {
    const char* name;
    uint64_t value;
  } sizes[] = {{"uncompressed_size_plus_1", zz + 2}, {"uncompressed_size_minus_1", zz - 2}, {"uncompressed_size_above_cap", ((1ull << (7 * vn)) - 1) & ~1ull}};
  for (const auto& s : sizes) {
    std::vector<uint8_t> d = f;
    if (!shape || (zz & 1) || zz < 2 || !varint_put(&d, usize_at, vn, s.value)) report_skipped(s.name, "the size's varint cannot hold the value in place");
    else report(s.name, d);
  }
  printf("], \"cap_value\": %llu, \"cap\": %llu}\n", (unsigned long long)((((1ull << (7 * vn)) - 1) & ~1ull) >> 1), 255ull * page->ip.src_len + 64);
  return 0;
}

// V2: the page header's definition_levels_byte_length (field 5 of DataPageHeaderV2) raised above the page's uncompressed size
static int damage_v2(const char* path) {
  std::vector<uint8_t> f;
  if (!read_file(path, &f)) return 2;
  Parsed p;
  Err e = parse_copy(f.data(), f.size(), &p);
  if (!e.ok()) {
    fprintf(stderr, "the undamaged file does not parse: %s\n", e.msg.c_str());
    return 2;
  }
  printf("{\"cases\": [");
  for (const auto& rg : p.rgs)
    for (const Chunk& k : rg)
      for (const HeaderPage& hp : k.headers.pages) {
        if (hp.h.type != 3 || hp.h.def_len <= 0) continue;
        // find the varint of def_len inside the header: the only place where zigzag(def_len) follows a field byte 0x15 and the
        // header re-parses to the changed value
        const size_t at0 = (size_t)k.meta.start() + hp.pos;
        for (size_t i = at0 + 1; i < at0 + hp.h.header_len; ++i) {
          const size_t vn = varint_len(f, i);
          if (f[i - 1] != 0x15 || varint_get(f, i, vn) != 2ull * (uint64_t)hp.h.def_len) continue;
          std::vector<uint8_t> d = f;
          const uint64_t big = ((1ull << (7 * vn)) - 1) & ~1ull;
          if (!varint_put(&d, i, vn, big)) continue;
          PageHeader h2;
          if (!parse_page_header(d.data() + at0, hp.h.header_len + 8, &h2) || h2.def_len != (int32_t)(big >> 1) || h2.uncompressed_size != hp.h.uncompressed_size ||
              h2.def_len <= h2.uncompressed_size)
            continue;
          report("v2_def_len_above_uncompressed_size", d);
          printf("]}\n");
          return 0;
        }
      }
  report_skipped("v2_def_len_above_uncompressed_size", "no V2 page whose def_len can be raised in place");
  printf("]}\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && !strcmp(argv[1], "dump")) return dump(argv[2]);
  if (argc == 3 && !strcmp(argv[1], "damage")) return damage(argv[2]);
  if (argc == 3 && !strcmp(argv[1], "damage_v2")) return damage_v2(argv[2]);
  fprintf(stderr, "usage: parquet_lz4_check dump FILE | damage FILE | damage_v2 FILE\n");
  return 2;
}
