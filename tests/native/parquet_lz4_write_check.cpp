// parquet_lz4_write_check.cpp -- the "compression" option of the Parquet writer on the CPU: csrc/dfx_parquet_lz4_enc.hpp (the block rule
// and its sequential encoder) with the additions to csrc/dfx_parquet_thrift_write.hpp and csrc/dfx_parquet_enc.hpp, as a stand-alone
// program (tests/test_parquet_lz4_write_host.py builds it plain and under the host sanitizers; tests/test_gpu_parquet_lz4_write.py takes
// the expected bytes of every file, and the sequence counts, from it).  The description format, its parser, the exact-size heap copies
// and the comparison with the source are parquet_write_check.cpp's, included as they are.
//   write DESC OUT N   the columns described in DESC as a whole file under compression = 7 and dictionary = N (0: none), launch by
//                      launch as dfx_parquet_write.cpp cuts them, every body one block of lz4_encode_block; then OUT taken back the
//                      way the device takes a compressed chunk -- csrc/dfx_parquet_meta.hpp's walk_headers -> inflate_page -> body
//                      pass -> decode_chunk -- and compared with the source; per chunk the footer's sizes and per page both header
//                      sizes and the block's sequences, as JSON
//   block IN OUT       the bytes of IN as one block into OUT: decoded again by lz4_decode_block and compared, walked with
//                      lz4_next_sequence for the end-of-block rules; sizes, statistics and (up to 64 of) the sequences as JSON
//   candidate          lz4_candidate_ok at the distances 65535 and 65536, at ref == p and on an empty entry: four 0 / 1
//   fits N ...         per made-up body size: [lz4_bound, 1: the i32 rule takes the body]
// Every input and every block is an exact-size heap copy, so a read or a store past an end is the sanitizer's to see.
#define main parquet_write_check_main
#include "parquet_write_check.cpp"
#undef main

#include "../../datafusion_archive_amd/csrc/dfx_parquet_dict_enc.hpp"
#include "../../datafusion_archive_amd/csrc/dfx_parquet_lz4_enc.hpp"

struct HeldPage {
  int64_t num_values = 0, non_null = 0;
  int encoding = pqw::ENCODING_PLAIN;
  std::vector<uint8_t> body;  // exactly the body
};

// `body` as one block: read from an exact-size copy, encoded into lz4_bound bytes, kept as an exact-size copy
static void compress(const uint8_t* body, size_t n, Heap* block, pqw::Lz4EncStats* stats) {
  Heap in, room;
  in.take(body, n);
  room.p = (uint8_t*)malloc((size_t)pqw::lz4_bound(n));
  room.n = (size_t)pqw::lz4_bound(n);
  const uint64_t len = pqw::lz4_encode_block(in.p, n, room.p, stats);
  if (len > room.n) abort();
  block->take(room.p, (size_t)len);
}

static int write_lz4_file(const Desc& d, const char* out_path, uint64_t limit, pqw::Lz4EncStats* stats, std::string* error) {
  for (const pqw::ColumnSpec& s : d.cols)
    if (!pqw::dtype_ok(s.dtype)) return *error = "column '" + s.name + "' of an unsupported type", DFX_NOT_IMPLEMENTED;
  if (!pqw::page_rows_ok((int64_t)d.page_rows) || !pqw::row_group_rows_ok((int64_t)d.row_group_rows) || !pqw::dictionary_ok((int64_t)limit) ||
      (limit > 0 && (int64_t)d.page_rows > pqw::kLaunchRows))  // (as dfx_parquet_write refuses them)
    return *error = "bad options", DFX_GENERAL;
  FILE* fp = fopen(out_path, "wb");
  if (!fp) return *error = "cannot create the file", DFX_IO_ERROR;
  pqw::FileWriter w(d.cols, put_file, fp, pqw::kCodecLz4Raw);
  std::vector<std::vector<HeldPage>> held(d.cols.size());
  std::vector<pqw::DictChunk> chunks(d.cols.size());
  int64_t group_rows = 0;
  int code = DFX_OK;
  bool ok = w.begin();
  auto close_group = [&]() {
    w.begin_row_group();
    for (size_t c = 0; c < held.size(); ++c) {
      w.begin_chunk(c);
      if (chunks[c].launches > 0) {
        Heap block;
        compress(chunks[c].body.data(), chunks[c].body.size(), &block, stats);
        ok = ok && w.add_dictionary_page((int64_t)chunks[c].entries, block.p, block.n, (int64_t)chunks[c].body.size());
      }
      for (const HeldPage& p : held[c]) {
        Heap block;
        compress(p.body.data(), p.body.size(), &block, stats);
        ok = ok && w.add_page(p.num_values, p.non_null, block.p, block.n, p.encoding, (int64_t)p.body.size());
      }
      held[c].clear();
      chunks[c] = pqw::DictChunk();
    }
    w.end_row_group(group_rows);
    group_rows = 0;
  };
  const int64_t per_launch = pqw::launch_rows((int64_t)d.page_rows);
  for (const Batch& b : d.batches) {
    for (int64_t r0 = 0; r0 < (int64_t)b.rows && code == DFX_OK;) {
      const int64_t piece = pqw::piece_rows(group_rows, (int64_t)b.rows - r0, (int64_t)d.row_group_rows);
      for (size_t c = 0; c < d.cols.size() && code == DFX_OK; ++c) {
        const pqw::SourceColumn src = source_of(d.cols[c], b.cols[c]);
        for (int64_t l0 = 0; l0 < piece && code == DFX_OK; l0 += per_launch) {
          const int64_t ln = std::min<int64_t>(per_launch, piece - l0);
          int stayed = 0;
          if (limit > 0 && pqw::dictionary_dtype(d.cols[c].dtype) && !chunks[c].plain) {
            std::vector<pqw::DictPage> pages;
            stayed = pqw::dict_encode_launch(src, r0 + l0, ln, (int64_t)d.page_rows, limit, &chunks[c], &pages);
            for (pqw::DictPage& pg : pages) {
              held[c].emplace_back();
              held[c].back().num_values = pg.info.num_values;
              held[c].back().non_null = pg.info.non_null;
              held[c].back().encoding = pqw::ENCODING_RLE_DICTIONARY;
              held[c].back().body.swap(pg.body);
              if (!d.cols[c].nullable && pg.info.non_null != pg.info.num_values) stayed = -2;
              if (!pqw::lz4_body_fits(held[c].back().body.size())) stayed = -1;
            }
          }
          for (int64_t p0 = 0; stayed == 0 && p0 < ln; p0 += (int64_t)d.page_rows) {
            const int64_t n = std::min<int64_t>((int64_t)d.page_rows, ln - p0);
            held[c].emplace_back();
            pqw::EncodedPage info;
            if (!pqw::encode_page(src, r0 + l0 + p0, n, &held[c].back().body, &info) || !pqw::lz4_body_fits(held[c].back().body.size())) stayed = -1;
            else if (!d.cols[c].nullable && info.non_null != n) stayed = -2;
            held[c].back().num_values = n;
            held[c].back().non_null = info.non_null;
          }
          if (stayed < 0) {
            *error = stayed == -1 ? "a page of column '" + d.cols[c].name + "' is refused by the i32 size rule" : "column '" + d.cols[c].name + "' is REQUIRED and holds nulls";
            code = DFX_EXECUTION_ERROR;
          }
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

// ---- the way back: header pass -> every page inflated into the image -> prologues -> body pass -> decode_chunk over the image ---------
struct Lz4Chunk {
  pq::ChunkHeaders headers;
  std::vector<uint64_t> sequences;  // per page of headers.pages
};
struct Lz4Parsed {
  Parsed p;
  std::vector<std::vector<Lz4Chunk>> rgs;
  Lz4Stats lz4;
};
static pq::Err parse_lz4_file(const uint8_t* f, size_t n, Lz4Parsed* out) {
  Parsed& P = out->p;
  if (n < 12) return pq::parser_error("a file of " + pq::num((long long)n) + " bytes is too short");
  if (memcmp(f, "PAR1", 4) != 0) return pq::parser_error("the file does not start with the magic PAR1");
  uint32_t flen = 0;
  pq::Err e = pq::check_tail(f + n - 8, n, &flen);
  if (!e.ok()) return e;
  e = pq::parse_file_meta(f + n - 8 - flen, flen, &P.meta);
  if (!e.ok()) return e;
  e = pq::resolve(P.meta, n, flen, &P.cols);
  if (!e.ok()) return e;
  for (size_t g = 0; g < P.meta.row_groups.size(); ++g) {
    const pq::RowGroupMeta& rg = P.meta.row_groups[g];
    P.rgs.emplace_back(rg.columns.size());
    out->rgs.emplace_back(rg.columns.size());
    for (size_t c = 0; c < rg.columns.size(); ++c) {
      Chunk& k = P.rgs.back()[c];
      Lz4Chunk& z = out->rgs.back()[c];
      k.meta = rg.columns[c];
      const std::string where = "column '" + P.cols[c].name + "', row group " + pq::num((long long)g);
      const uint8_t* chunk = f + k.meta.start();
      e = pq::walk_headers(chunk, (size_t)k.meta.total_compressed_size, k.meta.codec, P.cols[c], where, &z.headers);
      if (!e.ok()) return e;
      Heap image;
      image.n = (size_t)z.headers.image_len;
      image.p = (uint8_t*)calloc(image.n ? image.n : 1, 1);
      std::vector<PqPrologue> prologues;
      for (const pq::HeaderPage& hp : z.headers.pages) {
        Heap body;  // the block alone, in a heap block of its own size
        body.take(chunk + hp.ip.src_off, hp.ip.src_len);
        PqInflatePage ip = hp.ip;
        ip.src_off = 0;
        Lz4Stats one;
        if (!pq::inflate_page(body.p, ip, image.p, &one)) return pq::parser_error(pq::page_where(where, hp.page_no, hp.pos) + ": the compressed block is malformed");
        z.sequences.push_back(one.sequences);
        out->lz4.sequences += one.sequences;
        out->lz4.lit_extensions += one.lit_extensions;
        out->lz4.match_extensions += one.match_extensions;
        prologues.push_back(pq::page_prologue(image.p, hp.ip));
      }
      e = pq::walk_bodies(z.headers, image.p, prologues.data(), P.cols[c], rg.num_rows, where, &k.walked);
      if (e.ok()) e = pq::decode_chunk(image.p, P.cols[c], k.walked, rg.num_rows, where, &k.decoded);
      if (!e.ok()) return e;
    }
  }
  return pq::Err();
}

static int cmd_write_lz4(const char* desc_path, const char* out_path, const char* limit_text) {
  std::vector<uint8_t> raw;
  Desc d;
  if (!read_file(desc_path, &raw) || !parse_desc(raw, &d)) {
    fprintf(stderr, "cannot read the description\n");
    return 2;
  }
  std::string error;
  pqw::Lz4EncStats stats;
  const int code = write_lz4_file(d, out_path, strtoull(limit_text, nullptr, 10), &stats, &error);
  if (code != DFX_OK) {
    printf("{\"code\": %d, \"error\": ", code);
    put_str(error);
    printf("}\n");
    return 0;
  }
  std::vector<uint8_t> f;
  if (!read_file(out_path, &f)) return 2;
  Lz4Parsed z;
  Heap copy;
  copy.take(f.data(), f.size());
  const pq::Err e = parse_lz4_file(copy.p, copy.n, &z);
  if (!e.ok()) {
    printf("{\"code\": 0, \"bytes\": %zu, \"reader_code\": %d, \"reader_error\": ", f.size(), e.code);
    put_str(e.msg);
    printf("}\n");
    return 0;
  }
  printf("{\"code\": 0, \"bytes\": %zu, \"reader_code\": 0, \"num_rows\": %lld, \"mismatch\": ", f.size(), (long long)z.p.meta.num_rows);
  put_str(compare(d, z.p));
  printf(", \"encoder\": {\"sequences\": %llu, \"lit_extensions\": %llu, \"match_extensions\": %llu, \"steps_without_pick\": %llu}",
         (unsigned long long)stats.sequences, (unsigned long long)stats.lit_extensions, (unsigned long long)stats.match_extensions,
         (unsigned long long)stats.steps_without_pick);
  printf(", \"decoder\": {\"sequences\": %llu, \"lit_extensions\": %llu, \"match_extensions\": %llu}", (unsigned long long)z.lz4.sequences,
         (unsigned long long)z.lz4.lit_extensions, (unsigned long long)z.lz4.match_extensions);
  printf(", \"row_groups\": [");
  for (size_t g = 0; g < z.rgs.size(); ++g) {
    printf("%s{\"num_rows\": %lld, \"chunks\": [", g ? ", " : "", (long long)z.p.meta.row_groups[g].num_rows);
    for (size_t c = 0; c < z.rgs[g].size(); ++c) {
      const Chunk& k = z.p.rgs[g][c];
      const Lz4Chunk& zc = z.rgs[g][c];
      printf("%s{\"codec_id\": %d, \"total_compressed_size\": %lld, \"total_uncompressed_size\": %lld, \"has_dict\": %s, \"oversized_v1_pages\": %lld, \"pages\": [",
             c ? ", " : "", k.meta.codec, (long long)k.meta.total_compressed_size, (long long)k.meta.total_uncompressed_size, k.walked.has_dict ? "true" : "false",
             zc.headers.oversized_v1_pages);
      for (size_t i = 0; i < zc.headers.pages.size(); ++i) {
        const pq::HeaderPage& hp = zc.headers.pages[i];
        printf("%s{\"type\": %d, \"header_len\": %zu, \"compressed\": %u, \"uncompressed\": %u, \"sequences\": %llu}", i ? ", " : "", hp.h.type, (size_t)hp.h.header_len,
               hp.ip.src_len, hp.ip.dst_len, (unsigned long long)zc.sequences[i]);
      }
      printf("]}");
    }
    printf("]}");
  }
  printf("]}\n");
  return 0;
}

static int cmd_block(const char* in_path, const char* out_path) {
  std::vector<uint8_t> raw;
  if (!read_file(in_path, &raw)) return 2;
  const uint64_t n = raw.size();
  pqw::Lz4EncStats stats;
  Heap block;
  compress(raw.data(), raw.size(), &block, &stats);
  FILE* fp = fopen(out_path, "wb");
  if (!fp || fwrite(block.p, 1, block.n, fp) != block.n || fclose(fp) != 0) return 2;
  // back through the reader's decoder, into an exact-size image
  Heap image;
  image.n = (size_t)n;
  image.p = (uint8_t*)calloc(n ? n : 1, 1);
  Lz4Stats dec;
  const bool decodes = lz4_decode_block(block.p, block.n, image.p, n, &dec);
  const bool equal = decodes && (n == 0 || memcmp(image.p, raw.data(), (size_t)n) == 0);
  // the sequences themselves: where the last match starts and ends, the longest offset
  uint64_t pos = 0, outp = 0, last_match_start = 0, last_match_end = 0, max_offset = 0, matches = 0, count = 0;
  bool walked = true;
  std::vector<Lz4Seq> seqs;
  for (;;) {
    Lz4Seq q;
    if (!lz4_next_sequence(block.p, block.n, pos, outp, n, &q)) {
      walked = false;
      break;
    }
    ++count;
    if (seqs.size() < 64) seqs.push_back(q);
    outp += q.lit_len;
    if (q.last) break;
    last_match_start = outp;
    outp += q.match_len;
    last_match_end = outp;
    max_offset = std::max<uint64_t>(max_offset, q.offset);
    ++matches;
    pos = q.next;
  }
  printf("{\"n\": %llu, \"bytes\": %zu, \"bound\": %llu, \"decodes\": %s, \"equal\": %s, \"walked\": %s, \"sequences\": %llu, \"walked_sequences\": %llu, "
         "\"lit_extensions\": %llu, \"match_extensions\": %llu, \"steps_without_pick\": %llu, \"decoder_sequences\": %llu, \"matches\": %llu, "
         "\"last_match_start\": %llu, \"last_match_end\": %llu, \"max_offset\": %llu, \"seqs\": [",
         (unsigned long long)n, block.n, (unsigned long long)pqw::lz4_bound(n), decodes ? "true" : "false", equal ? "true" : "false", walked ? "true" : "false",
         (unsigned long long)stats.sequences, (unsigned long long)count, (unsigned long long)stats.lit_extensions, (unsigned long long)stats.match_extensions,
         (unsigned long long)stats.steps_without_pick, (unsigned long long)dec.sequences, (unsigned long long)matches, (unsigned long long)last_match_start,
         (unsigned long long)last_match_end, (unsigned long long)max_offset);
  for (size_t i = 0; i < seqs.size(); ++i) printf("%s[%u, %u, %u]", i ? ", " : "", seqs[i].lit_len, seqs[i].offset, seqs[i].match_len);
  printf("]}\n");
  return 0;
}

static int cmd_candidate() {
  // equal words at 0, 1 and 65536 of an exact-size buffer: 65536 - 1 = 65535 back holds, 65536 - 0 does not
  Heap buf;
  buf.n = 65536 + 4;
  buf.p = (uint8_t*)calloc(buf.n, 1);
  for (size_t i = 0; i < buf.n; ++i) buf.p[i] = (uint8_t)(i * 7 + 1);
  const uint8_t word[5] = {0xA1, 0xA1, 0xA1, 0xA1, 0xA1};
  memcpy(buf.p, word, 5);  // the words at 0 and at 1
  memcpy(buf.p + 65536, word, 4);
  printf("[%d, %d, %d, %d]\n", pqw::lz4_candidate_ok(65536, 1 + 1, buf.p) ? 1 : 0, pqw::lz4_candidate_ok(65536, 0 + 1, buf.p) ? 1 : 0,
         pqw::lz4_candidate_ok(65536, 65536 + 1, buf.p) ? 1 : 0, pqw::lz4_candidate_ok(65536, 0, buf.p) ? 1 : 0);
  return 0;
}

static int cmd_fits_lz4(int argc, char** argv) {
  printf("[");
  for (int i = 2; i < argc; ++i) {
    const uint64_t n = strtoull(argv[i], nullptr, 10);
    printf("%s[%llu, %d]", i > 2 ? ", " : "", (unsigned long long)pqw::lz4_bound(n), pqw::lz4_body_fits(n) ? 1 : 0);
  }
  printf("]\n");
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 5 && !strcmp(argv[1], "write")) return cmd_write_lz4(argv[2], argv[3], argv[4]);
  if (argc == 4 && !strcmp(argv[1], "block")) return cmd_block(argv[2], argv[3]);
  if (argc == 2 && !strcmp(argv[1], "candidate")) return cmd_candidate();
  if (argc >= 3 && !strcmp(argv[1], "fits")) return cmd_fits_lz4(argc, argv);
  fprintf(stderr, "usage: parquet_lz4_write_check write DESC|- OUT N | block IN OUT | candidate | fits N ...\n");
  return 2;
}
