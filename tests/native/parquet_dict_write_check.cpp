// parquet_dict_write_check.cpp -- the "dictionary" option of the Parquet writer on the CPU: csrc/dfx_parquet_dict_enc.hpp (the rules and the
// sequential encoder of a dictionary chunk) on top of what parquet_write_check.cpp exercises, as a stand-alone program
// (tests/test_parquet_dict_write_host.py builds it plain and under the host sanitizers; tests/test_gpu_parquet_dict_write.py takes the
// expected bytes of every file from it).  The description format, its parser, the exact-size heap copies, the way back through the
// READER's headers and the comparison with the source are parquet_write_check.cpp's, included as they are.
//   write DESC OUT N   the columns described in DESC as a whole file under dictionary = N (0: none), launch by launch as
//                      dfx_parquet_write.cpp cuts them; then OUT parsed and decoded by csrc/dfx_parquet_meta.hpp (every index page
//                      through csrc/dfx_parquet_rle.hpp) and compared with the source; per chunk the dictionary and per page the
//                      encoding, the index width and the run kind read from the page's bytes, as JSON
//   width E ...        the index width at E entries
//   run W NN EQ ...    per triple {width, non-null values, 1: all indices equal}: [run kind, header, run bytes, value block bytes]
//   stays E e B b N ...  the decision of a launch per quintuple: 0 / 1
//   damage FILE        FILE truncated at every length, and every byte of its first page header -- a dictionary page's -- set to 0x00,
//                      0x7f, 0xff one at a time: a truncation must be an error, a byte change an error or a file that still parses
#define main parquet_write_check_main
#include "parquet_write_check.cpp"
#undef main

#include "../../datafusion_archive_amd/csrc/dfx_parquet_dict_enc.hpp"

struct HeldPage {
  int64_t num_values = 0, non_null = 0;
  int encoding = pqw::ENCODING_PLAIN;
  std::vector<uint8_t> body;  // exactly the body
};

static int write_dict_file(const Desc& d, const char* out_path, uint64_t limit, std::string* error) {
  for (const pqw::ColumnSpec& s : d.cols)
    if (!pqw::dtype_ok(s.dtype)) return *error = "column '" + s.name + "' of an unsupported type", DFX_NOT_IMPLEMENTED;
  if (!pqw::page_rows_ok((int64_t)d.page_rows) || !pqw::row_group_rows_ok((int64_t)d.row_group_rows) || !pqw::dictionary_ok((int64_t)limit) ||
      (limit > 0 && (int64_t)d.page_rows > pqw::kLaunchRows))  // (as dfx_parquet_write refuses them)
    return *error = "bad options", DFX_GENERAL;
  FILE* fp = fopen(out_path, "wb");
  if (!fp) return *error = "cannot create the file", DFX_IO_ERROR;
  pqw::FileWriter w(d.cols, put_file, fp);
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
        Heap body;  // (an exact-size copy: the writer reads no byte past the entries)
        body.take(chunks[c].body.data(), chunks[c].body.size());
        ok = ok && w.add_dictionary_page((int64_t)chunks[c].entries, body.p, body.n);
      }
      for (const HeldPage& p : held[c]) ok = ok && w.add_page(p.num_values, p.non_null, p.body.data(), p.body.size(), p.encoding);
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
            }
          }
          for (int64_t p0 = 0; stayed == 0 && p0 < ln; p0 += (int64_t)d.page_rows) {
            const int64_t n = std::min<int64_t>((int64_t)d.page_rows, ln - p0);
            held[c].emplace_back();
            pqw::EncodedPage info;
            if (!pqw::encode_page(src, r0 + l0 + p0, n, &held[c].back().body, &info)) stayed = -1;
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

static int cmd_write_dict(const char* desc_path, const char* out_path, const char* limit_text) {
  std::vector<uint8_t> raw;
  Desc d;
  if (!read_file(desc_path, &raw) || !parse_desc(raw, &d)) {
    fprintf(stderr, "cannot read the description\n");
    return 2;
  }
  std::string error;
  const int code = write_dict_file(d, out_path, strtoull(limit_text, nullptr, 10), &error);
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
  printf(", \"row_groups\": [");
  for (size_t g = 0; g < p.rgs.size(); ++g) {
    printf("%s{\"num_rows\": %lld, \"chunks\": [", g ? ", " : "", (long long)p.meta.row_groups[g].num_rows);
    for (size_t c = 0; c < p.rgs[g].size(); ++c) {
      const Chunk& k = p.rgs[g][c];
      printf("%s{\"has_dict\": %s, \"dict_n\": %u, \"dict_len\": %u, \"dict_first\": %s, \"walked_strings\": %lld, \"pages\": [", c ? ", " : "",
             k.walked.has_dict ? "true" : "false", k.walked.dict_n, k.walked.dict_len,
             k.meta.has_dictionary_offset && k.meta.dictionary_page_offset < k.meta.data_page_offset ? "true" : "false", k.walked.walked_strings);
      for (size_t i = 0; i < k.walked.pages.size(); ++i) {
        const PqPage& pg = k.walked.pages[i];
        const bool dict = pg.enc == PQ_ENC_DICT;
        // the run kind from the index bytes themselves: the run's header follows the width byte; bit 0 set: bit-packed
        const char* run = !dict ? "plain" : pg.val_len == 0 ? "none" : (f[(size_t)k.meta.start() + pg.val_off] & 1) ? "packed" : "rle";
        printf("%s{\"num_values\": %u, \"run\": \"%s\", \"width\": %u, \"val_len\": %u}", i ? ", " : "", pg.num_values, run, dict ? pg.bit_width : 0u, pg.val_len);
      }
      printf("]}");
    }
    printf("]}");
  }
  printf("]}\n");
  return 0;
}

static int cmd_width(int argc, char** argv) {
  printf("[");
  for (int i = 2; i < argc; ++i) printf("%s%u", i > 2 ? ", " : "", pqw::dict_index_width(strtoull(argv[i], nullptr, 10)));
  printf("]\n");
  return 0;
}

static int cmd_run(int argc, char** argv) {
  printf("[");
  for (int i = 2; i + 2 < argc; i += 3) {
    const uint32_t w = (uint32_t)strtoul(argv[i], nullptr, 10);
    const uint64_t nn = strtoull(argv[i + 1], nullptr, 10);
    const uint32_t run = pqw::dict_run_kind(nn, argv[i + 2][0] == '1');
    printf("%s[%u, %llu, %llu, %llu]", i > 2 ? ", " : "", run, (unsigned long long)pqw::dict_run_header(run, nn), (unsigned long long)pqw::dict_run_bytes(run, w, nn),
           (unsigned long long)pqw::dict_value_bytes(run, w, nn));
  }
  printf("]\n");
  return 0;
}

static int cmd_stays(int argc, char** argv) {
  printf("[");
  for (int i = 2; i + 4 < argc; i += 5) {
    uint64_t v[5];
    for (int k = 0; k < 5; ++k) v[k] = strtoull(argv[i + k], nullptr, 10);
    printf("%s%d", i > 2 ? ", " : "", pqw::dict_stays(v[0], v[1], v[2], v[3], v[4]) ? 1 : 0);
  }
  printf("]\n");
  return 0;
}

static int cmd_damage_dict(const char* path) {
  std::vector<uint8_t> f;
  if (!read_file(path, &f)) return 2;
  pq::PageHeader h;
  {
    Parsed p;
    const pq::Err e = parse_copy(f.data(), f.size(), &p);
    if (!e.ok() || p.rgs.empty() || !p.rgs[0][0].walked.has_dict || p.rgs[0][0].meta.start() != 4 || !pq::parse_page_header(f.data() + 4, f.size() - 4, &h) || h.type != 2) {
      fprintf(stderr, "the undamaged file does not parse, or does not start with a dictionary page: %s\n", e.msg.c_str());
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
  for (size_t pos = 4; pos < 4 + h.header_len; ++pos) {
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
  printf("{\"truncations\": %lld, \"flips\": %lld, \"errors\": %lld, \"header_len\": %zu}\n", truncations, flips, errors, h.header_len);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 5 && !strcmp(argv[1], "write")) return cmd_write_dict(argv[2], argv[3], argv[4]);
  if (argc >= 3 && !strcmp(argv[1], "width")) return cmd_width(argc, argv);
  if (argc >= 5 && !strcmp(argv[1], "run")) return cmd_run(argc, argv);
  if (argc >= 7 && !strcmp(argv[1], "stays")) return cmd_stays(argc, argv);
  if (argc == 3 && !strcmp(argv[1], "damage")) return cmd_damage_dict(argv[2]);
  fprintf(stderr, "usage: parquet_dict_write_check write DESC|- OUT N | width E ... | run W NN EQ ... | stays E e B b N ... | damage FILE\n");
  return 2;
}
