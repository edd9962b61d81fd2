// dfx_parquet_write.cpp -- the executor of PhysicalPlan::Write { plan, filename, kind } (src/execution/physicalplan.rs:24-29) with
// kind = Parquet (FileType::Parquet, dfparser.rs:31-36), which the reference declares and never runs (deviation D13; the twin of
// dfx_csv_write.cpp, D11).
//
// A sink: it pulls its input to the end.  The schema is judged before a device is asked for.  The row sequence is cut by the shared
// geometry (dfx_parquet_enc.hpp): row groups of exactly row_group_rows rows, pieces (the rows of one batch inside one group), pages of
// page_rows rows.  Every piece is encoded in launch chains of at most pqw::launch_rows rows (dfx_k_parquet_write.hip): measure, scan,
// the read-back of the page table, encode, the copy of the bodies into a pinned buffer -- the two host synchronisations of a launch.
// A column chunk is contiguous in the file, so the pinned buffers of the open row group are held until it closes: at most one row
// group's encoded bytes.  At the close every column's pages go to the file as [header][body], straight from the pinned buffers; the
// host writes headers and the footer (dfx_parquet_thrift_write.hpp) and touches no value.  The bytes go to `filename` +
// ".dfx-partial" and are renamed at the end.
//
// Under "dictionary" = N > 0 every non-Boolean column chunk starts in dictionary mode (dfx_parquet_dict_enc.hpp has the format and the
// per-launch decision, dfx_k_parquet_write_dict.hip the kernels).  The columns of a launch whose chunks are in that mode take a chain of
// their own (encode_dict_columns); the decision is made on the device and comes back with the page table.  A column that falls back in
// a launch is encoded PLAIN by the ordinary chain, in the same call, with the Boolean columns and the columns that fell back earlier:
// that launch pays the ordinary chain's two synchronisations on top -- once in a chunk's life, which for a column that never fits its
// dictionary is once per row group.  The dictionary bodies stay on the
// device until the group closes: one copy and one synchronisation more per row group.  With the option at 0 none of this runs.
//
// Under "compression" = 7 (LZ4_RAW; dfx_parquet_lz4_enc.hpp has the block rule, dfx_k_parquet_write_lz4.hip the kernels) every body is
// packed into one raw LZ4 block before it leaves the device: pack_bodies, called by both chains after their encode kernel and by
// close_group for the dictionary bodies.  Only the blocks are copied into pinned memory: the open row group holds its COMPRESSED
// bytes.  A chain pays one synchronisation more (the table of block sizes, by which the packed buffer is sized); close_group's shares
// the one the dictionary copy has.  With the option at 0 none of this runs.
#include <errno.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>

#include "dfx_parquet_write.hpp"
#include "dfx_relation.hpp"

namespace dfx {

namespace {

using namespace pqw;

struct PqwOptions {
  int64_t row_group_rows = kDefaultRowGroupRows;
  int64_t page_rows = kDefaultPageRows;
  int64_t dictionary = 0;             // N: the most entries of a chunk's dictionary; 0: PLAIN pages only
  int64_t dictionary_hash_bits = 64;  // (debug) the Utf8 hash is cut to this many bits, so that a test can make strings collide
  int64_t compression = kCodecUncompressed;  // the Parquet codec id of every chunk: 0, or 7 (LZ4_RAW)
};

// what the refusal of a codec id calls it (parquet.thrift's CompressionCodec)
const char* other_codec_name(int64_t v) {
  static const char* const names[] = {"UNCOMPRESSED", "SNAPPY", "GZIP", "LZO", "BROTLI", "LZ4", "ZSTD", "LZ4_RAW"};
  return v >= 0 && v < 8 ? names[v] : "such a codec";
}

Status parse_options(const dfx_option* options, int32_t n_options, PqwOptions* o) {
  for (int32_t i = 0; i < n_options; ++i) {
    const char* key = options && options[i].key ? options[i].key : "(null)";
    const int64_t v = options ? options[i].value : 0;
    if (!strcmp(key, "row_group_rows")) {
      if (!row_group_rows_ok(v)) return Status::Err(DFX_GENERAL, strfmt("row_group_rows = %lld: at least 1", (long long)v));
      o->row_group_rows = v;
    } else if (!strcmp(key, "page_rows")) {
      if (!page_rows_ok(v)) return Status::Err(DFX_GENERAL, strfmt("page_rows = %lld: a multiple of 64 from 64 to 2^30", (long long)v));
      o->page_rows = v;
    } else if (!strcmp(key, "dictionary")) {
      if (!dictionary_ok(v)) return Status::Err(DFX_GENERAL, strfmt("dictionary = %lld: 0 (none) or the most entries of a chunk's dictionary, 1 to 2^20", (long long)v));
      o->dictionary = v;
    } else if (!strcmp(key, "dictionary_hash_bits")) {
      if (!dictionary_hash_bits_ok(v)) return Status::Err(DFX_GENERAL, strfmt("dictionary_hash_bits = %lld: 1 to 64", (long long)v));
      o->dictionary_hash_bits = v;
    } else if (!strcmp(key, "compression")) {
      if (!compression_ok(v)) return Status::Err(DFX_GENERAL, strfmt("compression = %lld: 0 (UNCOMPRESSED) or 7 (LZ4_RAW); %s is not written", (long long)v, other_codec_name(v)));
      o->compression = v;
    } else {
      return Status::Err(DFX_GENERAL, std::string("unknown option ") + key);
    }
  }
  // (the dictionary chain keeps a word per row and column of a launch; a page above kLaunchRows rows is a launch of its own, up to 2^30 rows)
  if (o->dictionary > 0 && o->page_rows > kLaunchRows)
    return Status::Err(DFX_GENERAL, strfmt("dictionary = %lld with page_rows = %lld: dictionary encoding takes pages of at most 2^20 rows", (long long)o->dictionary,
                                           (long long)o->page_rows));
  return Status::OK();
}

Status judge_schema(const SchemaInfo& sc) {
  if (sc.fields.empty()) return Status::Err(DFX_GENERAL, "Parquet writer needs a schema with at least one column");
  for (const Field& f : sc.fields)
    if (!dtype_ok(f.dtype)) return Status::Err(DFX_NOT_IMPLEMENTED, strfmt("Parquet writer: column '%s' of type %s", f.name.c_str(), dtype_name(f.dtype)));
  return Status::OK();
}

class ParquetSink {
 public:
  ParquetSink(std::unique_ptr<Relation> in, std::string filename, const PqwOptions& opt)
      : in_(std::move(in)), final_(std::move(filename)), tmp_(final_ + ".dfx-partial"), opt_(opt), writer_(specs(in_->schema()), &ParquetSink::put, this, (int)opt.compression) {}
  ~ParquetSink() {
    if (fp_) fclose(fp_);
    if (fp_ || created_) remove(tmp_.c_str());
  }
  Status run(int64_t* rows, int64_t* bytes);

 private:
  struct HeldPage {
    int64_t num_values, non_null;
    const uint8_t* body;  // in one of held_buffers_
    size_t bytes;
    int encoding;  // ENCODING_PLAIN / ENCODING_RLE_DICTIONARY
    int64_t uncompressed = -1;  // "compression": bytes of the body that `body` is the block of; below 0: `bytes`
  };
  struct PackedBodies {  // what pack_bodies leaves; to be read after the caller's next synchronisation, through check_packed
    std::shared_ptr<void> host;                  // pinned: the blocks, each at its base
    std::shared_ptr<void> table;                 // pinned: PqwLz4Out per body (already read back), then the control word
    std::vector<std::shared_ptr<void>> device;   // what the kernels in flight read and write
    std::vector<PqwLz4In> in;
    const PqwLz4Out* out = nullptr;
    const uint64_t* ctrl = nullptr;
    const uint8_t* block(size_t i) const { return (const uint8_t*)host.get() + out[i].base; }
  };
  struct DictColumn {  // a column's chunk of the open row group under the "dictionary" option
    bool active = false;  // in dictionary mode (never: Boolean columns, the option at 0)
    int64_t launches = 0;  // launches held in dictionary mode: > 0, the chunk gets a dictionary page
    uint64_t entries = 0, body_bytes = 0, body_cap = 0;
    std::shared_ptr<void> slots, entry_off, body;  // device: the table, Utf8 entry offsets, the dictionary page's body
  };
  static std::vector<ColumnSpec> specs(const SchemaInfo& sc) {
    std::vector<ColumnSpec> out;
    for (const Field& f : sc.fields) {
      ColumnSpec c;
      c.name = f.name;
      c.dtype = f.dtype;
      c.nullable = f.nullable;
      out.push_back(c);
    }
    return out;
  }
  static bool put(void* self, const void* p, size_t n) {
    ParquetSink* s = (ParquetSink*)self;
    if (fwrite(p, 1, n, s->fp_) == n) return true;
    s->io_ = Status::Err(DFX_IO_ERROR, strfmt("write to %s failed: %s", s->tmp_.c_str(), strerror(errno)));
    return false;
  }
  Status io_error() const { return io_.ok() ? Status::Err(DFX_IO_ERROR, "write to " + tmp_ + " failed") : io_; }
  Status encode_rows(const DeviceBatch& b, int64_t r0, int64_t n);
  Status encode_columns(const DeviceBatch& b, const int* cols, int nc, int64_t r0, int64_t n);
  Status encode_dict_columns(const DeviceBatch& b, const int* cols, int nc, int64_t r0, int64_t n);
  Status plan_columns(const DeviceBatch& b, const int* cols, int nc, int64_t r0, int64_t n, DevPqwPlan* plan, bool* any_boolean);
  Status pack_bodies(std::vector<PqwLz4In> in, PackedBodies* pk);
  Status check_packed(const PackedBodies& pk);
  bool lz4() const { return opt_.compression == kCodecLz4Raw; }
  Status check_pages(const PqwPage* pt, const DevPqwPlan& plan, int k, int col, int64_t n);
  Status open_group();
  Status close_group();

  std::unique_ptr<Relation> in_;
  std::string final_, tmp_;
  PqwOptions opt_;
  FileWriter writer_;
  FILE* fp_ = nullptr;
  bool created_ = false;
  Status io_;
  int64_t group_rows_ = 0;                          // rows of the open row group
  std::vector<std::vector<HeldPage>> held_;          // ... its encoded pages, column by column
  std::vector<std::shared_ptr<void>> held_buffers_;  // ... the pinned buffers they lie in
  std::vector<DictColumn> dict_;                     // ... its dictionary chunks ("dictionary" > 0)
  std::shared_ptr<void> dict_states_;                // PqwdState per column, on the device
  uint64_t dict_slots_ = 0;                          // slots of a chunk's table
};

// the plan of a launch chain over rows [r0, r0 + n) of the nc columns cols[] of the batch
Status ParquetSink::plan_columns(const DeviceBatch& b, const int* cols, int nc, int64_t r0, int64_t n, DevPqwPlan* plan, bool* any_boolean) {
  const SchemaInfo& sc = in_->schema();
  memset(plan, 0, sizeof(*plan));
  plan->n_cols = nc;
  plan->rows = n;
  plan->page_rows = opt_.page_rows;
  plan->n_tiles = tiles_of(n);
  plan->n_pages = pages_of(n, opt_.page_rows);
  *any_boolean = false;
  for (int k = 0; k < nc; ++k) {
    const DeviceColumn& col = b.columns[(size_t)cols[k]];
    DevPqwCol& d = plan->col[k];
    if (col.absent || col.length < r0 + n || col.dtype != sc.fields[(size_t)cols[k]].dtype)
      return Status::Err(DFX_INTERNAL_ERROR, "Parquet writer: a column of the batch is absent, short or not of the schema's type");
    d.dtype = (uint8_t)col.dtype;
    d.optional = sc.fields[(size_t)cols[k]].nullable ? 1 : 0;
    d.validity = (col.validity && col.null_count != 0) ? col.validity : nullptr;
    d.bit_offset = col.bit_offset + r0;
    if (col.dtype == DFX_UTF8) {
      if (!col.offsets) return Status::Err(DFX_INTERNAL_ERROR, "Parquet writer: Utf8 column without offsets");
      d.offsets = col.offsets + r0;
      d.data = col.data;
    } else if (col.dtype == DFX_BOOLEAN) {
      d.values = col.values;
      *any_boolean = true;
    } else {
      d.values = (const uint8_t*)col.values + (size_t)r0 * (size_t)dtype_width(col.dtype);
    }
  }
  return Status::OK();
}

// what the host refuses of column cols[k]'s pages of a launch: nulls in a REQUIRED column, a page the i32 rule refuses
Status ParquetSink::check_pages(const PqwPage* pt, const DevPqwPlan& plan, int k, int col, int64_t n) {
  const Field& f = in_->schema().fields[(size_t)col];
  for (int64_t p = 0; p < plan.n_pages; ++p) {
    const PqwPage& g = pt[(int64_t)k * plan.n_pages + p];
    const int64_t page_n = std::min<int64_t>(opt_.page_rows, n - p * opt_.page_rows);
    if (!f.nullable && (int64_t)g.non_null != page_n)
      return Status::Err(DFX_EXECUTION_ERROR, strfmt("Parquet writer: column '%s' is not nullable (REQUIRED) and its batch holds %lld nulls in a page of %lld rows",
                                                     f.name.c_str(), (long long)(page_n - (int64_t)g.non_null), (long long)page_n));
    if (g.flags & PQW_PAGE_TOO_LARGE || !body_fits(g.level_bytes, g.val_bytes))
      return Status::Err(DFX_EXECUTION_ERROR, strfmt("Parquet writer: a page of column '%s' takes %llu bytes; a page header holds sizes below 2^31 - 1 (smaller page_rows)",
                                                     f.name.c_str(), (unsigned long long)(g.level_bytes + g.val_bytes)));
  }
  return Status::OK();
}

// "compression" = 7: the bodies in[] (on the device, written by launches already on the stream) packed into raw LZ4 blocks, the blocks
// copied into a pinned buffer sized by their total.  One synchronisation inside (the table of sizes); the copy of the blocks and of the
// control word is left in flight: the caller synchronises and then asks check_packed.
Status ParquetSink::pack_bodies(std::vector<PqwLz4In> in, PackedBodies* pk) {
  hipStream_t s = ctx().stream;
  Status st;
  const size_t n = in.size();
  if (n == 0) return Status::Err(DFX_INTERNAL_ERROR, "Parquet writer: no body to pack");  // (the kernels would leave the table unwritten)
  uint64_t slots_bytes = 0;
  for (PqwLz4In& e : in) {
    if (!lz4_body_fits(e.len))
      return Status::Err(DFX_EXECUTION_ERROR, strfmt("Parquet writer: the LZ4 block of a page of %llu bytes may take 2^31 bytes or more; a page header holds sizes below 2^31 (smaller page_rows)",
                                                     (unsigned long long)e.len));
    e.slot_off = slots_bytes;
    e.pad = 0;
    slots_bytes += (lz4_bound(e.len) + 7ull) & ~7ull;
  }
  const size_t out_bytes = sizeof(PqwLz4Out) * (n + 1) + sizeof(uint64_t);
  auto h_in = pinned_alloc(sizeof(PqwLz4In) * n + 16, &st);
  if (!h_in) return st;
  auto d_in = device_alloc(sizeof(PqwLz4In) * n + 16, &st);
  if (!d_in) return st;
  auto slots = device_alloc((size_t)slots_bytes + 16, &st);
  if (!slots) return st;
  auto d_out = device_alloc(out_bytes, &st);
  if (!d_out) return st;
  pk->table = pinned_alloc(out_bytes, &st);
  if (!pk->table) return st;
  memcpy(h_in.get(), in.data(), sizeof(PqwLz4In) * n);
  PqwLz4Out* d_table = (PqwLz4Out*)d_out.get();
  uint64_t* d_ctrl = (uint64_t*)(d_table + n + 1);
  pk->out = (const PqwLz4Out*)pk->table.get();
  pk->ctrl = (const uint64_t*)(pk->out + n + 1);
  pk->device = {h_in, d_in, slots, d_out};
  DFX_HIP(hipMemsetAsync(d_ctrl, 0, sizeof(uint64_t), s));
  DFX_HIP(hipMemcpyAsync(d_in.get(), h_in.get(), sizeof(PqwLz4In) * n, hipMemcpyHostToDevice, s));
  DFX_HIP(launch_pqw_lz4((const PqwLz4In*)d_in.get(), (int64_t)n, (uint8_t*)slots.get(), slots_bytes, d_table, d_ctrl, s));
  DFX_HIP(hipMemcpyAsync(pk->table.get(), d_table, sizeof(PqwLz4Out) * (n + 1), hipMemcpyDeviceToHost, s));
  DFX_HIP(hipStreamSynchronize(s));  // the table of block sizes: the option's one synchronisation more
  const uint64_t total = pk->out[n].base;
  for (size_t i = 0; i < n; ++i)
    if ((uint64_t)pk->out[i].bytes > lz4_bound(in[i].len) || pk->out[i].base > total || (uint64_t)pk->out[i].bytes > total - pk->out[i].base)
      return Status::Err(DFX_INTERNAL_ERROR, "Parquet writer: an LZ4 block is larger than its bound or lies outside the packed buffer");
  auto packed = device_alloc((size_t)total + 16, &st);
  if (!packed) return st;
  pk->host = pinned_alloc((size_t)total + 16, &st);
  if (!pk->host) return st;
  pk->device.push_back(packed);
  DFX_HIP(launch_pqw_lz4_compact((const PqwLz4In*)d_in.get(), d_table, (int64_t)n, (const uint8_t*)slots.get(), slots_bytes, (uint8_t*)packed.get(), total, d_ctrl, s));
  DFX_HIP(hipMemcpyAsync((void*)pk->ctrl, d_ctrl, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  if (total) DFX_HIP(hipMemcpyAsync(pk->host.get(), packed.get(), (size_t)total, hipMemcpyDeviceToHost, s));
  pk->in = std::move(in);
  return Status::OK();
}

// after the synchronisation that follows pack_bodies: the guard's verdict, and the counters
Status ParquetSink::check_packed(const PackedBodies& pk) {
  if (*pk.ctrl != 0) return Status::Err(DFX_INTERNAL_ERROR, "Parquet writer: an LZ4 sequence would leave its block's slot, or a block its buffer");
  for (size_t i = 0; i < pk.in.size(); ++i) {
    ++counters().parquet_write_lz4_pages;
    counters().parquet_write_lz4_bytes_in += (long long)pk.in[i].len;
    counters().parquet_write_lz4_bytes_out += (long long)pk.out[i].bytes;
    counters().parquet_write_lz4_sequences += (long long)pk.out[i].sequences;
  }
  return Status::OK();
}

// one launch chain of PLAIN pages over rows [r0, r0 + n) of the nc columns cols[] of the batch
Status ParquetSink::encode_columns(const DeviceBatch& b, const int* cols, int nc, int64_t r0, int64_t n) {
  hipStream_t s = ctx().stream;
  Status st;
  DevPqwPlan plan;
  bool any_boolean = false;
  DFX_RETURN_IF_ERROR(plan_columns(b, cols, nc, r0, n, &plan, &any_boolean));
  const int64_t n_tiles = plan.n_tiles * nc, n_pages = plan.n_pages * nc;
  auto tiles = device_alloc(sizeof(PqwTile) * (size_t)n_tiles, &st);
  if (!tiles) return st;
  auto pages = device_alloc(sizeof(PqwPage) * (size_t)(n_pages + 1) + sizeof(uint64_t), &st);
  if (!pages) return st;
  auto table = pinned_alloc(sizeof(PqwPage) * (size_t)(n_pages + 1) + sizeof(uint64_t), &st);  // the page table, then the control word
  if (!table) return st;
  PqwPage* d_pages = (PqwPage*)pages.get();
  uint64_t* ctrl = (uint64_t*)(d_pages + n_pages + 1);
  DFX_HIP(hipMemsetAsync(ctrl, 0, sizeof(uint64_t), s));
  DFX_HIP(launch_pqw_measure(plan, (PqwTile*)tiles.get(), s));
  DFX_HIP(launch_pqw_scan(plan, (PqwTile*)tiles.get(), d_pages, s));
  DFX_HIP(hipMemcpyAsync(table.get(), d_pages, sizeof(PqwPage) * (size_t)(n_pages + 1), hipMemcpyDeviceToHost, s));
  DFX_HIP(hipStreamSynchronize(s));  // the page table: the one read-back of the launch
  const PqwPage* pt = (const PqwPage*)table.get();
  for (int k = 0; k < nc; ++k) DFX_RETURN_IF_ERROR(check_pages(pt, plan, k, cols[k], n));
  const uint64_t total = pt[n_pages].base;
  auto out = device_alloc((size_t)total + 16, &st);
  if (!out) return st;
  std::shared_ptr<void> host;
  if (!lz4()) {
    host = pinned_alloc((size_t)total + 16, &st);
    if (!host) return st;
  }
  if (any_boolean) DFX_HIP(hipMemsetAsync(out.get(), 0, (size_t)total + 16, s));  // Boolean pages are ORed into zeroes
  DFX_HIP(launch_pqw_encode(plan, (const PqwTile*)tiles.get(), d_pages, (uint8_t*)out.get(), total, ctrl, s));
  const uint64_t* hc = (const uint64_t*)((const PqwPage*)table.get() + n_pages + 1);
  DFX_HIP(hipMemcpyAsync((void*)hc, ctrl, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  PackedBodies pk;
  if (lz4()) {
    std::vector<PqwLz4In> in;
    for (int64_t i = 0; i < n_pages; ++i) {
      const uint64_t body = (uint64_t)pt[i].level_bytes + pt[i].val_bytes;
      if (pt[i].base > total || body > total - pt[i].base) return Status::Err(DFX_INTERNAL_ERROR, "Parquet writer: a page lies outside its launch's buffer");
      in.push_back(PqwLz4In{(const uint8_t*)out.get() + pt[i].base, 0, (uint32_t)body, 0});
    }
    DFX_RETURN_IF_ERROR(pack_bodies(std::move(in), &pk));
    host = pk.host;
  } else if (total) {
    DFX_HIP(hipMemcpyAsync(host.get(), out.get(), (size_t)total, hipMemcpyDeviceToHost, s));
  }
  DFX_HIP(hipStreamSynchronize(s));  // the bodies
  if (*hc != 0) return Status::Err(DFX_INTERNAL_ERROR, "Parquet writer: the measure and encode kernels disagree about a tile, or a tile would leave its page");
  if (lz4()) DFX_RETURN_IF_ERROR(check_packed(pk));
  held_buffers_.push_back(host);
  for (int k = 0; k < nc; ++k)
    for (int64_t p = 0; p < plan.n_pages; ++p) {
      const PqwPage& g = pt[(int64_t)k * plan.n_pages + p];
      const uint64_t body = (uint64_t)g.level_bytes + g.val_bytes;
      if (g.base > total || body > total - g.base) return Status::Err(DFX_INTERNAL_ERROR, "Parquet writer: a page lies outside its launch's buffer");
      HeldPage h;
      h.num_values = std::min<int64_t>(opt_.page_rows, n - p * opt_.page_rows);
      h.non_null = (int64_t)g.non_null;
      h.body = (const uint8_t*)host.get() + g.base;
      h.bytes = (size_t)body;
      if (lz4()) {
        const size_t i = (size_t)(k * plan.n_pages + p);
        h.body = pk.block(i);
        h.bytes = (size_t)pk.out[i].bytes;
        h.uncompressed = (int64_t)body;
      }
      h.encoding = ENCODING_PLAIN;
      held_[(size_t)cols[k]].push_back(h);
      if (g.kind == LEVELS_MIXED) ++counters().parquet_write_bitpacked_level_pages;
      else if (g.kind != LEVELS_NONE) ++counters().parquet_write_rle_level_pages;
    }
  return Status::OK();
}

// one launch chain over rows [r0, r0 + n) of the nc columns cols[] of the batch, whose chunks are all in dictionary mode: pages of
// dictionary indices for the columns that stay in it; a column that falls back is marked (dict_[col].active) and left to the caller
Status ParquetSink::encode_dict_columns(const DeviceBatch& b, const int* cols, int nc, int64_t r0, int64_t n) {
  hipStream_t s = ctx().stream;
  const size_t n_schema = dict_.size();
  Status st;
  DevPqwdPlan plan;
  bool any_boolean = false;
  DFX_RETURN_IF_ERROR(plan_columns(b, cols, nc, r0, n, &plan.base, &any_boolean));
  memset(plan.dict, 0, sizeof(plan.dict));
  plan.hash_mask = opt_.dictionary_hash_bits >= 64 ? ~0ull : (1ull << opt_.dictionary_hash_bits) - 1ull;
  PqwdState* d_states = (PqwdState*)dict_states_.get();
  for (int k = 0; k < nc; ++k) {
    DictColumn& dc = dict_[(size_t)cols[k]];
    DevPqwdCol& d = plan.dict[k];
    d.slots = (PqwdSlot*)dc.slots.get();
    d.state = d_states + cols[k];
    d.body = (uint8_t*)dc.body.get();
    d.entry_off = (uint32_t*)dc.entry_off.get();
    d.body_cap = dc.body_cap;
    d.mask = (uint32_t)(dict_slots_ - 1);
    d.limit = (uint32_t)opt_.dictionary;
  }
  const int64_t n_tiles = plan.base.n_tiles * nc, n_pages = plan.base.n_pages * nc;
  auto slot_of_row = device_alloc(sizeof(uint32_t) * (size_t)n * (size_t)nc, &st);
  if (!slot_of_row) return st;
  auto tiles = device_alloc(sizeof(PqwdTile) * (size_t)n_tiles, &st);
  if (!tiles) return st;
  const size_t table_bytes = sizeof(PqwPage) * (size_t)(n_pages + 1) + sizeof(uint64_t);
  auto pages = device_alloc(table_bytes, &st);
  if (!pages) return st;
  auto table = pinned_alloc(table_bytes + sizeof(PqwdState) * n_schema, &st);  // the page table, the control word, every column's state
  if (!table) return st;
  PqwPage* d_pages = (PqwPage*)pages.get();
  uint64_t* ctrl = (uint64_t*)(d_pages + n_pages + 1);
  const PqwPage* pt = (const PqwPage*)table.get();
  const uint64_t* hc = (const uint64_t*)(pt + n_pages + 1);
  const PqwdState* states = (const PqwdState*)(hc + 1);
  DFX_HIP(hipMemsetAsync(ctrl, 0, sizeof(uint64_t), s));
  DFX_HIP(launch_pqwd_measure(plan, (uint32_t*)slot_of_row.get(), (PqwdTile*)tiles.get(), d_pages, s));
  DFX_HIP(launch_pqw_bases(d_pages, n_pages, s));
  DFX_HIP(hipMemcpyAsync(table.get(), d_pages, sizeof(PqwPage) * (size_t)(n_pages + 1), hipMemcpyDeviceToHost, s));
  DFX_HIP(hipMemcpyAsync((void*)states, d_states, sizeof(PqwdState) * n_schema, hipMemcpyDeviceToHost, s));
  DFX_HIP(hipStreamSynchronize(s));  // the page table and, with it, every column's mode for this launch
  std::vector<std::shared_ptr<void>> outgrown;  // dictionary bodies being copied from: alive until the launch's second synchronisation
  bool any_stayed = false;
  for (int k = 0; k < nc; ++k) {
    DictColumn& dc = dict_[(size_t)cols[k]];
    const PqwdState& hs = states[cols[k]];
    if (hs.mode != PQWD_MODE_DICT) {  // fell back: PLAIN from this launch to the chunk's end
      dc.active = false;
      ++counters().parquet_write_dict_fallback_chunks;
      continue;
    }
    any_stayed = true;
    if (hs.entries < dc.entries || hs.entries > (uint64_t)opt_.dictionary || hs.body_bytes < dc.body_bytes || !body_fits(0, hs.body_bytes) ||
        hs.entries_before != dc.entries || hs.body_before != dc.body_bytes)
      return Status::Err(DFX_INTERNAL_ERROR, "Parquet writer: a dictionary's state on the device does not follow from the host's");
    DFX_RETURN_IF_ERROR(check_pages(pt, plan.base, k, cols[k], n));
    if (hs.body_bytes > dc.body_cap) {  // the body grows: the entries so far move, on the stream, before commit appends
      const uint64_t cap = std::max<uint64_t>({hs.body_bytes, 2 * dc.body_cap, 4096});
      auto grown = device_alloc((size_t)cap, &st);
      if (!grown) return st;
      if (dc.body_bytes) DFX_HIP(hipMemcpyAsync(grown.get(), dc.body.get(), (size_t)dc.body_bytes, hipMemcpyDeviceToDevice, s));
      outgrown.push_back(dc.body);
      dc.body = grown;
      dc.body_cap = cap;
      plan.dict[k].body = (uint8_t*)grown.get();
      plan.dict[k].body_cap = cap;
    }
    dc.entries = hs.entries;
    dc.body_bytes = hs.body_bytes;
    ++dc.launches;
  }
  if (!any_stayed) return Status::OK();
  const uint64_t total = pt[n_pages].base;
  auto out = device_alloc((size_t)total + 16, &st);
  if (!out) return st;
  std::shared_ptr<void> host;
  if (!lz4()) {
    host = pinned_alloc((size_t)total + 16, &st);
    if (!host) return st;
  }
  DFX_HIP(hipMemsetAsync(out.get(), 0, (size_t)total + 16, s));  // dictionary data pages are ORed into zeroes
  DFX_HIP(launch_pqwd_encode(plan, (const uint32_t*)slot_of_row.get(), (const PqwdTile*)tiles.get(), d_pages, (uint8_t*)out.get(), total, ctrl, s));
  DFX_HIP(hipMemcpyAsync((void*)hc, ctrl, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  PackedBodies pk;
  std::vector<int64_t> block_of((size_t)n_pages, -1);  // a page's entry in pk: the pages of the columns that stayed
  if (lz4()) {
    std::vector<PqwLz4In> in;
    for (int64_t i = 0; i < n_pages; ++i) {
      if (states[cols[i / plan.base.n_pages]].mode != PQWD_MODE_DICT) continue;
      const uint64_t body = (uint64_t)pt[i].level_bytes + pt[i].val_bytes;
      if (pt[i].base > total || body > total - pt[i].base) return Status::Err(DFX_INTERNAL_ERROR, "Parquet writer: a page lies outside its launch's buffer");
      block_of[(size_t)i] = (int64_t)in.size();
      in.push_back(PqwLz4In{(const uint8_t*)out.get() + pt[i].base, 0, (uint32_t)body, 0});
    }
    DFX_RETURN_IF_ERROR(pack_bodies(std::move(in), &pk));
    host = pk.host;
  } else if (total) {
    DFX_HIP(hipMemcpyAsync(host.get(), out.get(), (size_t)total, hipMemcpyDeviceToHost, s));
  }
  DFX_HIP(hipStreamSynchronize(s));  // the bodies
  if (*hc != 0) return Status::Err(DFX_INTERNAL_ERROR, "Parquet writer: the dictionary kernels disagree about a tile, or a tile would leave its page or its dictionary");
  if (lz4()) DFX_RETURN_IF_ERROR(check_packed(pk));
  held_buffers_.push_back(host);
  for (int k = 0; k < nc; ++k) {
    if (states[cols[k]].mode != PQWD_MODE_DICT) continue;
    for (int64_t p = 0; p < plan.base.n_pages; ++p) {
      const PqwPage& g = pt[(int64_t)k * plan.base.n_pages + p];
      const uint64_t body = (uint64_t)g.level_bytes + g.val_bytes;
      if (g.base > total || body > total - g.base) return Status::Err(DFX_INTERNAL_ERROR, "Parquet writer: a page lies outside its launch's buffer");
      HeldPage h;
      h.num_values = std::min<int64_t>(opt_.page_rows, n - p * opt_.page_rows);
      h.non_null = (int64_t)g.non_null;
      h.body = (const uint8_t*)host.get() + g.base;
      h.bytes = (size_t)body;
      if (lz4()) {
        const size_t i = (size_t)block_of[(size_t)(k * plan.base.n_pages + p)];
        h.body = pk.block(i);
        h.bytes = (size_t)pk.out[i].bytes;
        h.uncompressed = (int64_t)body;
      }
      h.encoding = ENCODING_RLE_DICTIONARY;
      held_[(size_t)cols[k]].push_back(h);
      const uint32_t levels = g.kind & ((1u << kPqwdRunShift) - 1u);
      if (levels == LEVELS_MIXED) ++counters().parquet_write_bitpacked_level_pages;
      else if (levels != LEVELS_NONE) ++counters().parquet_write_rle_level_pages;
      ++counters().parquet_write_dict_index_pages;
      if (g.kind >> kPqwdRunShift == DICT_RUN_RLE) ++counters().parquet_write_dict_rle_index_pages;
    }
  }
  return Status::OK();
}

// one launch: the columns in dictionary mode first; then the others -- with those that have just fallen back -- as PLAIN pages
Status ParquetSink::encode_rows(const DeviceBatch& b, int64_t r0, int64_t n) {
  const int n_cols = (int)b.columns.size();
  std::vector<int> cols;
  for (int c = 0; c < n_cols; ++c)
    if (dict_[(size_t)c].active) cols.push_back(c);
  for (size_t c0 = 0; c0 < cols.size(); c0 += kPqwMaxCols) DFX_RETURN_IF_ERROR(encode_dict_columns(b, cols.data() + c0, (int)std::min<size_t>(kPqwMaxCols, cols.size() - c0), r0, n));
  cols.clear();
  for (int c = 0; c < n_cols; ++c)
    if (!dict_[(size_t)c].active) cols.push_back(c);
  for (size_t c0 = 0; c0 < cols.size(); c0 += kPqwMaxCols) DFX_RETURN_IF_ERROR(encode_columns(b, cols.data() + c0, (int)std::min<size_t>(kPqwMaxCols, cols.size() - c0), r0, n));
  return Status::OK();
}

// a row group opens: under "dictionary" every non-Boolean column starts an empty dictionary -- its table {empty, none, unassigned}
Status ParquetSink::open_group() {
  if (opt_.dictionary <= 0) return Status::OK();
  hipStream_t s = ctx().stream;
  const SchemaInfo& sc = in_->schema();
  Status st;
  dict_slots_ = dict_table_slots((uint64_t)opt_.dictionary, (uint64_t)opt_.row_group_rows);
  if (!dict_states_) {
    dict_states_ = device_alloc(sizeof(PqwdState) * dict_.size(), &st);
    if (!dict_states_) return st;
  }
  DFX_HIP(hipMemsetAsync(dict_states_.get(), 0, sizeof(PqwdState) * dict_.size(), s));
  for (size_t c = 0; c < dict_.size(); ++c) {
    DictColumn& dc = dict_[c];
    if (!dictionary_dtype(sc.fields[c].dtype)) continue;
    if (!dc.slots) {
      dc.slots = device_alloc(sizeof(PqwdSlot) * (size_t)(dict_slots_ + 1), &st);  // (+ 1: the slot of the key that equals the empty word)
      if (!dc.slots) return st;
      if (sc.fields[c].dtype == DFX_UTF8) {
        dc.entry_off = device_alloc(sizeof(uint32_t) * (size_t)dict_slots_, &st);
        if (!dc.entry_off) return st;
      }
    }
    DFX_HIP(hipMemsetAsync(dc.slots.get(), 0xFF, sizeof(PqwdSlot) * (size_t)(dict_slots_ + 1), s));
    dc.active = true;
    dc.launches = 0;
    dc.entries = dc.body_bytes = 0;
  }
  return Status::OK();
}

// the open row group goes to the file: per column the dictionary page of a dictionary chunk, then [header][body] of every page,
// offsets recorded by the writer
Status ParquetSink::close_group() {
  hipStream_t s = ctx().stream;
  std::vector<std::shared_ptr<void>> bodies(dict_.size());
  std::vector<int64_t> block_of(dict_.size(), -1);  // "compression": a dictionary body's entry in pk
  std::vector<PqwLz4In> in;
  bool any = false;
  for (size_t c = 0; c < dict_.size(); ++c) {
    const DictColumn& dc = dict_[c];
    if (dc.launches == 0) continue;
    if (lz4()) {  // (a dictionary without an entry is a block as well: a token of no literals)
      block_of[c] = (int64_t)in.size();
      in.push_back(PqwLz4In{(const uint8_t*)dc.body.get(), 0, (uint32_t)dc.body_bytes, 0});
      continue;
    }
    if (dc.body_bytes == 0) continue;
    Status st;
    bodies[c] = pinned_alloc((size_t)dc.body_bytes, &st);
    if (!bodies[c]) return st;
    DFX_HIP(hipMemcpyAsync(bodies[c].get(), dc.body.get(), (size_t)dc.body_bytes, hipMemcpyDeviceToHost, s));
    any = true;
  }
  PackedBodies pk;
  if (!in.empty()) {  // one launch per group for its dictionary bodies
    DFX_RETURN_IF_ERROR(pack_bodies(std::move(in), &pk));
    any = true;
  }
  if (any) DFX_HIP(hipStreamSynchronize(s));  // the dictionary bodies: once per row group
  if (pk.out) DFX_RETURN_IF_ERROR(check_packed(pk));
  writer_.begin_row_group();
  for (size_t c = 0; c < held_.size(); ++c) {
    writer_.begin_chunk(c);
    if (dict_[c].launches > 0) {
      const bool packed = block_of[c] >= 0;
      if (!(packed ? writer_.add_dictionary_page((int64_t)dict_[c].entries, pk.block((size_t)block_of[c]), (size_t)pk.out[block_of[c]].bytes, (int64_t)dict_[c].body_bytes)
                   : writer_.add_dictionary_page((int64_t)dict_[c].entries, bodies[c].get(), (size_t)dict_[c].body_bytes)))
        return io_error();
      ++counters().parquet_write_dict_pages;
      counters().parquet_write_dict_entries += (long long)dict_[c].entries;
      dict_[c].launches = 0;
    }
    for (const HeldPage& h : held_[c])
      if (!writer_.add_page(h.num_values, h.non_null, h.body, h.bytes, h.encoding, h.uncompressed)) return io_error();
    held_[c].clear();
  }
  writer_.end_row_group(group_rows_);
  held_buffers_.clear();
  group_rows_ = 0;
  return Status::OK();
}

Status ParquetSink::run(int64_t* rows, int64_t* bytes) {
  const size_t n_cols = in_->schema().fields.size();
  fp_ = fopen(tmp_.c_str(), "wb");
  if (!fp_) return Status::Err(DFX_IO_ERROR, strfmt("cannot create %s: %s", tmp_.c_str(), strerror(errno)));
  created_ = true;
  if (!writer_.begin()) return io_error();
  held_.assign(n_cols, std::vector<HeldPage>());
  dict_.assign(n_cols, DictColumn());
  const int64_t per_launch = launch_rows(opt_.page_rows);
  int64_t n_rows = 0;
  for (;;) {
    DeviceBatch b;
    bool has = false;
    DFX_RETURN_IF_ERROR(in_->next(&b, &has));
    if (!has) break;
    if (b.columns.size() != n_cols) return Status::Err(DFX_INTERNAL_ERROR, "Parquet writer: batch and schema disagree");
    for (int64_t r0 = 0; r0 < b.num_rows;) {
      const int64_t piece = piece_rows(group_rows_, b.num_rows - r0, opt_.row_group_rows);
      if (group_rows_ == 0) DFX_RETURN_IF_ERROR(open_group());
      for (int64_t l0 = 0; l0 < piece; l0 += per_launch) DFX_RETURN_IF_ERROR(encode_rows(b, r0 + l0, std::min<int64_t>(per_launch, piece - l0)));
      r0 += piece;
      group_rows_ += piece;
      if (group_rows_ == opt_.row_group_rows) DFX_RETURN_IF_ERROR(close_group());
    }
    n_rows += b.num_rows;
  }
  if (group_rows_ > 0) DFX_RETURN_IF_ERROR(close_group());
  if (!writer_.finish()) return io_error();
  FILE* fp = fp_;
  fp_ = nullptr;
  if (fclose(fp) != 0) return Status::Err(DFX_IO_ERROR, strfmt("closing %s failed: %s", tmp_.c_str(), strerror(errno)));
  if (rename(tmp_.c_str(), final_.c_str()) != 0) return Status::Err(DFX_IO_ERROR, strfmt("cannot rename %s to %s: %s", tmp_.c_str(), final_.c_str(), strerror(errno)));
  created_ = false;
  counters().parquet_write_pages += writer_.pages();
  counters().parquet_write_row_groups += writer_.row_groups();
  counters().parquet_write_bytes += (long long)writer_.bytes();
  if (rows) *rows = n_rows;
  if (bytes) *bytes = (int64_t)writer_.bytes();
  return Status::OK();
}

}  // namespace

}  // namespace dfx

using namespace dfx;

extern "C" {

int32_t dfx_parquet_write(struct ArrowArrayStream* input, const char* filename, const dfx_option* options, int32_t n_options,
                          int64_t* rows_out, int64_t* bytes_out, char* err, size_t errlen) {
  return c_abi_guard(err, errlen, [&]() -> int32_t {
    if (!input || !filename) return to_c(Status::Err(DFX_GENERAL, "null argument"), err, errlen);
    PqwOptions opt;
    Status st = parse_options(options, n_options, &opt);
    if (!st.ok()) return to_c(st, err, errlen);
    std::unique_ptr<Relation> in;
    st = adopt_input_stream(input, &in);  // (needs no device; a column type the library does not know is refused here, by name)
    if (!st.ok()) return to_c(st, err, errlen);
    st = judge_schema(in->schema());
    if (!st.ok()) return to_c(st, err, errlen);
    st = ensure_init();  // no device: nothing is created, there is no host encoding path
    if (!st.ok()) return to_c(st, err, errlen);
    ParquetSink sink(std::move(in), filename, opt);
    st = sink.run(rows_out, bytes_out);
    if (!st.ok()) {
      (void)hipStreamSynchronize(ctx().stream);  // nothing of this call is in flight when its buffers go
      return to_c(st, err, errlen);
    }
    return DFX_OK;
  });
}

}  // extern "C"
