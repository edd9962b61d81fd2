// dfx_parquet.cpp -- the Parquet data source (deviation D12, parity unpinned): DataSourceMeta::ParquetFile { filename, schema,
// projection } (src/execution/datasource.rs:87-92; `STORED AS PARQUET`, dfparser.rs:177-178; LogicalPlan::ParquetFile in the
// push-down rule, sqlplanner.rs:525-532) is declared by the reference and executed nowhere.  The contract here is pyarrow's reader.
//
// open() reads the 8-byte tail and the footer only, builds the schema from the file and rejects what the subset excludes
// (dfx_parquet_meta.hpp: resolve) -- all of it before a device is asked for.  A row group is decoded as a whole at the first next()
// that needs it, so require_columns() has been heard: every NEEDED column chunk is read into a pinned staging buffer and copied to
// HBM; while that copy runs the host walks the chunk's page headers into the page table and the length chains of PLAIN byte arrays
// (walk_chunk), and the kernels of dfx_k_parquet.hip turn the chunk into an Arrow column.  Chunks go one after the other: a chunk's
// control block and counters are read back (one synchronisation) before the next chunk is read from the file.  A column nobody reads is neither read from the file nor copied: it is an `absent`
// placeholder, as CsvRelation leaves unconverted columns.  Batches are zero-copy slices of the decoded row group.
//
// A chunk of codec 7 (LZ4_RAW) is inflated on the device first (inflate_chunk: header pass on the host, k_pq_inflate, the pages'
// prologues read back, body pass on the host -- one synchronisation more per chunk); from the page table on it takes the same path,
// the kernels reading the inflated image instead of the chunk.  An UNCOMPRESSED chunk pays nothing for that.
#include <errno.h>
#include <fcntl.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>

#include "dfx_parquet_meta.hpp"
#include "dfx_relation.hpp"

namespace dfx {

namespace {

Status from_pq(const pq::Err& e) { return e.ok() ? Status::OK() : Status::Err(e.code, e.msg); }

bool pread_all(int fd, void* dst, size_t n, uint64_t off) {
  uint8_t* p = (uint8_t*)dst;
  while (n > 0) {
    const ssize_t got = pread(fd, p, n, (off_t)off);
    if (got < 0 && errno == EINTR) continue;
    if (got <= 0) return false;
    p += got;
    off += (uint64_t)got;
    n -= (size_t)got;
  }
  return true;
}

}  // namespace

class ParquetRelation : public Relation {
 public:
  ParquetRelation(std::string filename, int64_t batch_size) : filename_(std::move(filename)), batch_size_(batch_size) {}
  ~ParquetRelation() override {
    if (fd_ >= 0) close(fd_);
  }
  RelationKind kind() const override { return REL_PARQUET; }
  const SchemaInfo& schema() const override { return schema_; }
  Status next(DeviceBatch* out, bool* has) override;
  void require_columns(const std::vector<char>& needed) override {
    if (!loaded_any_) needed_ = needed;  // (a row group already decoded keeps its columns; the next one hears the new set)
    else pending_needed_ = needed, has_pending_ = true;
  }
  void explain(std::string* out, int depth) const override;
  Status open(const int32_t* projection, int32_t n_projection);

 private:
  bool is_needed(size_t c) const { return needed_.empty() || (c < needed_.size() && needed_[c]); }
  Status load_row_group();
  Status decode_chunk(size_t g, size_t c, DeviceColumn* col);
  Status inflate_chunk(const uint8_t* host, size_t len, const uint8_t* dev_chunk, int32_t codec, const pq::Column& pc, int64_t rows, const std::string& where,
                       std::shared_ptr<void>* image_out, pq::WalkedChunk* w);
  std::string filename_;
  int64_t batch_size_;
  int fd_ = -1;
  uint64_t file_size_ = 0;
  pq::FileMeta meta_;
  std::vector<pq::Column> cols_;  // every leaf of the file
  std::vector<int> proj_;         // stream column -> leaf
  SchemaInfo schema_;
  std::vector<char> needed_, pending_needed_;
  bool has_pending_ = false, loaded_any_ = false;
  size_t rg_ = 0;         // the row group being handed out
  bool rg_loaded_ = false;
  DeviceBatch rg_batch_;  // ... decoded
  int64_t pos_ = 0;       // ... rows handed out
  std::shared_ptr<void> stage_;  // pinned staging, as large as the largest chunk read so far
  size_t stage_bytes_ = 0;
  std::shared_ptr<void> image_stage_;  // pinned: the inflated image of a compressed BYTE_ARRAY chunk, for the length chains
  size_t image_stage_bytes_ = 0;
};

Status ParquetRelation::open(const int32_t* projection, int32_t n_projection) {
  fd_ = ::open(filename_.c_str(), O_RDONLY | O_CLOEXEC);
  if (fd_ < 0) return Status::Err(DFX_IO_ERROR, strfmt("cannot open %s: %s", filename_.c_str(), strerror(errno)));
  struct stat sb;
  if (fstat(fd_, &sb) != 0 || !S_ISREG(sb.st_mode)) return Status::Err(DFX_IO_ERROR, "cannot determine the size of " + filename_);
  file_size_ = (uint64_t)sb.st_size;
  const std::string in = " (" + filename_ + ")";
  if (file_size_ < 12) return Status::Err(DFX_PARSER_ERROR, strfmt("Parquet: a file of %llu bytes is too short", (unsigned long long)file_size_) + in);
  uint8_t head[4], tail[8];
  if (!pread_all(fd_, head, 4, 0) || !pread_all(fd_, tail, 8, file_size_ - 8)) return Status::Err(DFX_IO_ERROR, "cannot read " + filename_);
  if (memcmp(head, "PAR1", 4) != 0) return Status::Err(DFX_PARSER_ERROR, "Parquet: the file does not start with the magic PAR1" + in);
  uint32_t footer_len = 0;
  pq::Err e = pq::check_tail(tail, file_size_, &footer_len);
  if (!e.ok()) return Status::Err(e.code, e.msg + in);
  std::vector<uint8_t> footer(footer_len);
  if (footer_len && !pread_all(fd_, footer.data(), footer_len, file_size_ - 8 - footer_len)) return Status::Err(DFX_IO_ERROR, "cannot read the footer of " + filename_);
  e = pq::parse_file_meta(footer.data(), footer.size(), &meta_);
  if (e.ok()) e = pq::resolve(meta_, file_size_, footer_len, &cols_);
  if (!e.ok()) return Status::Err(e.code, e.msg + in);
  if (projection) {
    for (int32_t i = 0; i < n_projection; ++i) {
      if (projection[i] < 0 || (size_t)projection[i] >= cols_.size())
        return Status::Err(DFX_INVALID_COLUMN, strfmt("Parquet: projection index %d is out of range: %s has %d columns", projection[i], filename_.c_str(), (int)cols_.size()));
      proj_.push_back(projection[i]);
    }
  } else {
    for (size_t i = 0; i < cols_.size(); ++i) proj_.push_back((int)i);
  }
  for (int leaf : proj_) {
    Field f;
    f.name = cols_[leaf].name;
    f.dtype = cols_[leaf].dtype;
    f.nullable = cols_[leaf].optional;
    schema_.fields.push_back(f);
  }
  return ensure_init();  // the file has been judged without a device; decoding has no host path
}

void ParquetRelation::explain(std::string* out, int depth) const {
  size_t n = 0;
  for (size_t c = 0; c < proj_.size(); ++c) n += is_needed(c) ? 1 : 0;
  const size_t rgs = meta_.row_groups.size();
  std::string line = strfmt("ParquetDataSource: %s, %d row groups, %d of %d column chunks read, decoded on the device", filename_.c_str(), (int)rgs,
                            (int)(n * rgs), (int)(cols_.size() * rgs));
  line += batch_size_ > 0 ? strfmt(", batches of %lld rows", (long long)((batch_size_ + 63) / 64 * 64)) : std::string(", one batch per row group");
  // the codecs of the chunks read.  An UNCOMPRESSED chunk costs one host synchronisation; a compressed one two: its pages are
  // inflated on the device and their prologues read back before the host can build the page table (inflate_chunk).
  uint32_t codecs = 0;
  for (size_t c = 0; c < proj_.size(); ++c)
    for (const pq::RowGroupMeta& rg : meta_.row_groups)
      if (is_needed(c) && rg.columns[(size_t)proj_[c]].codec >= 0 && rg.columns[(size_t)proj_[c]].codec < 8) codecs |= 1u << rg.columns[(size_t)proj_[c]].codec;
  if (codecs) line += ", codecs:";
  for (int k = 0; k < 8; ++k)
    if (codecs & (1u << k)) line += std::string(" ") + pq::codec_name(k) + (k ? " (inflated on the device)" : "");
  for (size_t c = 0; c < proj_.size(); ++c) {
    if (!is_needed(c)) continue;
    uint32_t seen = 0;
    for (const pq::RowGroupMeta& rg : meta_.row_groups)
      for (int32_t enc : rg.columns[(size_t)proj_[c]].encodings)
        if (enc >= 0 && enc < 10) seen |= 1u << enc;
    line += "; " + cols_[(size_t)proj_[c]].name + ":";
    for (int enc = 0; enc < 10; ++enc)
      if (seen & (1u << enc)) line += std::string(" ") + pq::encoding_name(enc);
  }
  explain_line(out, depth, line);
}

Status ParquetRelation::decode_chunk(size_t g, size_t c, DeviceColumn* col) {
  const pq::Column& pc = cols_[(size_t)proj_[c]];
  const pq::RowGroupMeta& rg = meta_.row_groups[g];
  const pq::ChunkMeta& km = rg.columns[(size_t)proj_[c]];
  const size_t len = (size_t)km.total_compressed_size;
  const int64_t rows = rg.num_rows;
  hipStream_t s = ctx().stream;
  Status st;
  // ---- file -> pinned staging -> HBM (the stream is idle here: every path out of this function synchronises it)
  if (stage_bytes_ < len || !stage_) {
    stage_.reset();
    stage_ = pinned_alloc(std::max<size_t>(len, 64), &st);
    if (!stage_) return st;
    stage_bytes_ = std::max<size_t>(len, 64);
  }
  uint8_t* host = (uint8_t*)stage_.get();
  if (!pread_all(fd_, host, len, (uint64_t)km.start())) return Status::Err(DFX_IO_ERROR, "short read from " + filename_);
  auto chunk = device_alloc(len + 64, &st);
  if (!chunk) return st;
  DFX_HIP(hipMemcpyAsync(chunk.get(), host, len, hipMemcpyHostToDevice, s));
  counters().parquet_chunk_bytes += (long long)len;
  // ---- the page headers and the length chains, while the copy runs
  pq::WalkedChunk w;
  struct SyncOnExit {  // the chunk's copy reads the staging buffer, the uploads below `w`'s vectors: none is in flight on any path out
    hipStream_t s;
    ~SyncOnExit() { (void)hipStreamSynchronize(s); }
  } sync_on_exit{s};
  const std::string where = strfmt("column '%s', row group %d of %s", pc.name.c_str(), (int)g, filename_.c_str());
  if (km.codec == 0) {
    DFX_RETURN_IF_ERROR(from_pq(pq::walk_chunk(host, len, pc, rows, where, &w)));
  } else {
    // a compressed chunk: the kernels below read the inflated image, and so does the body pass (one more synchronisation)
    std::shared_ptr<void> image;
    DFX_RETURN_IF_ERROR(inflate_chunk(host, len, (const uint8_t*)chunk.get(), km.codec, pc, rows, where, &image, &w));
    chunk = image;
  }
  counters().parquet_pages += (long long)w.infos.size();
  counters().parquet_dict_pages += w.dict_data_pages;
  counters().parquet_plain_pages += w.plain_pages;
  counters().parquet_host_walked_strings += w.walked_strings;
  if (w.pages.empty()) return Status::Err(DFX_PARSER_ERROR, "Parquet: " + where + ": no data page");
  // ---- the page table and the kernels' buffers
  std::vector<std::shared_ptr<void>> keep;
  auto upload = [&](const void* p, size_t bytes, const void** dev) -> Status {
    auto d = device_alloc(std::max<size_t>(bytes, 8), &st);
    if (!d) return st;
    if (bytes) DFX_HIP(hipMemcpyAsync(d.get(), p, bytes, hipMemcpyHostToDevice, s));
    *dev = d.get();
    keep.push_back(d);
    return Status::OK();
  };
  auto scratch = [&](size_t bytes, bool zero, void** dev) -> Status {
    auto d = device_alloc(std::max<size_t>(bytes, 8), &st);
    if (!d) return st;
    if (zero) DFX_HIP(hipMemsetAsync(d.get(), 0, std::max<size_t>(bytes, 8), s));
    *dev = d.get();
    keep.push_back(d);
    return Status::OK();
  };
  DevPqColumn C;
  memset(&C, 0, sizeof(C));
  C.chunk = (const uint8_t*)chunk.get();
  C.n_pages = (uint32_t)w.pages.size();
  C.rows = (uint32_t)rows;
  C.optional = pc.optional ? 1u : 0u;
  C.dtype = (uint32_t)pc.dtype;
  C.width = (uint32_t)pq::physical_width(pc.physical);
  C.dict_off = w.dict_off;
  C.dict_n = w.dict_n;
  const bool has_dict_pages = (w.encodings_seen >> PQ_ENC_DICT) & 1, has_rle_bool = (w.encodings_seen >> PQ_ENC_RLE_BOOL) & 1;
  DFX_RETURN_IF_ERROR(upload(w.pages.data(), sizeof(PqPage) * w.pages.size(), (const void**)&C.pages));
  if (pc.dtype == DFX_UTF8) {
    DFX_RETURN_IF_ERROR(upload(w.dict_str.data(), sizeof(uint32_t) * w.dict_str.size(), (const void**)&C.dict_str));
    DFX_RETURN_IF_ERROR(upload(w.str_offs.data(), sizeof(uint32_t) * w.str_offs.size(), (const void**)&C.str_offs));
  }
  const size_t words = (size_t)(rows + 63) / 64;
  std::shared_ptr<void> validity;
  if (pc.optional) {
    validity = device_alloc((words + 1) * 8, &st);
    if (!validity) return st;
    DFX_HIP(hipMemsetAsync(validity.get(), 0, (words + 1) * 8, s));
    C.validity = (uint64_t*)validity.get();
    DFX_RETURN_IF_ERROR(scratch(sizeof(uint32_t) * w.rank_total, false, (void**)&C.word_rank));
  }
  if (has_rle_bool) DFX_RETURN_IF_ERROR(scratch(((size_t)w.dense_total / 64 + 2) * 8, true, (void**)&C.dense_bits));
  if (has_dict_pages) DFX_RETURN_IF_ERROR(scratch(sizeof(uint32_t) * w.dense_total, false, (void**)&C.dense_idx));
  DFX_RETURN_IF_ERROR(scratch(sizeof(uint32_t) * w.pages.size(), true, (void**)&C.page_nonnull));
  DFX_RETURN_IF_ERROR(scratch(sizeof(uint32_t) * w.pages.size(), true, (void**)&C.page_decoded));
  void* ctl = nullptr;  // CTRL_WORDS words of control block, then 4 words of statistics
  DFX_RETURN_IF_ERROR(scratch(sizeof(uint32_t) * CTRL_WORDS + sizeof(uint64_t) * 4, true, &ctl));
  C.ctrl = (uint32_t*)ctl;
  C.stats = (uint64_t*)((uint8_t*)ctl + sizeof(uint32_t) * CTRL_WORDS);
  // ---- the column
  col->dtype = pc.dtype;
  col->length = rows;
  std::shared_ptr<void> vals, starts, lens;
  if (pc.dtype == DFX_UTF8) {
    starts = device_alloc(sizeof(int32_t) * (size_t)rows, &st);
    if (!starts) return st;
    lens = device_alloc(sizeof(int32_t) * (size_t)(rows + 1), &st);
    if (!lens) return st;
  } else {
    vals = device_alloc(std::max<size_t>(pc.dtype == DFX_BOOLEAN ? words * 8 : (size_t)rows * dtype_width(pc.dtype), 8), &st);
    if (!vals) return st;
  }
  DFX_HIP(launch_pq_decode(C, has_rle_bool, has_dict_pages, vals.get(), (int32_t*)starts.get(), (int32_t*)lens.get(), (double)len, s));
  struct {
    uint32_t ctrl[CTRL_WORDS];
    uint64_t stats[4];
  } back;
  DFX_HIP(hipMemcpyAsync(&back, ctl, sizeof(back), hipMemcpyDeviceToHost, s));
  DFX_HIP(hipStreamSynchronize(s));
  if (back.ctrl[CTRL_ERROR] & PQ_ERR_ALL) {
    Status err = error_from_ctrl(back.ctrl[CTRL_ERROR] & PQ_ERR_ALL);
    err.msg += " (" + where + ")";
    return err;
  }
  std::shared_ptr<void> offs, data;
  int32_t total = 0;
  if (pc.dtype == DFX_UTF8) {
    // The lengths of dictionary-encoded rows come from the dictionary: one long string referenced by many rows sums past the chunk's
    // size and past 2^31.  launch_scan_i32 stores its 64-bit sums as int32, so the total is judged from the kernel's own 64-bit sum
    // (pq::utf8_total_error) before anything is scanned, allocated or gathered: the gather never sees a wrapped offset.
    DFX_RETURN_IF_ERROR(from_pq(pq::utf8_total_error(back.stats[3], where)));
    total = (int32_t)back.stats[3];
    offs = device_alloc(sizeof(int32_t) * (size_t)(rows + 1), &st);
    if (!offs) return st;
    auto tmp = device_alloc(sizeof(uint64_t) * (size_t)(rows / 4096 + 4), &st);
    if (!tmp) return st;
    DFX_HIP(launch_scan_i32((const int32_t*)lens.get(), (int32_t*)offs.get(), rows, (uint64_t*)tmp.get(), s));
    data = device_alloc((size_t)std::max<int32_t>(total, 8), &st);
    if (!data) return st;
    // every (start, length) is an extent the host walked inside the chunk, or (0, 0); the lengths sum to `total`
    DFX_HIP(launch_utf8_gather((const uint8_t*)chunk.get(), (const int32_t*)starts.get(), (const int32_t*)offs.get(), rows, (uint8_t*)data.get(), s));
    DFX_HIP(hipStreamSynchronize(s));
  }
  counters().parquet_rle_runs += (long long)back.stats[0];
  counters().parquet_bitpacked_runs += (long long)back.stats[1];
  col->null_count = (int64_t)back.stats[2];
  if (pc.dtype == DFX_UTF8) {
    col->offsets = (const int32_t*)offs.get();
    col->data = (const uint8_t*)data.get();
    col->data_bytes = total;
    col->owners.push_back(offs);
    col->owners.push_back(data);
  } else {
    col->values = vals.get();
    col->owners.push_back(vals);
  }
  if (pc.optional && col->null_count > 0) {
    col->validity = (const uint8_t*)validity.get();
    col->owners.push_back(validity);
  }
  return Status::OK();
}

// A compressed chunk (codec 7, LZ4_RAW).  host / dev_chunk: the chunk's len bytes in the staging buffer and, once the copy in
// flight on the stream has run, on the device.  The host's header pass sizes the inflated image and fills the inflate table while
// that copy runs; k_pq_inflate inflates every page into the image; the pages' prologues and the control word come back (the first
// of the chunk's two synchronisations), and the body pass builds the page table from them.  Only a BYTE_ARRAY chunk's image is
// copied back to the host, for the length chains (parquet_inflated_bytes_to_host; a device walk of the chains would end that).
Status ParquetRelation::inflate_chunk(const uint8_t* host, size_t len, const uint8_t* dev_chunk, int32_t codec, const pq::Column& pc, int64_t rows,
                                      const std::string& where, std::shared_ptr<void>* image_out, pq::WalkedChunk* w) {
  hipStream_t s = ctx().stream;
  Status st;
  std::vector<PqInflatePage> table;
  std::vector<uint8_t> back;
  struct SyncOnExit {  // the uploads read `table`, the copy back writes `back`: none is in flight when they go
    hipStream_t s;
    ~SyncOnExit() { (void)hipStreamSynchronize(s); }
  } sync_on_exit{s};
  pq::ChunkHeaders hd;
  DFX_RETURN_IF_ERROR(from_pq(pq::walk_headers(host, len, codec, pc, where, &hd)));
  table = hd.table();
  const size_t n = table.size();
  const size_t image_bytes = (size_t)hd.image_len + 64;
  auto image = device_alloc(image_bytes, &st);
  if (!image) return st;
  DFX_HIP(hipMemsetAsync(image.get(), 0, image_bytes, s));
  auto dev_table = device_alloc(std::max<size_t>(sizeof(PqInflatePage) * n, 8), &st);
  if (!dev_table) return st;
  if (n) DFX_HIP(hipMemcpyAsync(dev_table.get(), table.data(), sizeof(PqInflatePage) * n, hipMemcpyHostToDevice, s));
  // the control block, one word of statistics and the prologues: one zeroed buffer, one copy back
  const size_t ctrl_bytes = sizeof(uint32_t) * CTRL_WORDS, back_bytes = ctrl_bytes + sizeof(uint64_t) + sizeof(PqPrologue) * n;
  auto dev_back = device_alloc(back_bytes, &st);
  if (!dev_back) return st;
  DFX_HIP(hipMemsetAsync(dev_back.get(), 0, back_bytes, s));
  DevPqInflate I;
  memset(&I, 0, sizeof(I));
  I.chunk = dev_chunk;
  I.image = (uint8_t*)image.get();
  I.pages = (const PqInflatePage*)dev_table.get();
  I.n_pages = (uint32_t)n;
  I.ctrl = (uint32_t*)dev_back.get();
  I.stats = (uint64_t*)((uint8_t*)dev_back.get() + ctrl_bytes);
  I.prologues = (PqPrologue*)((uint8_t*)dev_back.get() + ctrl_bytes + sizeof(uint64_t));
  DFX_HIP(launch_pq_inflate(I, (double)hd.image_len, s));
  back.resize(back_bytes);
  DFX_HIP(hipMemcpyAsync(back.data(), dev_back.get(), back_bytes, hipMemcpyDeviceToHost, s));
  const bool chains = pc.physical == pq::PT_BYTE_ARRAY;
  if (chains) {
    if (image_stage_bytes_ < image_bytes || !image_stage_) {
      image_stage_.reset();
      image_stage_ = pinned_alloc(image_bytes, &st);
      if (!image_stage_) return st;
      image_stage_bytes_ = image_bytes;
    }
    if (hd.image_len) DFX_HIP(hipMemcpyAsync(image_stage_.get(), image.get(), (size_t)hd.image_len, hipMemcpyDeviceToHost, s));
    counters().parquet_inflated_bytes_to_host += (long long)hd.image_len;
  }
  DFX_HIP(hipStreamSynchronize(s));
  uint32_t ctrl_error = 0;
  uint64_t sequences = 0;
  memcpy(&ctrl_error, back.data() + sizeof(uint32_t) * CTRL_ERROR, sizeof(ctrl_error));
  memcpy(&sequences, back.data() + ctrl_bytes, sizeof(sequences));
  if (ctrl_error & PQ_ERR_ALL) {
    Status err = error_from_ctrl(ctrl_error & PQ_ERR_ALL);
    err.msg += " (" + where + ")";
    return err;
  }
  counters().parquet_inflated_pages += hd.inflated_pages;
  counters().parquet_stored_pages += hd.stored_pages;
  counters().parquet_inflated_bytes += hd.inflated_bytes;
  counters().parquet_lz4_sequences += (long long)sequences;
  std::vector<PqPrologue> prologues(n);
  if (n) memcpy(prologues.data(), back.data() + ctrl_bytes + sizeof(uint64_t), sizeof(PqPrologue) * n);
  DFX_RETURN_IF_ERROR(from_pq(pq::walk_bodies(hd, chains ? (const uint8_t*)image_stage_.get() : nullptr, prologues.data(), pc, rows, where, w)));
  *image_out = image;
  return Status::OK();
}

Status ParquetRelation::load_row_group() {
  if (has_pending_) {
    needed_ = pending_needed_;
    has_pending_ = false;
  }
  loaded_any_ = true;
  const int64_t rows = meta_.row_groups[rg_].num_rows;
  rg_batch_.num_rows = rows;
  rg_batch_.columns.clear();
  rg_batch_.columns.resize(proj_.size());
  for (size_t c = 0; c < proj_.size(); ++c) {
    DeviceColumn& col = rg_batch_.columns[c];
    col.dtype = schema_.fields[c].dtype;
    col.length = rows;
    if (!is_needed(c)) {
      col.absent = true;
      continue;
    }
    DFX_RETURN_IF_ERROR(decode_chunk(rg_, c, &col));
  }
  pos_ = 0;
  rg_loaded_ = true;
  return Status::OK();
}

Status ParquetRelation::next(DeviceBatch* out, bool* has) {
  *has = false;
  for (;;) {
    if (rg_ >= meta_.row_groups.size()) return Status::OK();  // Ok(None)
    if (meta_.row_groups[rg_].num_rows == 0) {  // a row group without rows yields no batch
      ++rg_;
      continue;
    }
    if (!rg_loaded_) DFX_RETURN_IF_ERROR(load_row_group());
    break;
  }
  const int64_t rows = rg_batch_.num_rows;
  const int64_t width = batch_size_ > 0 ? (batch_size_ + 63) / 64 * 64 : rows;  // slices stay byte-aligned in every bitmap
  const int64_t n = std::min(width, rows - pos_);
  out->num_rows = n;
  out->columns.clear();
  out->columns.reserve(rg_batch_.columns.size());
  for (const DeviceColumn& c : rg_batch_.columns) {
    DeviceColumn sl = c;  // shares the owners: zero copy
    sl.length = n;
    if (!c.absent && (pos_ != 0 || n != rows)) {
      if (c.dtype == DFX_UTF8) {
        sl.offsets = c.offsets + pos_;
        sl.data_bytes = 0;  // resolved lazily by the exporter from the offsets
      } else if (c.dtype == DFX_BOOLEAN) {
        sl.values = (const uint8_t*)c.values + (pos_ >> 3);
      } else {
        sl.values = (const uint8_t*)c.values + (size_t)pos_ * dtype_width(c.dtype);
      }
      if (c.validity) sl.validity = c.validity + (pos_ >> 3);
      if (c.null_count != 0) sl.null_count = -1;
    }
    out->columns.push_back(std::move(sl));
  }
  pos_ += n;
  if (pos_ >= rows) {
    ++rg_;
    rg_loaded_ = false;
    rg_batch_ = DeviceBatch();
  }
  *has = true;
  return Status::OK();
}

}  // namespace dfx

using namespace dfx;

extern "C" {

int32_t dfx_parquet_datasource_new(const char* filename, const int32_t* projection, int32_t n_projection, int64_t batch_size,
                                   struct ArrowArrayStream* out, char* err, size_t errlen) {
  return c_abi_guard(err, errlen, [&]() -> int32_t {
    if (!filename || !out || (projection && n_projection < 0)) return to_c(Status::Err(DFX_GENERAL, "null argument"), err, errlen);
    std::unique_ptr<ParquetRelation> rel(new ParquetRelation(filename, batch_size));
    Status st = rel->open(projection, n_projection);
    if (!st.ok()) return to_c(st, err, errlen);
    export_relation(std::move(rel), out);
    return DFX_OK;
  });
}

}  // extern "C"
