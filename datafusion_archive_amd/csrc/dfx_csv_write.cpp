// dfx_csv_write.cpp -- the executor of PhysicalPlan::Write { plan, filename, kind } ("execute a logical plan and write the
// output to a file", src/execution/physicalplan.rs:24-29), which the reference declares and never runs; kind = CSV.
//
// A sink, not a relation: it pulls its input to the end.  A stream of this library is unwrapped and its batches stay on the
// device; a foreign stream goes through HostStreamRelation like any operator input.  Every batch (in launches of at most
// kCwBatchRows rows) becomes text on the device (dfx_k_csvwrite.hip) and reaches the file through two pinned staging
// buffers: the fwrite of piece i overlaps the D2H copy of piece i + 1, the mirror of CsvRelation::open.  The text is written
// to `filename` + ".dfx-partial" and renamed at the end, so a failed write leaves nothing under the final name.
//
// Semantics (deviation D11, parity unpinned: arrow 0.12 has no csv writer): the file read back by dfx_csv_datasource_new
// with the same schema gives the same rows -- DESIGN.md section 9d lists the layout and the exceptions.
#include <errno.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>

#include "dfx_csvwrite.hpp"
#include "dfx_numfmt.hpp"
#include "dfx_relation.hpp"

namespace dfx {

namespace {

static_assert(kNfMaxF64 == 24 && kNfMaxCell >= kNfMaxF64 && kNfMaxCell >= kNfMaxInt && kNfMaxCell >= kNfMaxF32,
              "the slot of a fixed-width cell is sized by these bounds");

constexpr size_t kCwPiece = 8u << 20;  // bytes per pinned staging buffer

void append_name_cell(const std::string& name, bool one_column, std::string* out) {
  uint64_t quotes = 0;
  const bool quoted = nf_csv_scan((const uint8_t*)name.data(), name.size(), &quotes) || (one_column && name.empty());
  const size_t at = out->size();
  out->resize(at + (size_t)nf_csv_cell_len(name.size(), quotes, quoted));
  nf_csv_put_cell((const uint8_t*)name.data(), name.size(), quoted, (uint8_t*)&(*out)[at]);
}

class CsvSink {
 public:
  CsvSink(std::unique_ptr<Relation> in, std::string filename) : in_(std::move(in)), final_(std::move(filename)), tmp_(final_ + ".dfx-partial") {}
  ~CsvSink() {
    if (fp_) fclose(fp_);
    if (fp_ || created_) remove(tmp_.c_str());
    for (int i = 0; i < 2; ++i)
      if (done_[i]) (void)hipEventDestroy(done_[i]);
  }
  Status run(int64_t* rows, int64_t* bytes);

 private:
  Status open();
  Status put(const void* p, size_t n) {
    if (n && fwrite(p, 1, n, fp_) != n) return Status::Err(DFX_IO_ERROR, strfmt("write to %s failed: %s", tmp_.c_str(), strerror(errno)));
    bytes_ += (int64_t)n;
    return Status::OK();
  }
  Status write_rows(const DeviceBatch& b, int64_t r0, int64_t n);
  Status drain_text(const uint8_t* text, uint64_t total);
  std::unique_ptr<Relation> in_;
  std::string final_, tmp_;
  FILE* fp_ = nullptr;
  bool created_ = false;
  int64_t bytes_ = 0;
  std::shared_ptr<void> stage_[2];
  hipEvent_t done_[2] = {nullptr, nullptr};
};

Status CsvSink::open() {
  const SchemaInfo& sc = in_->schema();
  if (sc.fields.empty()) return Status::Err(DFX_GENERAL, "CSV writer needs a schema with at least one column");
  if (sc.fields.size() > (size_t)kCwMaxCols) return Status::Err(DFX_NOT_IMPLEMENTED, strfmt("CSV writer with more than %d columns", kCwMaxCols));
  for (const Field& f : sc.fields)
    if (f.dtype < DFX_BOOLEAN || f.dtype > DFX_UTF8) return Status::Err(DFX_NOT_IMPLEMENTED, std::string("CSV column of type ") + dtype_name(f.dtype));
  fp_ = fopen(tmp_.c_str(), "wb");
  if (!fp_) return Status::Err(DFX_IO_ERROR, strfmt("cannot create %s: %s", tmp_.c_str(), strerror(errno)));
  created_ = true;
  std::string header;
  for (size_t i = 0; i < sc.fields.size(); ++i) {
    append_name_cell(sc.fields[i].name, sc.fields.size() == 1, &header);
    header += i + 1 < sc.fields.size() ? ',' : '\n';
  }
  return put(header.data(), header.size());
}

// device text -> file: the D2H copy of piece i + 1 runs while piece i is written
Status CsvSink::drain_text(const uint8_t* text, uint64_t total) {
  hipStream_t s = ctx().stream;
  Status st;
  for (int i = 0; i < 2; ++i) {
    if (!stage_[i]) {
      stage_[i] = pinned_alloc(kCwPiece, &st);
      if (!stage_[i]) return st;
    }
    if (!done_[i]) DFX_HIP(hipEventCreateWithFlags(&done_[i], hipEventDisableTiming));
  }
  const uint64_t pieces = (total + kCwPiece - 1) / kCwPiece;
  for (uint64_t i = 0; i <= pieces; ++i) {
    if (i < pieces) {  // (buffer i & 1 was written out in iteration i - 1, before this copy is queued)
      const size_t want = (size_t)std::min<uint64_t>(kCwPiece, total - i * kCwPiece);
      DFX_HIP(hipMemcpyAsync(stage_[i & 1].get(), text + i * kCwPiece, want, hipMemcpyDeviceToHost, s));
      DFX_HIP(hipEventRecord(done_[i & 1], s));
    }
    if (i > 0) {
      const uint64_t j = i - 1;
      DFX_HIP(hipEventSynchronize(done_[j & 1]));
      DFX_RETURN_IF_ERROR(put(stage_[j & 1].get(), (size_t)std::min<uint64_t>(kCwPiece, total - j * kCwPiece)));
    }
  }
  return Status::OK();
}

Status CsvSink::write_rows(const DeviceBatch& b, int64_t r0, int64_t n) {
  hipStream_t s = ctx().stream;
  Status st;
  DevCwPlan plan;
  memset(&plan, 0, sizeof(plan));
  plan.n_cols = (int32_t)b.columns.size();
  for (int c = 0; c < plan.n_cols; ++c) {
    const DeviceColumn& col = b.columns[(size_t)c];
    DevCwCol& d = plan.col[c];
    if (col.absent || col.length < r0 + n) return Status::Err(DFX_INTERNAL_ERROR, "CSV writer: a column of the batch is absent or short");
    d.dtype = (uint8_t)col.dtype;
    d.validity = (col.validity && col.null_count != 0) ? col.validity : nullptr;
    d.bit_offset = col.bit_offset + r0;
    if (col.dtype == DFX_UTF8) {
      if (!col.offsets) return Status::Err(DFX_INTERNAL_ERROR, "CSV writer: Utf8 column without offsets");
      d.offsets = col.offsets + r0;
      d.data = col.data;
    } else if (col.dtype == DFX_BOOLEAN) {
      d.values = col.values;
    } else {
      d.values = (const uint8_t*)col.values + (size_t)r0 * (size_t)dtype_width(col.dtype);
    }
  }
  const uint32_t stride = csvw_layout(&plan);
  const int64_t n_tiles = (n + 63) / 64;
  auto slots = device_alloc((size_t)n_tiles * 64 * stride, &st);
  if (!slots) return st;
  auto tiles = device_alloc(sizeof(uint64_t) * (size_t)(2 * n_tiles + 1 + 2), &st);  // tile_bytes, tile_base (+ 1), ctrl
  if (!tiles) return st;
  uint64_t* tile_bytes = (uint64_t*)tiles.get();
  uint64_t* tile_base = tile_bytes + n_tiles;
  uint64_t* ctrl = tile_base + n_tiles + 1;
  DFX_HIP(hipMemsetAsync(ctrl, 0, 2 * sizeof(uint64_t), s));
  DFX_HIP(launch_csvw_format(plan, n, (uint8_t*)slots.get(), tile_bytes, s));
  DFX_HIP(launch_csvw_scan(tile_bytes, n_tiles, tile_base, s));
  uint64_t total = 0;
  DFX_HIP(hipMemcpyAsync(&total, tile_base + n_tiles, sizeof(uint64_t), hipMemcpyDeviceToHost, s));
  DFX_HIP(hipStreamSynchronize(s));
  auto text = device_alloc((size_t)total + 16, &st);
  if (!text) return st;
  DFX_HIP(launch_csvw_assemble(plan, n, (const uint8_t*)slots.get(), tile_base, (uint8_t*)text.get(), total, ctrl, (double)total, s));
  uint64_t hc[2] = {0, 0};
  DFX_HIP(hipMemcpyAsync(hc, ctrl, sizeof(hc), hipMemcpyDeviceToHost, s));
  DFX_RETURN_IF_ERROR(drain_text((const uint8_t*)text.get(), total));
  DFX_HIP(hipStreamSynchronize(s));
  if (hc[0] != 0) return Status::Err(DFX_INTERNAL_ERROR, "CSV writer: the format and assemble kernels disagree about a tile's length");
  counters().csv_write_cells += (long long)n * plan.n_cols;
  counters().csv_write_general_tiles += (long long)hc[1];
  return Status::OK();
}

Status CsvSink::run(int64_t* rows, int64_t* bytes) {
  DFX_RETURN_IF_ERROR(open());
  int64_t n_rows = 0;
  for (;;) {
    DeviceBatch b;
    bool has = false;
    DFX_RETURN_IF_ERROR(in_->next(&b, &has));
    if (!has) break;
    if (b.columns.size() != in_->schema().fields.size()) return Status::Err(DFX_INTERNAL_ERROR, "CSV writer: batch and schema disagree");
    for (int64_t r0 = 0; r0 < b.num_rows; r0 += kCwBatchRows) DFX_RETURN_IF_ERROR(write_rows(b, r0, std::min<int64_t>(kCwBatchRows, b.num_rows - r0)));
    n_rows += b.num_rows;
  }
  FILE* fp = fp_;
  fp_ = nullptr;
  if (fclose(fp) != 0) return Status::Err(DFX_IO_ERROR, strfmt("closing %s failed: %s", tmp_.c_str(), strerror(errno)));
  if (rename(tmp_.c_str(), final_.c_str()) != 0) return Status::Err(DFX_IO_ERROR, strfmt("cannot rename %s to %s: %s", tmp_.c_str(), final_.c_str(), strerror(errno)));
  created_ = false;
  counters().csv_write_bytes += bytes_;
  if (rows) *rows = n_rows;
  if (bytes) *bytes = bytes_;
  return Status::OK();
}

}  // namespace

}  // namespace dfx

using namespace dfx;

extern "C" {

int32_t dfx_csv_write(struct ArrowArrayStream* input, const char* filename, const dfx_option* options, int32_t n_options,
                      int64_t* rows_out, int64_t* bytes_out, char* err, size_t errlen) {
  return c_abi_guard(err, errlen, [&]() -> int32_t {
    if (!input || !filename) return to_c(Status::Err(DFX_GENERAL, "null argument"), err, errlen);
    if (n_options > 0)  // the writer defines no option of its own
      return to_c(Status::Err(DFX_GENERAL, std::string("unknown option ") + ((options && options[0].key) ? options[0].key : "(null)")), err, errlen);
    Status st = ensure_init();  // no device: nothing is created, there is no host formatting path
    if (!st.ok()) return to_c(st, err, errlen);
    std::unique_ptr<Relation> in;
    st = adopt_input_stream(input, &in);
    if (!st.ok()) return to_c(st, err, errlen);
    CsvSink sink(std::move(in), filename);
    st = sink.run(rows_out, bytes_out);
    if (!st.ok()) {
      (void)hipStreamSynchronize(ctx().stream);  // nothing of this call is in flight when its buffers go
      return to_c(st, err, errlen);
    }
    return DFX_OK;
  });
}

// One value formatted on the host by the code the kernel runs (dfx_numfmt.hpp).  See include/dfx.h.
int32_t dfx_debug_format_value(int32_t dtype, uint64_t bits, char* buf, size_t buflen) {
  if (!buf) return -1;
  if (dtype == DFX_UTF8) {  // buf holds the value on entry; the cell replaces it
    const uint64_t n = bits & ~(1ull << 63);
    const bool force = (bits >> 63) != 0;
    if (n > buflen) return -1;
    uint64_t quotes = 0;
    const bool quoted = nf_csv_scan((const uint8_t*)buf, n, &quotes) || (force && n == 0);
    const uint64_t len = nf_csv_cell_len(n, quotes, quoted);
    if (len > buflen || len > (uint64_t)INT32_MAX) return -1;
    const std::string value(buf, (size_t)n);
    if (nf_csv_put_cell((const uint8_t*)value.data(), n, quoted, (uint8_t*)buf) != len) return -1;
    if (len < buflen) buf[len] = 0;
    return (int32_t)len;
  }
  if (dtype < DFX_BOOLEAN || dtype > DFX_FLOAT64) return -1;
  uint8_t cell[kNfMaxCell + 8];
  const int len = nf_format_value(dtype, bits, cell);
  if (len <= 0 || len > nf_max_cell(dtype)) return -1;  // the bound the kernel sizes its slots by
  if ((size_t)len > buflen) return -1;
  memcpy(buf, cell, (size_t)len);
  if ((size_t)len < buflen) buf[len] = 0;
  return len;
}

}  // extern "C"
