// dfx_table.cpp -- HBM-resident tables (the in-memory DataSource: src/execution/datasource.rs:27-30,
// relation.rs:34-54): the scan, the concatenation of a stream's batches, the synthetic generators and the dfx_table_* C ABI.
// (The library-level C ABI -- init, info, options, counters, profiling -- is dfx_options.cpp.)
#include "dfx_gather.hpp"
#include "dfx_relation.hpp"

struct dfx_table {
  std::shared_ptr<dfx::TableData> data;
};

namespace dfx {

TableScanRelation::TableScanRelation(std::shared_ptr<const TableData> t, int64_t batch_rows, int64_t row_begin, int64_t n_rows)
    : table_(std::move(t)), batch_rows_(batch_rows) {
  begin_ = std::max<int64_t>(0, std::min(row_begin, table_->num_rows));
  end_ = (n_rows < 0 || n_rows > table_->num_rows - begin_) ? table_->num_rows : begin_ + n_rows;  // (no begin_ + n_rows overflow for an `everything` n_rows)
  pos_ = begin_;
  if (batch_rows_ <= 0) batch_rows_ = end_ > begin_ ? end_ - begin_ : 1;
  batch_rows_ = (batch_rows_ + 63) / 64 * 64;  // slices stay byte-aligned in every bitmap
}

void TableScanRelation::explain(std::string* out, int depth) const {
  std::string range = (begin_ != 0 || end_ != table_->num_rows) ? strfmt(", rows [%lld, %lld) of them", (long long)begin_, (long long)end_) : std::string();
  explain_line(out, depth, strfmt("TableScan: %lld rows resident in HBM%s, %d columns, batches of %lld rows (zero-copy slices)",
                                  (long long)table_->num_rows, range.c_str(), (int)table_->columns.size(), (long long)batch_rows_));
}

Status TableScanRelation::next(DeviceBatch* out, bool* has) {
  *has = false;
  if (pos_ >= end_) return Status::OK();  // Ok(None)
  const int64_t n = std::min(batch_rows_, end_ - pos_);
  out->num_rows = n > 0 ? n : 0;
  out->columns.clear();
  out->columns.reserve(table_->columns.size());
  for (const DeviceColumn& c : table_->columns) {
    DeviceColumn s = c;  // shares the owners: zero copy
    s.length = out->num_rows;
    if (c.dtype == DFX_UTF8) {
      s.offsets = c.offsets + pos_;
      s.data_bytes = 0;  // resolved lazily by the exporter from the offsets
    } else if (c.dtype == DFX_BOOLEAN) {
      s.values = (const uint8_t*)c.values + (pos_ >> 3);
    } else {
      s.values = (const uint8_t*)c.values + (size_t)pos_ * dtype_width(c.dtype);
    }
    if (c.validity) s.validity = c.validity + (pos_ >> 3);
    if (c.null_count != 0) s.null_count = -1;
    out->columns.push_back(std::move(s));
  }
  pos_ += batch_rows_;
  emitted_any_ = true;
  *has = true;
  return Status::OK();
}

// the columns a GROUP BY key's Int32 shadow can be made for (dfx_key_shadow.hpp): plain Int64, no nulls
static void register_key_shadows(TableData* t) {
  for (const DeviceColumn& c : t->columns)
    if (c.dtype == DFX_INT64 && !c.absent && c.null_count == 0 && c.length == t->num_rows) t->memo.key_shadows.add_column(c.values, c.length);
  // ... and an operand's Float32 shadow (dfx_value_shadow.hpp): plain Float64, no nulls
  for (const DeviceColumn& c : t->columns)
    if (c.dtype == DFX_FLOAT64 && !c.absent && c.null_count == 0 && c.length == t->num_rows) t->memo.value_shadows.add_column(c.values, c.length);
}

namespace {

// every batch of the input that has rows, and a first one that has none (its columns are what an empty table adopts)
Status collect_batches(Relation* rel, std::vector<DeviceBatch>* batches, int64_t* total) {
  for (;;) {
    DeviceBatch b;
    bool has = false;
    DFX_RETURN_IF_ERROR(rel->next(&b, &has));
    if (!has) return Status::OK();
    *total += b.num_rows;
    if (b.num_rows > 0 || batches->empty()) batches->push_back(std::move(b));
  }
}

// concatenates device batches column-wise into one resident table.  One batch is adopted as it is; several batches are
// copied: fixed-width values with D2D copies, validity / Boolean bits and Utf8 cells with the multi-batch gathers of
// dfx_k_sort.hip driven by the identity permutation (BatchGather, dfx_gather.hpp).
Status build_table(Relation* rel, std::shared_ptr<TableData>* out) {
  std::shared_ptr<TableData> t(new TableData());
  t->schema = rel->schema();
  std::vector<DeviceBatch> batches;
  int64_t total = 0;
  DFX_RETURN_IF_ERROR(collect_batches(rel, &batches, &total));
  t->num_rows = total;
  const size_t nc = t->schema.fields.size();
  t->columns.resize(nc);
  if (batches.empty()) {
    for (size_t c = 0; c < nc; ++c) {
      t->columns[c].dtype = t->schema.fields[c].dtype;
      t->columns[c].length = 0;
    }
    *out = t;
    return Status::OK();
  }
  BatchGather gather(batches, "multi-batch upload of 2^32 or more rows with nullable / Utf8 / Boolean columns");
  for (size_t c = 0; c < nc; ++c) {
    DeviceColumn& col = t->columns[c];
    if (batches.size() == 1 && batches[0].columns[c].bit_offset == 0) {  // common case: adopt
      col = batches[0].columns[c];
      continue;
    }
    col.dtype = t->schema.fields[c].dtype;
    col.length = total;
    std::shared_ptr<void> valid;
    int64_t zeros = 0;
    DFX_RETURN_IF_ERROR(gather.validity((int)c, &valid, &zeros));
    if (valid) {  // this table's rule: the bitmap of a column that had one is kept, all valid or not
      col.validity = (const uint8_t*)valid.get();
      col.null_count = zeros;
      col.owners.push_back(valid);
    }
    DFX_RETURN_IF_ERROR(gather.values((int)c, "Utf8 column of a resident table", &col));
  }
  DFX_HIP(hipStreamSynchronize(ctx().stream));
  register_key_shadows(t.get());
  *out = t;
  return Status::OK();
}

}  // namespace
}  // namespace dfx

using namespace dfx;

extern "C" {

int32_t dfx_table_from_stream(struct ArrowArrayStream* input, dfx_table** out, char* err, size_t errlen) {
  return c_abi_guard(err, errlen, [&]() -> int32_t {
    if (!out) return to_c(Status::Err(DFX_GENERAL, "null argument"), err, errlen);
    *out = nullptr;
    Status st = ensure_init();
    if (!st.ok()) return to_c(st, err, errlen);
    std::unique_ptr<Relation> in;
    st = adopt_input_stream(input, &in);
    if (!st.ok()) return to_c(st, err, errlen);
    std::shared_ptr<TableData> t;
    st = build_table(in.get(), &t);
    if (!st.ok()) return to_c(st, err, errlen);
    *out = new dfx_table{t};
    return DFX_OK;
  });
}

static_assert(dfx::kSynthNullStream == DFX_SYNTH_NULL_STREAM, "device and header agree on the validity stream");
int32_t dfx_table_synth(const dfx_synth_column* cols, int32_t n_cols, uint64_t seed, int64_t row_begin, int64_t n_rows,
                        dfx_table** out, char* err, size_t errlen) {
  return c_abi_guard(err, errlen, [&]() -> int32_t {
    if (!out || !cols || n_cols < 1 || n_rows < 0) return to_c(Status::Err(DFX_GENERAL, "invalid argument"), err, errlen);
    *out = nullptr;
    Status st = ensure_init();
    if (!st.ok()) return to_c(st, err, errlen);
    std::shared_ptr<TableData> t(new TableData());
    t->num_rows = n_rows;
    hipStream_t s = ctx().stream;
    for (int c = 0; c < n_cols; ++c) {
      Field f;
      f.name = cols[c].name ? cols[c].name : strfmt("c%d", c);
      const int kind = DFX_SYNTH_KIND(cols[c].kind);
      const uint32_t permille = (uint32_t)DFX_SYNTH_NULL_PERMILLE(cols[c].kind);
      f.dtype = (kind == DFX_SYNTH_I64_UNIFORM || kind == DFX_SYNTH_I64_ZIPF || kind == DFX_SYNTH_I64_WIDE) ? DFX_INT64 : kind == DFX_SYNTH_I32_UNIFORM ? DFX_INT32 : DFX_FLOAT64;
      f.nullable = permille != 0;
      if (cols[c].kind < 0 || kind > DFX_SYNTH_I64_WIDE || permille > 1000 || (cols[c].kind >> 18) != 0)
        return to_c(Status::Err(DFX_NOT_IMPLEMENTED, "unknown synthetic column kind"), err, errlen);
      t->schema.fields.push_back(f);
      DeviceColumn col;
      col.dtype = f.dtype;
      col.length = n_rows;
      auto vals = device_alloc((size_t)std::max<int64_t>(n_rows, 1) * 8, &st);  // (4-byte kinds: half used)
      if (!vals) return to_c(st, err, errlen);
      hipError_t e = launch_synth(kind, cols[c].column_id, cols[c].p0, cols[c].p1, seed, row_begin, n_rows, vals.get(), s);
      if (e != hipSuccess) return to_c(Status::Err(DFX_EXECUTION_ERROR, hipGetErrorString(e)), err, errlen);
      col.values = vals.get();
      col.owners.push_back(vals);
      if (permille != 0 && n_rows > 0) {
        auto bits = device_alloc((size_t)((n_rows + 63) / 64) * 8 + 8, &st);
        if (!bits) return to_c(st, err, errlen);
        uint64_t* count = (uint64_t*)bits.get() + (n_rows + 63) / 64;  // (the word behind the bitmap)
        e = hipMemsetAsync(count, 0, 8, s);
        if (e == hipSuccess) e = launch_synth_validity(cols[c].column_id, permille, seed, row_begin, n_rows, (uint64_t*)bits.get(), count, s);
        uint64_t nulls = 0;
        if (e == hipSuccess) e = hipMemcpyAsync(&nulls, count, 8, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return to_c(Status::Err(DFX_EXECUTION_ERROR, hipGetErrorString(e)), err, errlen);
        col.validity = (const uint8_t*)bits.get();
        col.bit_offset = 0;
        col.null_count = (int64_t)nulls;
        col.owners.push_back(bits);
      }
      t->columns.push_back(std::move(col));
    }
    hipError_t e = hipStreamSynchronize(s);
    if (e != hipSuccess) return to_c(Status::Err(DFX_EXECUTION_ERROR, hipGetErrorString(e)), err, errlen);
    register_key_shadows(t.get());
    *out = new dfx_table{t};
    return DFX_OK;
  });
}

int64_t dfx_table_num_rows(const dfx_table* t) { return t ? t->data->num_rows : 0; }
int32_t dfx_table_num_columns(const dfx_table* t) { return t ? (int32_t)t->data->columns.size() : 0; }
const void* dfx_table_column_device_ptr(const dfx_table* t, int32_t column) {
  if (!t || column < 0 || column >= (int32_t)t->data->columns.size()) return nullptr;
  return t->data->columns[column].values;
}

int32_t dfx_table_scan_new(const dfx_table* t, int64_t batch_rows, struct ArrowArrayStream* out, char* err, size_t errlen) {
  return c_abi_guard(err, errlen, [&]() -> int32_t {
    if (!t || !out) return to_c(Status::Err(DFX_GENERAL, "null argument"), err, errlen);
    std::unique_ptr<Relation> rel(new TableScanRelation(t->data, batch_rows));
    export_relation(std::move(rel), out);
    return DFX_OK;
  });
}

int32_t dfx_table_scan_range_new(const dfx_table* t, int64_t row_begin, int64_t n_rows, int64_t batch_rows, struct ArrowArrayStream* out,
                                 char* err, size_t errlen) {
  return c_abi_guard(err, errlen, [&]() -> int32_t {
    if (!t || !out) return to_c(Status::Err(DFX_GENERAL, "null argument"), err, errlen);
    if (row_begin < 0 || (row_begin & 63) != 0 || row_begin > t->data->num_rows)
      return to_c(Status::Err(DFX_GENERAL, "row_begin must be a multiple of 64 inside the table"), err, errlen);
    std::unique_ptr<Relation> rel(new TableScanRelation(t->data, batch_rows, row_begin, n_rows));
    export_relation(std::move(rel), out);
    return DFX_OK;
  });
}

void dfx_table_free(dfx_table* t) { delete t; }
}  // extern "C"
