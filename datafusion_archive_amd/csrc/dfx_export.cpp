// dfx_export.cpp -- device relation -> host Arrow C stream: the exported stream of every operator, the download of a device
// batch into host Arrow memory, and the C-ABI calls that work on any exported stream (drain on the device, explain).
#include "dfx_relation.hpp"

#include <stdlib.h>
#include <string.h>

namespace dfx {

namespace {

struct ExportedStream {
  std::unique_ptr<Relation> rel;
  std::string last_error;
};

struct ArrayPriv {
  std::vector<std::shared_ptr<void>> pinned; // large result buffers: pooled pinned memory (fast D2H)
  std::vector<void*> host_buffers;           // malloc'd, 64-byte aligned
  std::vector<const void*> buffer_ptrs;      // this array's buffers
  std::vector<struct ArrowArray> kids;
  std::vector<struct ArrowArray*> kid_ptrs;
};

void release_array(struct ArrowArray* a) {
  if (!a || !a->release) return;
  ArrayPriv* p = (ArrayPriv*)a->private_data;
  for (auto& k : p->kids)
    if (k.release) k.release(&k);
  for (void* b : p->host_buffers) free(b);
  delete p;
  a->release = nullptr;
}

void* host_alloc(size_t bytes) {
  void* p = nullptr;
  const size_t cap = ((bytes ? bytes : 1) + 63) / 64 * 64;  // padded to 64 bytes, tail zeroed
  if (posix_memalign(&p, 64, cap) != 0) return nullptr;
  memset((uint8_t*)p + (cap - 64), 0, 64);
  return p;
}

// result buffer owned by the exported array: pinned (pooled) when large, so the D2H copy runs at
// PCIe speed instead of through a pageable staging copy
void* alloc_result(ArrayPriv* p, size_t bytes) {
  ScopedUs t_alloc(&counters().export_alloc_us);
  if (bytes >= (1u << 16)) {
    Status st;
    std::shared_ptr<void> b = pinned_alloc(bytes + 64, &st);
    if (b) {
      p->pinned.push_back(b);
      return b.get();
    }
  }
  void* raw = host_alloc(bytes);
  if (raw) p->host_buffers.push_back(raw);
  return raw;
}

// move `n` bits starting at src bit `off` to bit 0 of dst (dst pre-zeroed)
void realign_bits(const uint8_t* src, int64_t off, int64_t n, uint8_t* dst) {
  for (int64_t i = 0; i < n; ++i)
    if ((src[(off + i) >> 3] >> ((off + i) & 7)) & 1) dst[i >> 3] |= (uint8_t)(1u << (i & 7));
}

Status download_column(const DeviceColumn& c, struct ArrowArray* out, std::vector<std::function<void()>>* fixups) {
  ArrayPriv* p = new ArrayPriv();
  memset(out, 0, sizeof(*out));
  out->private_data = p;
  out->release = release_array;
  out->length = c.length;
  out->offset = 0;
  const int64_t n = c.length;
  hipStream_t s = ctx().stream;
  // validity
  void* vbuf = nullptr;
  if (c.validity && c.null_count != 0) {
    const size_t bytes = (size_t)((c.bit_offset + n + 7) >> 3);
    void* raw = alloc_result(p, bytes);
    if (!raw) return Status::Err(DFX_EXECUTION_ERROR, "host allocation failed");
    DFX_HIP(hipMemcpyAsync(raw, c.validity, bytes, hipMemcpyDeviceToHost, s));
    vbuf = raw;
    if (c.bit_offset != 0) {
      void* al = alloc_result(p, (size_t)((n + 7) >> 3));
      memset(al, 0, (size_t)((n + 7) >> 3));
      const int64_t bo = c.bit_offset;
      fixups->push_back([raw, al, bo, n]() { realign_bits((const uint8_t*)raw, bo, n, (uint8_t*)al); });
      vbuf = al;
    }
    ArrowArray* oo = out;
    fixups->push_back([oo, vbuf, n]() {  // count nulls once the bits are on the host
      int64_t set = 0;
      const uint8_t* b = (const uint8_t*)vbuf;
      for (int64_t i = 0; i < n; ++i) set += (b[i >> 3] >> (i & 7)) & 1;
      oo->null_count = n - set;
    });
  }
  p->buffer_ptrs.push_back(vbuf);
  if (c.dtype == DFX_UTF8) {
    void* obuf = alloc_result(p, sizeof(int32_t) * (size_t)(n + 1));
    if (!obuf) return Status::Err(DFX_EXECUTION_ERROR, "host allocation failed");
    if (c.offsets) DFX_HIP(hipMemcpyAsync(obuf, c.offsets, sizeof(int32_t) * (size_t)(n + 1), hipMemcpyDeviceToHost, s));
    else memset(obuf, 0, sizeof(int32_t) * (size_t)(n + 1));
    p->buffer_ptrs.push_back(obuf);
    p->buffer_ptrs.push_back(nullptr);  // data: sized from the offsets once they are on the host
    const uint8_t* dev_data = c.data;
    fixups->push_back([obuf, p, dev_data, n]() {  // fetch the referenced bytes, rebase offsets to 0
      int32_t* o = (int32_t*)obuf;
      const int32_t o0 = o[0];
      const int64_t nbytes = (int64_t)o[n] - o0;
      void* dbuf = alloc_result(p, (size_t)(nbytes > 0 ? nbytes : 1));
      if (nbytes > 0 && dev_data) (void)hipMemcpy(dbuf, dev_data + o0, (size_t)nbytes, hipMemcpyDeviceToHost);
      if (o0 != 0)
        for (int64_t i = 0; i <= n; ++i) o[i] -= o0;
      p->buffer_ptrs[2] = dbuf;
    });
    out->n_buffers = 3;
  } else if (c.dtype == DFX_BOOLEAN) {
    const size_t bytes = (size_t)((c.bit_offset + n + 7) >> 3);
    void* raw = alloc_result(p, bytes);
    if (!raw) return Status::Err(DFX_EXECUTION_ERROR, "host allocation failed");
    if (n) DFX_HIP(hipMemcpyAsync(raw, c.values, bytes, hipMemcpyDeviceToHost, s));
    void* vals = raw;
    if (c.bit_offset != 0) {
      void* al = alloc_result(p, (size_t)((n + 7) >> 3));
      memset(al, 0, (size_t)((n + 7) >> 3));
      const int64_t bo = c.bit_offset;
      fixups->push_back([raw, al, bo, n]() { realign_bits((const uint8_t*)raw, bo, n, (uint8_t*)al); });
      vals = al;
    }
    p->buffer_ptrs.push_back(vals);
    out->n_buffers = 2;
  } else {
    const size_t bytes = (size_t)n * dtype_width(c.dtype);
    if (c.host_values && c.host_values_of == c.values && c.host_bytes == bytes && bytes) {  // already on the host (see DeviceColumn)
      p->pinned.push_back(c.host_values);
      p->buffer_ptrs.push_back(c.host_values.get());
      out->n_buffers = 2;
      out->buffers = p->buffer_ptrs.data();
      out->null_count = 0;
      ++counters().export_host_ready;
      return Status::OK();
    }
    void* raw = alloc_result(p, bytes);
    if (!raw) return Status::Err(DFX_EXECUTION_ERROR, "host allocation failed");
    // large fixed-width result columns (pinned destination): copied by a kernel on the query's stream when the option
    // says so (export.kernel_copy; the copy engines' path has sporadic multi-millisecond stalls on these boxes)
    if (bytes >= (1u << 16) && agg_options().export_kernel_copy && !p->pinned.empty() && p->pinned.back().get() == raw) {
      DFX_HIP(launch_copy_to_host(c.values, raw, bytes, s));
    } else if (bytes) {
      DFX_HIP(hipMemcpyAsync(raw, c.values, bytes, hipMemcpyDeviceToHost, s));
    }
    p->buffer_ptrs.push_back(raw);
    out->n_buffers = 2;
  }
  out->buffers = p->buffer_ptrs.data();
  out->null_count = 0;
  return Status::OK();
}

Status download_batch(const DeviceBatch& b, struct ArrowArray* out) {
  ScopedUs t_export(&counters().export_us);
  ArrayPriv* p = new ArrayPriv();
  memset(out, 0, sizeof(*out));
  out->private_data = p;
  out->release = release_array;
  out->length = b.num_rows;
  p->kids.resize(b.columns.size());
  p->kid_ptrs.resize(b.columns.size());
  std::vector<std::function<void()>> fixups;
  for (size_t i = 0; i < b.columns.size(); ++i) {
    memset(&p->kids[i], 0, sizeof(struct ArrowArray));
    p->kid_ptrs[i] = &p->kids[i];
  }
  Status st;
  for (size_t i = 0; i < b.columns.size() && st.ok(); ++i) st = download_column(b.columns[i], &p->kids[i], &fixups);
  if (st.ok()) {
    hipError_t e = hipStreamSynchronize(ctx().stream);
    if (e != hipSuccess) st = Status::Err(DFX_EXECUTION_ERROR, strfmt("HIP error %s after D2H", hipGetErrorString(e)));
  }
  if (!st.ok()) {
    release_array(out);
    return st;
  }
  for (auto& f : fixups) f();
  p->buffer_ptrs.push_back(nullptr);  // struct validity
  out->n_buffers = 1;
  out->buffers = p->buffer_ptrs.data();
  out->n_children = (int64_t)p->kids.size();
  out->children = p->kid_ptrs.empty() ? nullptr : p->kid_ptrs.data();
  return Status::OK();
}

int exported_get_schema(struct ArrowArrayStream* s, struct ArrowSchema* out) {
  ExportedStream* es = (ExportedStream*)s->private_data;
  schema_to_arrow(es->rel->schema(), out);
  return 0;
}

int exported_get_next(struct ArrowArrayStream* s, struct ArrowArray* out) {
  ExportedStream* es = (ExportedStream*)s->private_data;
  memset(out, 0, sizeof(*out));
  DeviceBatch b;
  bool has = false;
  Status st;
  try {
    st = es->rel->next(&b, &has);
    if (st.ok() && has) st = download_batch(b, out);
  } catch (const std::exception& e) {  // nothing unwinds across the C ABI
    st = Status::Err(DFX_INTERNAL_ERROR, std::string("internal exception: ") + e.what());
  } catch (...) {
    st = Status::Err(DFX_INTERNAL_ERROR, "internal exception");
  }
  if (!st.ok()) {
    es->last_error = st.msg;
    if (out->release) out->release(out);
    memset(out, 0, sizeof(*out));
    return st.code;
  }
  return 0;  // released (zeroed) array == end of stream
}

const char* exported_get_last_error(struct ArrowArrayStream* s) {
  ExportedStream* es = (ExportedStream*)s->private_data;
  return es->last_error.empty() ? nullptr : es->last_error.c_str();
}

void exported_release(struct ArrowArrayStream* s) {
  if (!s || !s->release) return;
  delete (ExportedStream*)s->private_data;
  s->release = nullptr;
  s->private_data = nullptr;
}

}  // namespace

void export_relation(std::unique_ptr<Relation> rel, struct ArrowArrayStream* out) {
  ExportedStream* es = new ExportedStream();
  es->rel = std::move(rel);
  memset(out, 0, sizeof(*out));
  out->get_schema = exported_get_schema;
  out->get_next = exported_get_next;
  out->get_last_error = exported_get_last_error;
  out->release = exported_release;
  out->private_data = es;
}

Relation* peek_exported(struct ArrowArrayStream* s) {
  if (!s || s->release != exported_release) return nullptr;
  return ((ExportedStream*)s->private_data)->rel.get();
}

std::unique_ptr<Relation> take_exported(struct ArrowArrayStream* s) {
  if (!s || s->release != exported_release) return nullptr;
  ExportedStream* es = (ExportedStream*)s->private_data;
  std::unique_ptr<Relation> rel = std::move(es->rel);
  delete es;
  memset(s, 0, sizeof(*s));
  return rel;
}

}  // namespace dfx

using namespace dfx;

extern "C" {

// Measurement hook: pull every batch of a library stream and leave it ON THE DEVICE (no host RecordBatch is built, no
// D2H copy) -- what an operator stacked on top would see.  bench.py times FilterRelation's mask + compaction kernels
// with it (BASELINE config 2 as written); rows / batches count what came out.
int32_t dfx_relation_drain_device(struct ArrowArrayStream* stream, int64_t* rows, int64_t* batches, char* err, size_t errlen) {
  return c_abi_guard(err, errlen, [&]() -> int32_t {
    Relation* r = peek_exported(stream);
    if (!r) return to_c(Status::Err(DFX_GENERAL, "not a stream of this library"), err, errlen);
    int64_t nr = 0, nb = 0;
    for (;;) {
      DeviceBatch b;
      bool has = false;
      Status st = r->next(&b, &has);
      if (!st.ok()) return to_c(st, err, errlen);
      if (!has) break;
      nr += b.num_rows;
      ++nb;
    }
    hipError_t e = hipStreamSynchronize(ctx().stream);
    if (e != hipSuccess) return to_c(Status::Err(DFX_EXECUTION_ERROR, strfmt("HIP error %s", hipGetErrorString(e))), err, errlen);
    if (rows) *rows = nr;
    if (batches) *batches = nb;
    return DFX_OK;
  });
}

int64_t dfx_relation_explain(struct ArrowArrayStream* stream, char* buf, size_t buflen) {
  try {
    Relation* r = peek_exported(stream);
    if (!r) return -1;
    std::string text;
    r->explain(&text, 0);
    if (buf && buflen) snprintf(buf, buflen, "%s", text.c_str());
    return (int64_t)text.size();
  } catch (...) {
    return -1;
  }
}

}  // extern "C"
