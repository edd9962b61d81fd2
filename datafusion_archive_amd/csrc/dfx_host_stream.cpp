// dfx_host_stream.cpp -- host Arrow C stream -> device batches: HostStreamRelation and adopt_input_stream.
#include "dfx_relation.hpp"

#include <atomic>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <string.h>

namespace dfx {

namespace {

// Host Arrow batches -> HBM (relation.rs:34-54 is the reference's feed).  PCIe Gen5 x16 moves ~57 GB/s out of
// pinned memory here, HBM streams at > 6 TB/s: this relation is bound by the link whatever it does, and its forms (option
// "host.stream" = 0 / 1 / 2 / 3, HostStreamOptions::mode; measured by tools/pin_probe.py, tools/host_stream_probe.py and
// bench.py host_streamed_pcie_inclusive) differ by how close they get to it: see next_in_order, next_staged, next_one_ahead.
// In every form the producer's buffers are only read between get_next and release (tests/c_abi/host_stream.c poisons them on
// release), and columns nobody reads downstream never cross the link (require_columns).
class HostStreamRelation : public Relation {
 public:
  explicit HostStreamRelation(struct ArrowArrayStream* s) {
    stream_ = *s;  // move
    memset(s, 0, sizeof(*s));
  }
  ~HostStreamRelation() override {
    drop(&pending_);
    if (copy_stream_) (void)hipStreamSynchronize(copy_stream_);  // (staged pieces still crossing the link read the pinned slots)
    for (hipEvent_t e : slot_event_)
      if (e) (void)hipEventDestroy(e);
    if (batch_event_) (void)hipEventDestroy(batch_event_);
    if (fence_) (void)hipEventDestroy(fence_);
    if (copy_stream_) (void)hipStreamDestroy(copy_stream_);
    if (stream_.release) stream_.release(&stream_);
  }
  RelationKind kind() const override { return REL_HOST_STREAM; }
  void host_stream_options(const HostStreamOptions& o) override {
    if (started_ || opts_set_) return;  // the first operator above decides, before the first batch
    hopt_ = o;
    opts_set_ = true;
  }

  Status init() {
    struct ArrowSchema as;
    memset(&as, 0, sizeof(as));
    const int rc = stream_.get_schema(&stream_, &as);
    if (rc != 0) return stream_error(rc, "get_schema");
    Status st = schema_from_arrow(&as, &schema_);
    if (as.release) as.release(&as);
    return st;
  }

  const SchemaInfo& schema() const override { return schema_; }
  void require_columns(const std::vector<char>& needed) override { needed_ = needed; }
  void explain(std::string* out, int depth) const override {
    int n = 0;
    for (size_t i = 0; i < schema_.fields.size(); ++i) n += (needed_.empty() || needed_[i]) ? 1 : 0;
    explain_line(out, depth, strfmt("HostStream: host Arrow batches, %d of %d columns uploaded per batch (%s%s)", n, (int)schema_.fields.size(),
                                    mode() == 1 ? "pinned staging ring filled by library threads, DMA on a copy stream" :
                                    mode() >= 2 ? "one batch ahead, own copy stream" : "in order on the library's stream",
                                    mode() == 3 ? ", large buffers page-locked in place" : ""));
  }

  Status next(DeviceBatch* out, bool* has) override {
    *has = false;
    DFX_RETURN_IF_ERROR(ensure_init());
    if (!opts_set_) {  // no operator above brought its own option set: the process defaults
      hopt_ = host_stream_options_of(agg_options());
      opts_set_ = true;
    }
    switch (mode()) {
      case 0: return next_in_order(out, has);
      case 1: return next_staged(out, has);
      default: return next_one_ahead(out, has);
    }
  }

 private:
  struct InFlight {
    bool valid = false;
    struct ArrowArray arr;        // the producer's batch, borrowed until `event` fires
    DeviceBatch batch;
    hipEvent_t event = nullptr;
    std::vector<void*> registered;  // host ranges page-locked for this batch
    Status upload, error;
    InFlight() { memset(&arr, 0, sizeof(arr)); }
  };
  struct Piece {
    const uint8_t* host;
    uint8_t* dev;
    size_t bytes;
  };
  // how the bytes of one batch move: what upload() / h2d() are told instead of finding it in the object
  struct Transport {
    hipStream_t stream;  // the copies are queued here
    bool list_pieces;    // staged form: h2d only lists what has to travel, run_pieces moves it
    bool pin_in_place;   // host.stream = 3: the producer's large buffers are page-locked before their copy
  };

  // host.stream = 0, the default: a batch is copied on the library's own stream when it is asked for, the producer's array
  // is released when the stream has passed the copies (one synchronisation per batch).  HIP copies large pageable buffers by
  // pinning them chunk-wise inside the runtime: 53-54 GB/s here = 0.85 of the link, which is what this path delivers end to end.
  Status next_in_order(DeviceBatch* out, bool* has) {
    started_ = true;
    InFlight f;
    Status st = pull(&f, Transport{ctx().stream, false, false}, /*fence=*/false);
    if (!st.ok() || !f.valid) {
      drop(&f);
      return st;
    }
    st = f.upload;
    {  // host buffers are borrowed until here -- also when upload failed part-way: earlier columns' copies may be queued
      hipError_t e = hipStreamSynchronize(ctx().stream);
      if (e != hipSuccess && st.ok()) st = Status::Err(DFX_EXECUTION_ERROR, strfmt("HIP error %s after H2D", hipGetErrorString(e)));
    }
    return deliver(&f, st, out, has);
  }

  // host.stream = 2: batch i + 1 is pulled from the producer and copied on a stream of its own while the consumer works on
  // batch i, the producer's array released on the copy's event (no synchronisation of the compute stream).  Not the default:
  // 40-43 GB/s end to end against 53 for the in-order form (tools/host_stream_probe.py) -- a pageable copy blocks the calling
  // thread whichever stream it is queued on, so nothing overlaps, and the second stream costs the runtime's pinned-chunk
  // pipeline its rhythm.
  // host.stream = 3: the same, with the producer's large buffers page-locked in place (hipHostRegister) so that the DMA engine
  // reads them directly.  Measured end to end it LOSES as well (bench.py host_streamed_pcie_inclusive: 40-46 GB/s against 53-54
  // for HIP's own staged copy of pageable memory) although the copy out of registered memory alone is faster (57 GB/s,
  // tools/pin_probe.py) -- locking 256 MB costs 2.2 ms of the 4.7 ms its transfer takes, and it does not overlap the
  // transfer of the batch before.
  Status next_one_ahead(DeviceBatch* out, bool* has) {
    if (!copy_stream_) DFX_HIP(hipStreamCreateWithFlags(&copy_stream_, hipStreamNonBlocking));
    if (!started_) {  // the first batch: nothing to overlap it with yet
      started_ = true;
      DFX_RETURN_IF_ERROR(pull_ahead(&pending_));
    }
    if (!pending_.valid) {
      Status st = pending_.error;  // an error met while prefetching surfaces when ITS batch is asked for
      pending_.error = Status::OK();
      return st;
    }
    InFlight cur;
    std::swap(cur, pending_);
    Status ahead = pull_ahead(&pending_);  // queue the NEXT batch's copies behind this one's before waiting
    if (!ahead.ok()) {
      drop(&pending_);
      pending_.error = ahead;
    }
    Status st = cur.upload;
    if (cur.event) {  // the copies of this batch have read the producer's buffers: only now may they be released
      hipError_t e = hipEventSynchronize(cur.event);
      if (e != hipSuccess && st.ok()) st = Status::Err(DFX_EXECUTION_ERROR, strfmt("HIP error %s after H2D", hipGetErrorString(e)));
    }
    return deliver(&cur, st, out, has);
  }
  // pull() onto the copy stream, then the batch's copy event: the consumer's kernels wait for it, so does the release
  Status pull_ahead(InFlight* f) {
    DFX_RETURN_IF_ERROR(pull(f, Transport{copy_stream_, false, mode() == 3}, /*fence=*/true));
    if (!f->valid) return Status::OK();
    hipError_t e = hipEventCreateWithFlags(&f->event, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(f->event, copy_stream_);
    if (e != hipSuccess && f->upload.ok()) f->upload = Status::Err(DFX_EXECUTION_ERROR, strfmt("HIP error %s after H2D", hipGetErrorString(e)));
    // the consumer's kernels run on the library's stream: they start when the copies have landed
    if (f->event) (void)hipStreamWaitEvent(ctx().stream, f->event, 0);
    return Status::OK();
  }

  // The staged form (host.stream = 1; NOT the default: measured slower than HIP's own pageable copy on this platform, see
  // HostStreamOptions).  The DMA engine reads PINNED host memory at 57 GB/s and pageable memory not at all: HIP's own
  // copy of a pageable buffer pins it chunk-wise inside the runtime (53-54 GB/s, the calling thread blocked throughout), locking
  // the producer's pages in place costs half the transfer's time (tools/pin_probe.py).  Here the library owns a ring of pinned
  // slots; `threads` library threads copy the producer's buffers into slots piece by piece (one thread fills at ~29 GB/s: it
  // takes two to four to outrun the engine) and queue each slot's DMA on a copy stream as soon as it is full, so the engine
  // drains slot i while slots i + 1 ... are being filled.  The producer's buffers are read by those memcpys only: the array
  // is released when the threads have joined, with the last slots still crossing the link; the consumer's kernels wait for
  // the batch's copy event on the library's stream -- no host synchronisation at all.
  Status next_staged(DeviceBatch* out, bool* has) {
    started_ = true;
    if (!copy_stream_) DFX_HIP(hipStreamCreateWithFlags(&copy_stream_, hipStreamNonBlocking));
    InFlight f;
    pieces_.clear();
    Status st = pull(&f, Transport{copy_stream_, true, false}, /*fence=*/true);
    if (!st.ok() || !f.valid) {
      drop(&f);
      return st;
    }
    st = f.upload;
    if (st.ok()) st = run_pieces();
    hipError_t e = hipSuccess;
    if (st.ok()) {  // the consumer's kernels (library stream) start when this batch's last piece has landed
      if (!batch_event_) e = hipEventCreateWithFlags(&batch_event_, hipEventDisableTiming);
      if (e == hipSuccess) e = hipEventRecord(batch_event_, copy_stream_);
      if (e == hipSuccess) e = hipStreamWaitEvent(ctx().stream, batch_event_, 0);
      if (e != hipSuccess) st = Status::Err(DFX_EXECUTION_ERROR, strfmt("HIP error %s after H2D", hipGetErrorString(e)));
    } else {
      (void)hipStreamSynchronize(copy_stream_);  // pieces already queued read pinned slots, not the producer: nothing else to wait for
    }
    return deliver(&f, st, out, has);  // every byte of the producer's buffers has been copied out by now
  }
  Status ensure_ring() {
    const size_t piece = (size_t)std::max(1, hopt_.piece_mb) << 20;
    const int slots = std::max(2, std::min(64, hopt_.slots));
    if (ring_ && ring_piece_ == piece && (int)slot_event_.size() == slots) return Status::OK();
    if (copy_stream_) (void)hipStreamSynchronize(copy_stream_);
    Status st;
    ring_ = pinned_alloc(piece * (size_t)slots, &st);
    if (!ring_) return st;
    ring_piece_ = piece;
    for (hipEvent_t e : slot_event_)
      if (e) (void)hipEventDestroy(e);
    slot_event_.assign((size_t)slots, nullptr);
    for (auto& e : slot_event_) DFX_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    slot_gen_.assign((size_t)slots, 0);
    return Status::OK();
  }
  Status run_pieces() {
    if (pieces_.empty()) return Status::OK();
    DFX_RETURN_IF_ERROR(ensure_ring());
    const size_t n = pieces_.size(), R = slot_event_.size();
    size_t total = 0;
    for (const Piece& p : pieces_) total += p.bytes;
    std::fill(slot_gen_.begin(), slot_gen_.end(), 0);
    std::atomic<size_t> next{0};
    std::mutex mu;
    std::condition_variable cv;
    Status first_error = Status::OK();
    const int device = ctx().device;
    uint8_t* const ring = (uint8_t*)ring_.get();
    auto worker = [&]() {
      (void)hipSetDevice(device);  // (the current device is a per-thread setting)
      for (;;) {
        const size_t i = next.fetch_add(1);
        if (i >= n) break;
        const size_t sl = i % R, turn = i / R;
        {  // my slot's previous occupant (piece i - R, taken earlier by some thread) has been queued ...
          std::unique_lock<std::mutex> lk(mu);
          cv.wait(lk, [&] { return slot_gen_[sl] == turn; });
        }
        hipError_t e = hipSuccess;
        if (slot_used_ || turn > 0) e = hipEventSynchronize(slot_event_[sl]);  // ... and has left the slot
        const Piece& p = pieces_[i];
        if (e == hipSuccess) {
          memcpy(ring + sl * ring_piece_, p.host, p.bytes);
          e = hipMemcpyAsync(p.dev, ring + sl * ring_piece_, p.bytes, hipMemcpyHostToDevice, copy_stream_);
        }
        if (e == hipSuccess) e = hipEventRecord(slot_event_[sl], copy_stream_);
        {
          std::lock_guard<std::mutex> lk(mu);
          if (e != hipSuccess && first_error.ok()) first_error = Status::Err(DFX_EXECUTION_ERROR, strfmt("HIP error %s in the staged H2D copy", hipGetErrorString(e)));
          slot_gen_[sl] = turn + 1;
        }
        cv.notify_all();
      }
    };
    // small batches (the reference's 1024-row batches): the calling thread alone -- starting threads costs more than the copy
    const int threads = total < ((size_t)4 << 20) ? 1 : std::max(1, std::min(16, hopt_.threads));
    std::vector<std::thread> pool;
    for (int t = 1; t < threads; ++t) pool.emplace_back(worker);
    worker();
    for (std::thread& t : pool) t.join();
    slot_used_ = true;
    counters().h2d_staged_bytes += (long long)total;
    return first_error;
  }

  // pull one batch from the producer and queue its copies as `t` says (f->valid stays false at the end of the stream)
  Status pull(InFlight* f, const Transport& t, bool fence) {
    if (done_) return Status::OK();
    const int rc = stream_.get_next(&stream_, &f->arr);
    if (rc != 0) {
      memset(&f->arr, 0, sizeof(f->arr));
      return stream_error(rc, "get_next");
    }
    if (f->arr.release == nullptr) {  // end of stream == Ok(None)
      done_ = true;
      return Status::OK();
    }
    f->valid = true;
    if (fence) {  // (without: copies on the library's own stream, in order with everything else)
      // The device buffers of this batch come from the pool: they may have been handed back by a consumer whose kernels are
      // still queued on the library's stream.  The copies wait for everything that stream holds right now.
      if (!fence_) DFX_HIP(hipEventCreateWithFlags(&fence_, hipEventDisableTiming));
      DFX_HIP(hipEventRecord(fence_, ctx().stream));
      DFX_HIP(hipStreamWaitEvent(t.stream, fence_, 0));
    }
    f->upload = upload(f->arr, &f->batch, f, t);
    return Status::OK();
  }

  // the end of every form: the batch out, the array back to the producer -- also when `st` says the batch failed
  Status deliver(InFlight* f, Status st, DeviceBatch* out, bool* has) {
    DeviceBatch b = std::move(f->batch);
    drop(f);
    if (!st.ok()) return st;
    *out = std::move(b);
    *has = true;
    return Status::OK();
  }

  void drop(InFlight* f) {  // unpin, hand the array back to the producer
    if (f->event) {
      (void)hipEventSynchronize(f->event);
      (void)hipEventDestroy(f->event);
      f->event = nullptr;
    }
    for (void* p : f->registered) (void)hipHostUnregister(p);
    f->registered.clear();
    if (f->arr.release) f->arr.release(&f->arr);
    memset(&f->arr, 0, sizeof(f->arr));
    f->batch = DeviceBatch();
    f->valid = false;
  }

  Status stream_error(int rc, const char* what) {
    const char* m = stream_.get_last_error ? stream_.get_last_error(&stream_) : nullptr;
    // our own streams return a dfx_status; foreign producers an errno
    const int code = (rc > 0 && rc <= DFX_EXECUTION_ERROR) ? rc : DFX_IO_ERROR;
    return Status::Err(code, m ? std::string(m) : strfmt("input stream %s failed with code %d", what, rc));
  }

  Status h2d(const void* host, size_t bytes, std::shared_ptr<void>* dev, InFlight* f, const Transport& t) {
    Status st;
    *dev = device_alloc(bytes ? bytes : 8, &st);
    if (!*dev) return st;
    if (t.list_pieces) {  // staged form: only list what has to travel (run_pieces moves it)
      for (size_t at = 0; at < bytes; at += ring_piece_bytes()) {
        Piece p;
        p.host = (const uint8_t*)host + at;
        p.dev = (uint8_t*)dev->get() + at;
        p.bytes = std::min(ring_piece_bytes(), bytes - at);
        pieces_.push_back(p);
      }
      counters().h2d_bytes += (long long)bytes;
      return Status::OK();
    }
    if (t.pin_in_place && bytes >= kPinThreshold) {
      if (hipHostRegister(const_cast<void*>(host), bytes, hipHostRegisterDefault) == hipSuccess) f->registered.push_back(const_cast<void*>(host));
      else (void)hipGetLastError();  // not lockable (already registered, overlapping pages ...): the staged copy below still works
    }
    if (bytes) DFX_HIP(hipMemcpyAsync(dev->get(), host, bytes, hipMemcpyHostToDevice, t.stream));
    counters().h2d_bytes += (long long)bytes;
    return Status::OK();
  }

  Status upload(const struct ArrowArray& arr, DeviceBatch* out, InFlight* f, const Transport& t) {
    if ((size_t)arr.n_children != schema_.fields.size())
      return Status::Err(DFX_ARROW_ERROR, strfmt("batch has %lld columns, schema has %zu", (long long)arr.n_children, schema_.fields.size()));
    out->num_rows = arr.length;
    out->columns.clear();
    out->columns.resize(schema_.fields.size());
    for (size_t ci = 0; ci < schema_.fields.size(); ++ci) {
      const struct ArrowArray* c = arr.children[ci];
      const int dt = schema_.fields[ci].dtype;
      DeviceColumn& d = out->columns[ci];
      const int64_t off = arr.offset + c->offset;
      const int64_t n = arr.length;
      d.dtype = dt;
      d.length = n;
      if (ci < needed_.size() && !needed_[ci]) {  // projection push-down: never read downstream, so never crosses PCIe
        d.absent = true;
        continue;
      }
      d.bit_offset = off & 7;
      const uint8_t* validity = (c->n_buffers > 0) ? (const uint8_t*)c->buffers[0] : nullptr;
      if (validity && c->null_count != 0) {
        std::shared_ptr<void> dv;
        const int64_t b0 = off >> 3, b1 = (off + n + 7) >> 3;
        DFX_RETURN_IF_ERROR(h2d(validity + b0, (size_t)(b1 - b0), &dv, f, t));
        d.validity = (const uint8_t*)dv.get();
        d.owners.push_back(dv);
        d.null_count = c->null_count < 0 ? -1 : c->null_count;
      }
      if (dt == DFX_UTF8) {
        if (c->n_buffers < 3) return Status::Err(DFX_ARROW_ERROR, "Utf8 array without 3 buffers");
        // producers may export a zero-length string array with a null (or zero-sized) offsets buffer: offsets = {0}
        static const int32_t kZeroOffset[1] = {0};
        const bool no_offsets = c->buffers[1] == nullptr;
        if (no_offsets && n != 0) return Status::Err(DFX_ARROW_ERROR, "Utf8 array without an offsets buffer");
        const int32_t* offs = no_offsets ? kZeroOffset : (const int32_t*)c->buffers[1] + off;
        const uint8_t* data = (const uint8_t*)c->buffers[2];
        std::shared_ptr<void> doff, ddata;
        DFX_RETURN_IF_ERROR(h2d(offs, sizeof(int32_t) * (size_t)(n + 1), &doff, f, t));
        const int32_t o0 = offs[0], o1 = offs[n];
        if (o1 < o0 || (o1 > o0 && !data)) return Status::Err(DFX_ARROW_ERROR, "Utf8 array with inconsistent offsets");
        DFX_RETURN_IF_ERROR(h2d(data ? data + o0 : nullptr, (size_t)(o1 - o0), &ddata, f, t));
        d.offsets = (const int32_t*)doff.get();
        d.data = (const uint8_t*)ddata.get() - o0;  // raw offsets index straight into it
        d.data_bytes = o1 - o0;
        d.owners.push_back(doff);
        d.owners.push_back(ddata);
      } else if (dt == DFX_BOOLEAN) {
        if (c->n_buffers < 2) return Status::Err(DFX_ARROW_ERROR, "Boolean array without 2 buffers");
        std::shared_ptr<void> dv;
        const int64_t b0 = off >> 3, b1 = (off + n + 7) >> 3;
        DFX_RETURN_IF_ERROR(h2d((const uint8_t*)c->buffers[1] + b0, (size_t)(b1 - b0), &dv, f, t));
        d.values = dv.get();
        d.owners.push_back(dv);
      } else {
        if (c->n_buffers < 2) return Status::Err(DFX_ARROW_ERROR, "primitive array without 2 buffers");
        const int w = dtype_width(dt);
        std::shared_ptr<void> dv;
        DFX_RETURN_IF_ERROR(h2d((const uint8_t*)c->buffers[1] + (size_t)off * w, (size_t)n * w, &dv, f, t));
        d.values = dv.get();
        d.owners.push_back(dv);
      }
    }
    return Status::OK();
  }

  static constexpr size_t kPinThreshold = (size_t)1 << 20;  // smaller buffers: the staged copy costs less than locking pages
  HostStreamOptions hopt_;
  bool opts_set_ = false;
  int mode() const { return hopt_.mode < 0 || hopt_.mode > 3 ? 0 : hopt_.mode; }  // the one source of the form
  size_t ring_piece_bytes() const { return (size_t)std::max(1, hopt_.piece_mb) << 20; }
  // staged form
  std::vector<Piece> pieces_;
  std::shared_ptr<void> ring_;
  size_t ring_piece_ = 0;
  std::vector<hipEvent_t> slot_event_;
  std::vector<size_t> slot_gen_;
  bool slot_used_ = false;
  hipEvent_t batch_event_ = nullptr;
  struct ArrowArrayStream stream_;
  SchemaInfo schema_;
  std::vector<char> needed_;
  hipStream_t copy_stream_ = nullptr;
  hipEvent_t fence_ = nullptr;
  InFlight pending_;  // one batch ahead: the batch that is crossing PCIe while the consumer works on the one before
  bool started_ = false, done_ = false;
};

}  // namespace

Status adopt_input_stream(struct ArrowArrayStream* input, std::unique_ptr<Relation>* out) {
  if (!input || !input->release) return Status::Err(DFX_GENERAL, "input stream is null or released");
  if (peek_exported(input)) {  // one of ours: stay on the device
    *out = take_exported(input);
    return Status::OK();
  }
  std::unique_ptr<HostStreamRelation> h(new HostStreamRelation(input));
  DFX_RETURN_IF_ERROR(h->init());
  *out = std::move(h);
  return Status::OK();
}

}  // namespace dfx
