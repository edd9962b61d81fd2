// dfx_comm.cpp -- the communicator of the multi-GPU exchange (include/dfx.h: dfx_comm_*): the run-time binding of RCCL, the
// slab of device words the ranks talk over, and the two collectives the exchange (dfx_exchange.cpp) is made of beyond
// ncclAllGather -- an all-to-all and a variable-size all-gather of 64-bit words, both grouped ncclSend / ncclRecv.
#include "dfx_comm.hpp"

#include <dlfcn.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>

namespace dfx {

Rccl& rccl() {
  static Rccl r;
  static std::once_flag once;
  std::call_once(once, [] {
    // DFX_RCCL_LIB: bind this library instead (a differently named RCCL build; the tests' host-staged stand-in that lets
    // several ranks share one GPU, tests/native/rccl_stub.cpp)
    const char* override_lib = getenv("DFX_RCCL_LIB");
    const char* names[] = {override_lib, "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    for (const char* n : names) {
      if (!n || !*n) continue;
      r.handle = dlopen(n, RTLD_NOW | (n == override_lib ? RTLD_LOCAL : RTLD_GLOBAL));
      if (r.handle || n == override_lib) break;  // an override that does not load is an error, not a reason to look elsewhere
    }
    if (!r.handle) {
      const char* e = dlerror();
      r.why = std::string("RCCL is not available (dlopen librccl.so.1: ") + (e ? e : "?") + ")";
      return;
    }
#define DFX_SYM(field, name)                                                      \
  r.field = (decltype(r.field))dlsym(r.handle, name);                             \
  if (!r.field && r.why.empty()) r.why = std::string("RCCL lacks the symbol ") + name;
    DFX_SYM(GetUniqueId, "ncclGetUniqueId")
    DFX_SYM(CommInitRank, "ncclCommInitRank")
    DFX_SYM(CommDestroy, "ncclCommDestroy")
    DFX_SYM(CommCount, "ncclCommCount")
    DFX_SYM(GroupStart, "ncclGroupStart")
    DFX_SYM(GroupEnd, "ncclGroupEnd")
    DFX_SYM(Send, "ncclSend")
    DFX_SYM(Recv, "ncclRecv")
    DFX_SYM(AllGather, "ncclAllGather")
    DFX_SYM(GetErrorString, "ncclGetErrorString")
#undef DFX_SYM
  });
  return r;
}

Status nccl_status(ncclResult_t rc, const char* what) {
  if (rc == ncclSuccess) return Status::OK();
  Rccl& r = rccl();
  return Status::Err(DFX_EXECUTION_ERROR, strfmt("RCCL %s failed: %s", what, r.GetErrorString ? r.GetErrorString(rc) : "?"));
}

Status all_to_all_words(dfx_comm* c, const std::vector<SendWords>& send, const std::vector<RecvWords>& recv, hipStream_t s, const uint64_t* t_out,
                        uint64_t* t_in) {
  Rccl& r = rccl();
  if (c->world > 1) DFX_NCCL(r.GroupStart(), "ncclGroupStart");
  Status st = Status::OK();
  for (int peer = 0; peer < c->world && st.ok(); ++peer) {
    const uint64_t* sp = send[(size_t)peer].from;
    uint64_t* rp = recv[(size_t)peer].into;
    const size_t sn = send[(size_t)peer].words, rn = recv[(size_t)peer].words;
    if (peer == c->rank) {
      if (sn != rn) st = Status::Err(DFX_INTERNAL_ERROR, "exchange: a rank's own bucket changed size");
      else if (sn) {
        hipError_t e = hipMemcpyAsync(rp, sp, sn * sizeof(uint64_t), hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) st = Status::Err(DFX_EXECUTION_ERROR, strfmt("HIP error %s in the exchange", hipGetErrorString(e)));
      }
      if (st.ok() && t_out) {
        hipError_t e = hipMemcpyAsync(t_in + peer, t_out + peer, sizeof(uint64_t), hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) st = Status::Err(DFX_EXECUTION_ERROR, strfmt("HIP error %s in the exchange", hipGetErrorString(e)));
      }
      continue;
    }
    if (sn) st = nccl_status(r.Send(sp, sn, ncclUint64, peer, c->comm, s), "ncclSend");
    if (st.ok() && t_out) st = nccl_status(r.Send(t_out + peer, 1, ncclUint64, peer, c->comm, s), "ncclSend");
    if (st.ok() && rn) st = nccl_status(r.Recv(rp, rn, ncclUint64, peer, c->comm, s), "ncclRecv");
    if (st.ok() && t_in) st = nccl_status(r.Recv(t_in + peer, 1, ncclUint64, peer, c->comm, s), "ncclRecv");
  }
  if (c->world > 1) {
    Status ge = nccl_status(r.GroupEnd(), "ncclGroupEnd");
    if (st.ok()) st = ge;
  }
  return st;
}

Status all_gather_v_words(dfx_comm* c, const uint64_t* mine, const std::vector<uint64_t>& sizes, uint64_t* all, hipStream_t s) {
  std::vector<SendWords> send((size_t)c->world);
  std::vector<RecvWords> recv((size_t)c->world);
  uint64_t base = 0;
  for (int r = 0; r < c->world; ++r) {
    send[(size_t)r] = {mine, (size_t)sizes[(size_t)c->rank]};
    recv[(size_t)r] = {all + base, (size_t)sizes[(size_t)r]};
    base += sizes[(size_t)r];
  }
  return all_to_all_words(c, send, recv, s);
}

}  // namespace dfx

using namespace dfx;

extern "C" {

int32_t dfx_comm_unique_id(uint8_t* id, char* err, size_t errlen) {
  return c_abi_guard(err, errlen, [&]() -> int32_t {
    if (!id) return to_c(Status::Err(DFX_GENERAL, "null argument"), err, errlen);
    Rccl& r = rccl();
    if (!r.why.empty()) return to_c(Status::Err(DFX_EXECUTION_ERROR, r.why), err, errlen);
    static_assert(sizeof(ncclUniqueId) == DFX_COMM_ID_BYTES, "ncclUniqueId size");
    ncclUniqueId u;
    Status st = nccl_status(r.GetUniqueId(&u), "ncclGetUniqueId");
    if (st.ok()) memcpy(id, &u, sizeof(u));
    return to_c(st, err, errlen);
  });
}

int32_t dfx_comm_init(const uint8_t* id, int32_t world, int32_t rank, dfx_comm** out, char* err, size_t errlen) {
  return c_abi_guard(err, errlen, [&]() -> int32_t {
    if (!id || !out) return to_c(Status::Err(DFX_GENERAL, "null argument"), err, errlen);
    if (world < 1 || world > 1024 || rank < 0 || rank >= world) return to_c(Status::Err(DFX_GENERAL, "bad world / rank"), err, errlen);
    Status st = ensure_init();  // the library's device is the communicator's device
    if (!st.ok()) return to_c(st, err, errlen);
    Rccl& r = rccl();
    if (!r.why.empty()) return to_c(Status::Err(DFX_EXECUTION_ERROR, r.why), err, errlen);
    ncclUniqueId u;
    memcpy(&u, id, sizeof(u));
    std::unique_ptr<dfx_comm> c(new dfx_comm());
    c->world = world;
    c->rank = rank;
    c->at = SlabLayout(world);
    {  // ncclCommInitRank binds the communicator to the calling thread's CURRENT device
      hipError_t e = hipSetDevice(ctx().device);
      if (e != hipSuccess) return to_c(Status::Err(DFX_EXECUTION_ERROR, strfmt("hipSetDevice(%d): %s", ctx().device, hipGetErrorString(e))), err, errlen);
    }
    // the slab first: a rank that cannot have it must not enter the collective communicator set-up half-way
    c->slab = device_alloc(sizeof(uint64_t) * c->at.total, &st);
    if (!c->slab) return to_c(st, err, errlen);
    c->words = (uint64_t*)c->slab.get();
    {
      hipError_t e = hipMemset(c->words, 0, sizeof(uint64_t) * c->at.total);
      if (e != hipSuccess) return to_c(Status::Err(DFX_EXECUTION_ERROR, strfmt("hipMemset: %s", hipGetErrorString(e))), err, errlen);
    }
    st = nccl_status(r.CommInitRank(&c->comm, world, u, rank), "ncclCommInitRank");
    if (!st.ok()) return to_c(st, err, errlen);
    *out = c.release();
    return DFX_OK;
  });
}

int32_t dfx_comm_ranks(const dfx_comm* c) {
  if (!c || !c->comm || !rccl().CommCount) return -1;
  int n = -1;
  return rccl().CommCount(c->comm, &n) == ncclSuccess ? (int32_t)n : -1;
}

void dfx_comm_destroy(dfx_comm* c) {
  if (!c) return;
  (void)hipStreamSynchronize(ctx().stream);  // nothing of this communicator is still queued on the library's stream
  if (c->comm && rccl().CommDestroy) (void)rccl().CommDestroy(c->comm);
  delete c;
}

}  // extern "C"
