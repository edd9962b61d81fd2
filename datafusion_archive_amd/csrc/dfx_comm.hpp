// dfx_comm.hpp -- the communicator of the multi-GPU exchange and the two collectives the library builds from grouped
// ncclSend / ncclRecv (dfx_comm.cpp).  Private to dfx_comm.cpp and dfx_exchange.cpp; hosts see the opaque dfx_comm of dfx.h.
#pragma once
#include <rccl/rccl.h>

#include <memory>
#include <string>
#include <vector>

#include "dfx_exchange_plan.hpp"
#include "dfx_host.hpp"

// RCCL is bound at run time (dlopen "librccl.so.1"): the library has no link-time dependency on it, a process that has
// already loaded an RCCL (PyTorch ships one under the same soname) shares that copy, and hosts without RCCL can still
// load the library -- dfx_comm_* then fail with ExecutionError.
namespace dfx {
struct Rccl {
  void* handle = nullptr;
  std::string why;  // not empty: why there is no RCCL
  decltype(&ncclGetUniqueId) GetUniqueId = nullptr;
  decltype(&ncclCommInitRank) CommInitRank = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclCommCount) CommCount = nullptr;
  decltype(&ncclGroupStart) GroupStart = nullptr;
  decltype(&ncclGroupEnd) GroupEnd = nullptr;
  decltype(&ncclSend) Send = nullptr;
  decltype(&ncclRecv) Recv = nullptr;
  decltype(&ncclAllGather) AllGather = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
};
Rccl& rccl();

Status nccl_status(ncclResult_t rc, const char* what);
#define DFX_NCCL(call, what)                         \
  do {                                               \
    Status st__ = nccl_status((call), what);         \
    if (!st__.ok()) return st__;                     \
  } while (0)
}  // namespace dfx

struct dfx_comm {
  ncclComm_t comm = nullptr;
  int world = 1;
  int rank = 0;
  // Device words reserved when the communicator is created: everything the ranks use to tell each other how they are --
  // counts, failure marks, ready flags, the ungrouped state blocks -- lives here, so that no allocation can fail between a
  // rank's decision to take part in a collective and the collective itself.
  std::shared_ptr<void> slab;
  uint64_t* words = nullptr;
  dfx::SlabLayout at{1};  // where its regions lie
};

namespace dfx {

struct SendWords {
  const uint64_t* from;
  size_t words;
};
struct RecvWords {
  uint64_t* into;
  size_t words;
};
// all-to-all of 64-bit words on stream s: send[peer] goes to peer, recv[peer] comes from it; peer == rank is a device-to-device copy.
// t_out / t_in (may be null): one TRAILER word more per peer -- t_out[peer] travels behind the bucket, lands in t_in[peer]
Status all_to_all_words(dfx_comm* c, const std::vector<SendWords>& send, const std::vector<RecvWords>& recv, hipStream_t s,
                        const uint64_t* t_out = nullptr, uint64_t* t_in = nullptr);

// every rank's variable-sized blob to every rank: `mine` (device, sizes[rank] words) lands in `all` behind the blobs of the
// lower ranks.  sizes[] (words per rank) is known to everybody beforehand.  Grouped sends / receives like the all-to-all.
Status all_gather_v_words(dfx_comm* c, const uint64_t* mine, const std::vector<uint64_t>& sizes, uint64_t* all, hipStream_t s);

}  // namespace dfx
