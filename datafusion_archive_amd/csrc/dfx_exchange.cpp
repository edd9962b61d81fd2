// dfx_exchange.cpp -- multi-GPU GROUP BY: the exchange of group partials as ONE library call over RCCL.
//
// The reference is single-process (README.md:20); SURVEY.md section 8(e) defines the MI355X addition: every rank (one
// process per GPU) aggregates its own row range, the GROUPS (never the rows) are bucketed by hash(key) % world, every rank
// merges the buckets it owns and emits them.  dfx_aggregate_partial_{build,export,import} expose the device steps to a host
// that brings its own collective (datafusion_archive_amd/distributed.py: torch.distributed); dfx_aggregate_exchange below
// is the whole protocol inside the library, on the library's stream, over the communicator of dfx_comm.cpp.  The relation's
// half (count, scatter, merge kernels) is AggregateRelation::exchange_* / ungrouped_* in dfx_aggregate_partial.cpp; the
// arithmetic every rank must do alike is dfx_exchange_plan.hpp.
//
// Grouped, in the common case TWO collective rounds and TWO host synchronisations (exchange_grouped names the steps):
//   before   everything round 2 needs is allocated for a capacity the rank ANNOUNCES: send buffer for its own groups, receive
//            buffer and import table for twice as many (ranks that scanned row ranges of one table own about as many groups
//            as each holds) -- a rank that cannot allocate says so in round 1 instead of failing between two collectives.
//   round 1  a count kernel, then ONE ncclAllGather of world + 3 words per rank: {state word: how the rank is | the shape of
//            what it exchanges, receive capacity, send capacity, its group count per owner rank}.  ONE read-back: every rank
//            holds the whole count matrix and every rank's state -- the agreement, the counts and the buffer sizes in one.
//   (extra)  only if some rank receives or holds more than it announced -- every rank computes that from the same matrix, so
//            all take this branch or none does: allocate again, agree() on the outcome (one round, one read-back more).
//   round 2  the buckets as grouped ncclSend / ncclRecv, once per chunk of accumulator planes (more than kMaxAggs
//            accumulators), merged on the same stream.  The LAST chunk's message to every peer carries one trailer word:
//            how the sender was when it sent.  ONE synchronisation reads the trailers and the new table's control block.
//            There is no closing agreement: what a rank does after its last collective can only fail that rank.
// Utf8 keys put an agree() and the rounds of globalise_dictionaries in front (dictionary ids are rank-local).
// Ungrouped aggregates (one row per rank): agree(), an ncclAllGather of the state block per chunk, agree().
#include <string.h>

#include <algorithm>
#include <string>
#include <unordered_map>
#include <vector>

#include "dfx_comm.hpp"
#include "dfx_relation.hpp"

namespace dfx {

static_assert(kUngroupedStateWords == 2 * (size_t)kMaxAggs, "the slab's ungrouped state blocks hold 2 words per accumulator slot");

// test hook (tests/test_gpu_exchange_world2.py): the process-wide switch dfx_set_option("test.exchange_fail", rank << 8 | stage)
// makes that rank fail locally at that stage (stage numbers: kFailStages below; 0 = off, the default).  A switch the host
// sets explicitly, not an environment variable the production library would consult in every exchange.
static int64_t g_exchange_fail = 0;
void set_exchange_test_failure(int64_t v) { g_exchange_fail = v; }
static const char* const kFailStages[] = {"", "drain", "count", "payload_alloc", "export", "dict_local", "dict_blob_alloc", "merge"};
static bool inject_failure(const dfx_comm* c, const char* stage) {
  const int64_t v = g_exchange_fail;
  if (v <= 0) return false;
  const int st = (int)(v & 0xFF);
  return st > 0 && st < (int)(sizeof(kFailStages) / sizeof(kFailStages[0])) && (int)(v >> 8) == c->rank && !strcmp(kFailStages[st], stage);
}
static Status injected(const dfx_comm* c, const char* stage) {
  return inject_failure(c, stage) ? Status::Err(DFX_EXECUTION_ERROR, strfmt("injected failure at stage '%s' (test.exchange_fail)", stage)) : Status::OK();
}
static Status hip_local(hipError_t e) {
  return e == hipSuccess ? Status::OK() : Status::Err(DFX_EXECUTION_ERROR, strfmt("HIP error %s in the exchange", hipGetErrorString(e)));
}

// THE read-back: copy to the host, synchronise the stream (also when the copy failed), the first failure of the two.
// Callers between two collectives fold the result into their `local`; see THE rule below.
static Status read_back(uint64_t* host, const uint64_t* device, size_t words, hipStream_t s) {
  Status rb = hip_local(hipMemcpyAsync(host, device, sizeof(uint64_t) * words, hipMemcpyDeviceToHost, s));
  Status sy = hip_local(hipStreamSynchronize(s));
  return rb.ok() ? sy : rb;
}

// what the peers said, as this rank's error
static Status peer_error(const PeerCheck& p, const char* failed_when) {
  switch (p.verdict) {
    case PeerVerdict::Failed:
      return Status::Err(DFX_EXECUTION_ERROR, strfmt("multi-GPU exchange: rank %d failed %s", p.rank, failed_when));
    case PeerVerdict::Differs:
      return Status::Err(DFX_EXECUTION_ERROR,
                         strfmt("multi-GPU exchange: rank %d is exchanging a different query (keys / accumulator chunks / dictionaries)", p.rank));
    case PeerVerdict::Ok: break;
  }
  return Status::OK();
}

// THE rule of this file: between its first and its last collective a rank never returns on a LOCAL failure.  It folds the
// failure into `local`, goes on taking part in every collective with well-formed (if meaningless) messages, and all ranks
// leave together at the next agree(): every rank tells every rank whether it is still well -- one word per peer over the
// reserved slab -- plus a word describing what it is about to exchange (`shape`: keys, chunks, dictionaries ...), so ranks
// whose queries differ (one of them carries a deferred set-up error, say) find out instead of waiting for each other.
// Returns the rank's own error if it has one, else "rank r failed <what>" / "ranks disagree", else OK -- the same verdict
// (ok or not) on every rank.  (A collective that itself fails inside RCCL is RCCL's to report: nothing to agree over.)
static Status agree(dfx_comm* c, const Status& local, uint64_t shape, const char* what, int64_t* host_syncs, hipStream_t s) {
  if (c->world <= 1) return local;
  const int W = c->world;
  const uint64_t word = rank_state_word(local.ok(), shape);
  std::vector<uint64_t> hf((size_t)W * 2, 0);
  for (int r = 0; r < W; ++r) hf[(size_t)r] = word;
  uint64_t* d = c->words + c->at.flags;
  // a local HIP failure here does not excuse this rank from the round: its peers are already waiting in it.  It takes part
  // with whatever the slab holds (a stale word at worst: the peers then disagree on the shape and leave as well) and
  // reports its own error afterwards.
  Status mine = local;
  {
    Status cp = hip_local(hipMemcpyAsync(d, hf.data(), sizeof(uint64_t) * hf.size(), hipMemcpyHostToDevice, s));
    if (!cp.ok()) (void)hipStreamSynchronize(s);
    if (mine.ok()) mine = cp;
  }
  std::vector<SendWords> send((size_t)W);
  std::vector<RecvWords> recv((size_t)W);
  for (int peer = 0; peer < W; ++peer) {
    send[(size_t)peer] = {d + peer, 1};
    recv[(size_t)peer] = {d + W + peer, 1};
  }
  Status coll = all_to_all_words(c, send, recv, s);
  if (!coll.ok()) return mine.ok() ? coll : mine;  // (a collective that fails inside RCCL is RCCL's to report)
  {
    Status rb = read_back(hf.data(), d, hf.size(), s);
    if (mine.ok()) mine = rb;
  }
  ++*host_syncs;
  if (!mine.ok()) return mine;
  return peer_error(check_peers(hf.data() + W, W, word), what);
}

// the same global dictionary on every rank: rank 0's strings in id order, then rank 1's new ones, ...  `remap`: this rank's
// local id -> global id.  sizes[3 r], sizes[3 r + 1]: rank r's strings and bytes; its blob (lens as u32 padded to words,
// then the bytes) begins at blobs[base[r]], except this rank's own, which is read from lens / pool.
struct GlobalDictionary {
  std::vector<uint32_t> lens;
  std::vector<uint8_t> pool;
  std::vector<uint64_t> remap;
};
static Status build_global_dictionary(int world, int rank, const std::vector<uint64_t>& sizes, const std::vector<uint64_t>& base,
                                      const std::vector<uint64_t>& blobs, const std::vector<uint32_t>& lens, const std::vector<uint8_t>& pool,
                                      GlobalDictionary* g) {
  std::unordered_map<std::string, uint64_t> ids;
  for (int r = 0; r < world; ++r) {
    const uint64_t n_ids = sizes[(size_t)r * 3], n_bytes = sizes[(size_t)r * 3 + 1];
    const uint32_t* rl = r == rank ? lens.data() : (const uint32_t*)(blobs.data() + base[(size_t)r]);
    const uint8_t* rp = r == rank ? pool.data() : (const uint8_t*)(blobs.data() + base[(size_t)r] + (n_ids + 1) / 2);
    uint64_t at = 0;
    for (uint64_t i = 0; i < n_ids; ++i) {
      if (at + rl[i] > n_bytes) return Status::Err(DFX_INTERNAL_ERROR, "multi-GPU exchange: malformed dictionary blob");
      std::string str((const char*)rp + at, (size_t)rl[i]);
      at += rl[i];
      auto ins = ids.emplace(std::move(str), (uint64_t)g->lens.size());
      if (ins.second) {
        g->lens.push_back(rl[i]);
        g->pool.insert(g->pool.end(), (const uint8_t*)ins.first->first.data(), (const uint8_t*)ins.first->first.data() + ins.first->first.size());
      }
      if (r == rank) g->remap.push_back(ins.first->second);
    }
  }
  return Status::OK();
}

// Utf8 GROUP BY keys: dictionary ids are rank-local.  Every rank learns every rank's strings (sizes first, then lengths +
// bytes), builds the SAME global dictionary on the host, rewrites its key plane to global ids and installs the global
// dictionary for the emit.  O(distinct strings of all ranks) on the host.
// Aligned on every rank: per dictionary a sizes round (carrying the failure mark), an agree() after the blob buffers were
// allocated, the blob round, an agree() after the host-side build.  Returns the same verdict on every rank.
static Status globalise_dictionaries(AggregateRelation* a, dfx_comm* c, int64_t* host_syncs) {
  const int world = c->world;
  hipStream_t s = ctx().stream;
  Status local = Status::OK();
  for (int d = 0; d < a->exchange_dicts(); ++d) {
    std::vector<uint32_t> lens;
    std::vector<uint8_t> pool;
    if (local.ok()) local = a->exchange_dict_local(d, &lens, &pool);
    if (local.ok()) local = injected(c, "dict_local");
    if (!local.ok()) { lens.clear(); pool.clear(); }
    // blob = lens (u32, padded to words) + bytes (padded to words)
    const uint64_t len_words = ((uint64_t)lens.size() + 1) / 2, pool_words = ((uint64_t)pool.size() + 7) / 8;
    uint64_t hmine[3] = {local.ok() ? (uint64_t)lens.size() : kPeerFailed, (uint64_t)pool.size(), 0};
    uint64_t* dmine = c->words + c->at.dict_mine;
    uint64_t* dall = c->words + c->at.dict_all;
    DFX_HIP(hipMemcpyAsync(dmine, hmine, sizeof(hmine), hipMemcpyHostToDevice, s));  // (breaks THE rule: leaves before the sizes round on a local HIP error)
    std::vector<uint64_t> three((size_t)world, 3);
    DFX_RETURN_IF_ERROR(all_gather_v_words(c, dmine, three, dall, s));
    std::vector<uint64_t> hall((size_t)world * 3, 0);
    DFX_RETURN_IF_ERROR(read_back(hall.data(), dall, hall.size(), s));  // (breaks THE rule: leaves between the sizes round and the agree())
    ++*host_syncs;
    hall[(size_t)c->rank * 3] = hmine[0];
    hall[(size_t)c->rank * 3 + 1] = hmine[1];
    if (const int failed = first_failed_rank(hall.data(), world, 3); failed >= 0)
      return local.ok() ? peer_error({PeerVerdict::Failed, failed}, "before the exchange") : local;
    std::vector<uint64_t> sizes((size_t)world), base((size_t)world + 1, 0);
    for (int r = 0; r < world; ++r) {
      sizes[(size_t)r] = (hall[(size_t)r * 3] + 1) / 2 + (hall[(size_t)r * 3 + 1] + 7) / 8;
      base[(size_t)r + 1] = base[(size_t)r] + sizes[(size_t)r];
    }
    std::vector<uint64_t> blob((size_t)std::max<uint64_t>(1, len_words + pool_words), 0);
    if (!lens.empty()) memcpy(blob.data(), lens.data(), sizeof(uint32_t) * lens.size());
    if (!pool.empty()) memcpy(blob.data() + len_words, pool.data(), pool.size());
    // the blob buffers: allocated before the ranks commit themselves to the blob round
    Status st;
    auto dblob = device_alloc(sizeof(uint64_t) * blob.size(), &st);
    std::shared_ptr<void> dblobs;
    if (dblob) dblobs = device_alloc(sizeof(uint64_t) * (size_t)std::max<uint64_t>(1, base[(size_t)world]), &st);
    if (!dblob || !dblobs) local = st;
    if (local.ok()) local = injected(c, "dict_blob_alloc");
    if (local.ok()) local = hip_local(hipMemcpyAsync(dblob.get(), blob.data(), sizeof(uint64_t) * blob.size(), hipMemcpyHostToDevice, s));
    DFX_RETURN_IF_ERROR(agree(c, local, (uint64_t)d, "while it prepared its dictionary", host_syncs, s));
    DFX_RETURN_IF_ERROR(all_gather_v_words(c, (const uint64_t*)dblob.get(), sizes, (uint64_t*)dblobs.get(), s));
    std::vector<uint64_t> blobs((size_t)std::max<uint64_t>(1, base[(size_t)world]), 0);
    DFX_RETURN_IF_ERROR(read_back(blobs.data(), (const uint64_t*)dblobs.get(), blobs.size(), s));  // (breaks THE rule: leaves between the blob round and the agree())
    ++*host_syncs;
    GlobalDictionary g;
    local = build_global_dictionary(world, c->rank, hall, base, blobs, lens, pool, &g);
    if (local.ok()) local = a->exchange_dict_globalise(d, g.lens, g.pool, g.remap);
    DFX_RETURN_IF_ERROR(agree(c, local, (uint64_t)d, "while it installed the global dictionary", host_syncs, s));
  }
  return Status::OK();
}

// ---- ungrouped: one row per rank.  All-gather the accumulator states, fold them with the aggregates' algebra ---------------
// (never adds to xchg_rounds / xchg_host_syncs: those count the grouped form)
static Status exchange_ungrouped(AggregateRelation* a, dfx_comm* c, int64_t* stats, long long t_begin) {
  const int world = c->world;
  hipStream_t s = ctx().stream;
  int64_t host_syncs = 0;
  Status local = a->ungrouped_state_begin();  // (drains the input: DivideByZero, out of memory ...)
  if (local.ok()) local = hip_local(hipStreamSynchronize(s));
  const long long t_local = ScopedUs::now();
  counters().xchg_local_us += t_local - t_begin;
  if (local.ok()) local = injected(c, "drain");
  const int nw = a->ungrouped_state_words();
  const int n_chunks = a->exchange_chunks();
  {
    Status ag = agree(c, local, 0x100ull | ((uint64_t)n_chunks << 16) | ((uint64_t)nw << 24), "before the exchange", &host_syncs, s);
    counters().xchg_wait_peers_us += ScopedUs::now() - t_local;
    DFX_RETURN_IF_ERROR(ag);
  }
  ScopedUs t_rest(&counters().xchg_exchange_us);
  if (nw > (int)kUngroupedStateWords) return Status::Err(DFX_INTERNAL_ERROR, "exchange: ungrouped state wider than the communicator's slab");
  uint64_t* all = c->words + c->at.state_all;
  for (int ch = 0; ch < n_chunks; ++ch) {  // more than kMaxAggs accumulators: one state block per chunk
    if (local.ok()) local = a->ungrouped_select_chunk(ch);
    if (local.ok() && ch == n_chunks - 1) local = injected(c, "merge");
    const void* mine = a->ungrouped_state_device();
    if (!local.ok() || !mine) mine = c->words + c->at.state_mine;  // (something well-formed to send: every rank gives up at the agree() below)
    if (world > 1) {
      DFX_NCCL(rccl().AllGather(mine, all, (size_t)nw, ncclUint64, c->comm, s), "ncclAllGather");
    } else {
      Status cp = hip_local(hipMemcpyAsync(all, mine, sizeof(uint64_t) * (size_t)nw, hipMemcpyDeviceToDevice, s));
      if (local.ok()) local = cp;
    }
    // (a local HIP failure is folded into `local`: the peers are about to enter the next chunk's all-gather and the
    // agree() behind the loop -- this rank goes with them)
    std::vector<uint64_t> host((size_t)nw * (size_t)world);
    {
      Status rb = read_back(host.data(), all, host.size(), s);
      if (local.ok()) local = rb;
    }
    ++host_syncs;
    if (local.ok()) local = a->ungrouped_state_merge(host.data(), world, c->rank);
  }
  if (local.ok()) local = a->ungrouped_select_chunk(0);
  DFX_RETURN_IF_ERROR(agree(c, local, 0x101ull, "while it merged the ranks' states", &host_syncs, s));
  if (stats) {
    stats[0] = stats[1] = 1;
    stats[2] = (int64_t)(sizeof(uint64_t) * (size_t)nw * (size_t)n_chunks);
    stats[3] = host_syncs;
  }
  return Status::OK();
}

// ---- grouped --------------------------------------------------------------------------------------------------------------
// what the steps of exchange_grouped share
struct GroupedExchange {
  AggregateRelation* a = nullptr;
  dfx_comm* c = nullptr;
  hipStream_t s = nullptr;
  Status local;  // this rank's first local failure (THE rule)
  int n_chunks = 0;
  int widest = 0;      // words of the widest chunk's rows: the payload buffers serve every chunk
  uint64_t shape = 0;  // what this rank is about to exchange, for its state word
  uint64_t send_cap = 0, recv_cap = 0;  // groups the payload buffers (and the import table) have room for
  std::shared_ptr<void> send, recv;
  int64_t rounds = 0, host_syncs = 0;
};

static std::shared_ptr<void> alloc_payload(const GroupedExchange& x, uint64_t groups, Status* st) {
  return device_alloc(sizeof(uint64_t) * (size_t)payload_buffer_words(groups, x.widest, x.c->world), st);
}

static void drain_and_synchronise(GroupedExchange& x) {
  x.local = x.a->exchange_drain();
  if (x.local.ok()) x.local = hip_local(hipStreamSynchronize(x.s));
}

static void describe_query(GroupedExchange& x) {
  x.n_chunks = x.a->exchange_chunks();
  x.shape = 0x200ull | ((uint64_t)x.n_chunks << 12) | ((uint64_t)x.a->exchange_dicts() << 20);
  for (int ch = 0; ch < x.n_chunks; ++ch) {
    x.widest = std::max(x.widest, x.a->exchange_chunk_words(ch));
    x.shape = x.shape * 31 + (uint64_t)x.a->exchange_chunk_words(ch);
  }
  x.shape &= 0xFFFFFFFFFFFFull;
}

// Utf8 keys: the dictionaries are globalised first (rounds of their own: sizes, blobs, agreements); a rank that failed its
// drain must not enter them, so this form keeps an agreement in front
static Status agree_and_globalise_dictionaries(GroupedExchange& x) {
  Status ag = agree(x.c, x.local, x.shape, "before the exchange", &x.host_syncs, x.s);
  ++x.rounds;
  DFX_RETURN_IF_ERROR(ag);
  return globalise_dictionaries(x.a, x.c, &x.host_syncs);
}

// everything the payload round needs, before anybody commits to it
static void allocate_for_announced_capacity(GroupedExchange& x) {
  const uint64_t own_groups = x.local.ok() ? x.a->exchange_group_bound() : 0;  // (what the host knows; the count kernel has the last word)
  x.send_cap = own_groups + 64;
  x.recv_cap = 2 * own_groups + 4096;
  if (x.local.ok()) {
    Status st;
    x.send = alloc_payload(x, x.send_cap, &st);
    if (x.send) x.recv = alloc_payload(x, x.recv_cap, &st);
    if (!x.send || !x.recv) x.local = st;
  }
  if (x.local.ok()) x.local = injected(x.c, "payload_alloc");
  if (x.local.ok()) x.local = x.a->exchange_import_begin(x.recv_cap);
}

// round 1: count, fill the header, all-gather.  Returns only what RCCL reports.
static Status round1_all_gather(GroupedExchange& x) {
  const int W = x.c->world;
  uint64_t* d_mine = x.c->words + x.c->at.round1_mine;
  uint64_t* d_all = x.c->words + x.c->at.round1_all;
  if (x.local.ok()) {
    x.local = x.a->exchange_count(W, d_mine + kRound1Header);
    if (x.local.ok()) x.local = injected(x.c, "count");
  }
  if (!x.local.ok()) {  // a rank that is not well sends zeros behind its failure mark (its table may not even exist)
    Status z = hip_local(hipMemsetAsync(d_mine + kRound1Header, 0, sizeof(uint64_t) * (size_t)W, x.s));
    (void)z;
  }
  Status f0 = hip_local(launch_fill_u64(d_mine + kRound1State, rank_state_word(x.local.ok(), x.shape), 1, x.s));
  Status f1 = hip_local(launch_fill_u64(d_mine + kRound1RecvCap, x.recv_cap, 1, x.s));
  Status f2 = hip_local(launch_fill_u64(d_mine + kRound1SendCap, x.send_cap, 1, x.s));
  if (x.local.ok()) x.local = f0.ok() ? (f1.ok() ? f2 : f1) : f0;
  const size_t MW = Round1Matrix::message_words(W);
  if (W > 1) {
    DFX_NCCL(rccl().AllGather(d_mine, d_all, MW, ncclUint64, x.c->comm, x.s), "ncclAllGather");
  } else {
    Status cp = hip_local(hipMemcpyAsync(d_all, d_mine, sizeof(uint64_t) * MW, hipMemcpyDeviceToDevice, x.s));
    if (x.local.ok()) x.local = cp;
  }
  ++x.rounds;
  return Status::OK();
}

// the ONE read-back before the payload: every rank's state, capacities and counts
static std::vector<uint64_t> read_round1(GroupedExchange& x) {
  const int W = x.c->world;
  std::vector<uint64_t> words((size_t)W * Round1Matrix::message_words(W));
  Status rb = read_back(words.data(), x.c->words + x.c->at.round1_all, words.size(), x.s);
  if (x.local.ok()) x.local = rb;
  ++x.host_syncs;
  return words;
}

// some rank owns (or holds) more groups than it made room for: this rank allocates again if it is one of them, and the ranks
// agree on the outcome.  (the second exchange_import_begin overwrites the relation's import_keep; that is to be
// fixed HERE, with a test of its own.)
static Status allocate_again_and_agree(GroupedExchange& x, const PayloadPlan& plan) {
  x.local = Status::OK();
  Status st;
  if (plan.send_total() > x.send_cap) {
    x.send.reset();
    x.send_cap = plan.send_total();
    x.send = alloc_payload(x, x.send_cap, &st);
    if (!x.send) x.local = st;
  }
  if (x.local.ok() && plan.recv_total() > x.recv_cap) {
    x.recv.reset();
    x.recv_cap = plan.recv_total();
    x.recv = alloc_payload(x, x.recv_cap, &st);
    if (!x.recv) x.local = st;
    if (x.local.ok()) x.local = x.a->exchange_import_begin(x.recv_cap);
  }
  Status ag = agree(x.c, x.local, 0x201ull, "while it allocated its exchange buffers", &x.host_syncs, x.s);
  ++x.rounds;
  DFX_RETURN_IF_ERROR(ag);
  return x.local;  // (world == 1: agree() is the identity)
}

// round 2: the buckets, one all-to-all per chunk of accumulator planes over the same keys, merged on the same stream.  The
// last chunk's messages carry the trailers.  A rank whose scatter / merge kernels fail keeps sending and receiving what was
// agreed (its peers merge rows they will throw away): its trailer ends the exchange on every rank.  Returns only what
// all_to_all_words reports; *sent_words: what this rank sent.
static Status round2_buckets(GroupedExchange& x, const PayloadPlan& plan, uint64_t* t_in, int64_t* sent_words) {
  const int W = x.c->world;
  uint64_t* sw = (uint64_t*)x.send.get();
  uint64_t* rw = (uint64_t*)x.recv.get();
  uint64_t* t_out = sw + payload_trailer_at(x.send_cap, x.widest);  // [W] how this rank was when it sent its last bucket
  std::vector<SendWords> send((size_t)W);
  std::vector<RecvWords> recv((size_t)W);
  for (int ch = 0; ch < x.n_chunks; ++ch) {
    const uint64_t nw = (uint64_t)x.a->exchange_chunk_words(ch);
    const bool last = ch == x.n_chunks - 1;
    if (x.local.ok()) x.local = x.a->exchange_export_chunk(ch, plan.send_counts, x.send.get(), (int64_t)(plan.send_total() * nw));
    if (x.local.ok() && last) x.local = injected(x.c, "export");
    if (last) {
      Status f = hip_local(launch_fill_u64(t_out, x.local.ok() ? 1ull : kPeerFailed, W, x.s));
      if (x.local.ok()) x.local = f;
      Status z = hip_local(hipMemsetAsync(t_in, 0, sizeof(uint64_t) * (size_t)W, x.s));
      if (x.local.ok()) x.local = z;
    }
    for (int peer = 0; peer < W; ++peer) {
      send[(size_t)peer] = {sw + plan.sbase[(size_t)peer] * nw, (size_t)((uint64_t)plan.send_counts[(size_t)peer] * nw)};
      recv[(size_t)peer] = {rw + plan.rbase[(size_t)peer] * nw, (size_t)((uint64_t)plan.recv_counts[(size_t)peer] * nw)};
    }
    DFX_RETURN_IF_ERROR(all_to_all_words(x.c, send, recv, x.s, last ? t_out : nullptr, last ? t_in : nullptr));
    ++x.rounds;
    if (x.local.ok()) x.local = x.a->exchange_import_chunk(ch, x.recv.get(), plan.recv_counts.data(), W);
    *sent_words += (int64_t)(plan.send_total() * nw);
  }
  return Status::OK();
}

// the one synchronisation of the payload rounds: the peers' trailers and, inside exchange_import_finish, the new table's
// control block (also when this rank is not well: the trailers)
static std::vector<uint64_t> read_trailers_and_finish_import(GroupedExchange& x, const uint64_t* t_in) {
  std::vector<uint64_t> trailers((size_t)x.c->world, 0);
  Status rb = hip_local(hipMemcpyAsync(trailers.data(), t_in, sizeof(uint64_t) * trailers.size(), hipMemcpyDeviceToHost, x.s));
  if (x.local.ok()) x.local = rb;
  Status fin = x.a->exchange_import_finish();
  if (x.local.ok()) x.local = fin;
  ++x.host_syncs;
  return trailers;
}

static Status exchange_grouped(AggregateRelation* a, dfx_comm* c, int64_t* stats, long long t_begin) {
  GroupedExchange x;
  x.a = a;
  x.c = c;
  x.s = ctx().stream;
  drain_and_synchronise(x);
  const long long t_local = ScopedUs::now();
  counters().xchg_local_us += t_local - t_begin;
  if (x.local.ok()) x.local = injected(c, "drain");
  describe_query(x);
  if (a->exchange_dicts() > 0) DFX_RETURN_IF_ERROR(agree_and_globalise_dictionaries(x));
  allocate_for_announced_capacity(x);
  DFX_RETURN_IF_ERROR(round1_all_gather(x));
  const std::vector<uint64_t> round1 = read_round1(x);
  counters().xchg_wait_peers_us += ScopedUs::now() - t_local;
  ScopedUs t_rest(&counters().xchg_exchange_us);
  // (every rank has finished round 1 -- the last collective before this point -- so leaving here strands nobody)
  if (!x.local.ok()) return x.local;
  const Round1Matrix M{round1.data(), c->world};
  DFX_RETURN_IF_ERROR(peer_error(M.check_peers(rank_state_word(true, x.shape)), "before the exchange"));
  const PayloadPlan plan = plan_payload(M, c->rank);  // (need_more: the same on every rank, it is computed from the same matrix)
  if (plan.need_more) DFX_RETURN_IF_ERROR(allocate_again_and_agree(x, plan));
  uint64_t* t_in = (uint64_t*)x.recv.get() + payload_trailer_at(x.recv_cap, x.widest);  // [W] how the peers were when they sent their last bucket
  int64_t sent_words = 0;
  DFX_RETURN_IF_ERROR(round2_buckets(x, plan, t_in, &sent_words));
  const std::vector<uint64_t> trailers = read_trailers_and_finish_import(x, t_in);
  counters().xchg_rounds += x.rounds;
  counters().xchg_host_syncs += x.host_syncs;
  if (!x.local.ok()) return x.local;
  if (const int failed = first_failed_rank(trailers.data(), c->world); failed >= 0)
    return peer_error({PeerVerdict::Failed, failed}, "during the payload rounds");
  if (stats) {
    stats[0] = (int64_t)plan.send_total();
    stats[1] = (int64_t)plan.recv_total();
    stats[2] = (int64_t)sizeof(uint64_t) * sent_words;
    stats[3] = x.host_syncs;
  }
  return Status::OK();
}

Status AggregateRelation::exchange(dfx_comm* c, int64_t* stats) {
  if (!c) return Status::Err(DFX_GENERAL, "null communicator");
  if (stats) stats[0] = stats[1] = stats[2] = stats[3] = 0;
  // phase clocks of this rank (counters xchg_*): the local scan until the stream is idle, the first agreement (the wait for the
  // slowest rank), everything after
  ++counters().xchg_calls;
  const long long t_begin = ScopedUs::now();
  return is_ungrouped() ? exchange_ungrouped(this, c, stats, t_begin) : exchange_grouped(this, c, stats, t_begin);
}

}  // namespace dfx

using namespace dfx;

extern "C" int32_t dfx_aggregate_exchange(struct ArrowArrayStream* agg, dfx_comm* comm, int64_t* stats, char* err, size_t errlen) {
  return c_abi_guard(err, errlen, [&]() -> int32_t {
    Relation* r = peek_exported(agg);
    if (Status refused = distinct_sets_exchange_refusal(r); !refused.ok())  // (dfx_distinct.cpp: COUNT_DISTINCT, MIN / MAX of Utf8)
      return to_c(refused, err, errlen);
    if (!r || r->kind() != REL_AGGREGATE)
      return to_c(Status::Err(DFX_GENERAL, "not an aggregate stream of this library"), err, errlen);
    return to_c(static_cast<AggregateRelation*>(r)->exchange(comm, stats), err, errlen);
  });
}
