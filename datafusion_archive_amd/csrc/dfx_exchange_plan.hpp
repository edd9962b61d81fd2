// dfx_exchange_plan.hpp -- the host arithmetic of the multi-GPU exchange (dfx_exchange.cpp), free of HIP and RCCL: where
// things lie in the communicator's slab, what a rank's state word says, how round 1's messages read as a count matrix, what
// every rank concludes from it.  Every rank runs these functions over the SAME words; that they conclude the same is what
// keeps the ranks in the same collectives.  Plain C++17, so that tests/native/exchange_plan_check.cpp can hold them against
// naive restatements at worlds no test has run on a GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace dfx {

// ---- a rank's state word ----------------------------------------------------------------------------------------------
constexpr uint64_t kPeerFailed = ~0ull;  // travels instead of a state word / a count / a trailer: the sender hit an error, every rank gives up together

// "I am well, and this is what I am about to exchange" (`shape`: keys, chunks, dictionaries ...), or the failure mark
inline uint64_t rank_state_word(bool well, uint64_t shape) { return well ? (1ull | (shape << 8)) : kPeerFailed; }

enum class PeerVerdict { Ok, Failed, Differs };
struct PeerCheck {
  PeerVerdict verdict = PeerVerdict::Ok;
  int rank = -1;  // who failed / who differs
};
// the lowest rank whose word (words[r * stride]) is the failure mark, or -1
inline int first_failed_rank(const uint64_t* words, int world, size_t stride = 1) {
  for (int r = 0; r < world; ++r)
    if (words[(size_t)r * stride] == kPeerFailed) return r;
  return -1;
}
// words[r * stride]: what rank r said; mine: what this rank said (a rank that is not well never asks).  The lowest failed
// rank is named before any rank that merely differs.
inline PeerCheck check_peers(const uint64_t* words, int world, uint64_t mine, size_t stride = 1) {
  const int failed = first_failed_rank(words, world, stride);
  if (failed >= 0) return {PeerVerdict::Failed, failed};
  for (int r = 0; r < world; ++r)
    if (words[(size_t)r * stride] != mine) return {PeerVerdict::Differs, r};
  return {};
}

// ---- the slab ---------------------------------------------------------------------------------------------------------
constexpr size_t kUngroupedStateWords = 16;  // 2 x kMaxAggs (dfx_device.hpp): has-value flag + value bits per accumulator slot
// a round-1 message: state word, receive capacity, send capacity, then W counts
enum : size_t { kRound1State = 0, kRound1RecvCap = 1, kRound1SendCap = 2, kRound1Header = 3 };

// offsets in 64-bit words of the regions of dfx_comm::words, W = world (a few spare words behind most regions)
struct SlabLayout {
  size_t flags = 0;        // [2 W]             agree(): the word for every peer | the word from every peer
  size_t dict_mine = 0;    // [3]               a dictionary's {strings or failure mark, bytes, 0}
  size_t dict_all = 0;     // [3 W]             ... of every rank
  size_t state_mine = 0;   // [16]              ungrouped: zeros to send when this rank has no state block
  size_t state_all = 0;    // [16 W]            ungrouped: every rank's state block
  size_t round1_mine = 0;  // [W + 3]           grouped: this rank's round-1 message
  size_t round1_all = 0;   // [W][W + 3]        grouped: every rank's
  size_t total = 0;

  explicit SlabLayout(int world) {
    const size_t W = (size_t)world;
    size_t at = 0;
    auto take = [&at](size_t words, size_t spare) {
      const size_t begin = at;
      at += words + spare;
      return begin;
    };
    flags = take(2 * W, 0);
    dict_mine = take(3, 1);
    dict_all = take(3 * W, 4);
    state_mine = take(kUngroupedStateWords, 0);
    state_all = take(kUngroupedStateWords * W, 8);
    round1_mine = take(W + kRound1Header, 1);
    round1_all = take(W * (W + kRound1Header), 8);
    total = at;
  }
};

// ---- round 1 as every rank reads it -----------------------------------------------------------------------------------
// W messages of W + 3 words, in rank order
struct Round1Matrix {
  const uint64_t* words;
  int world;

  static size_t message_words(int world) { return (size_t)world + kRound1Header; }
  const uint64_t* message(int r) const { return words + (size_t)r * message_words(world); }
  uint64_t state_word(int r) const { return message(r)[kRound1State]; }
  uint64_t recv_capacity(int r) const { return message(r)[kRound1RecvCap]; }  // groups r can receive without allocating anything more
  uint64_t send_capacity(int r) const { return message(r)[kRound1SendCap]; }  // ... and send
  uint64_t count(int from, int to) const { return message(from)[kRound1Header + (size_t)to]; }  // groups `from` holds that `to` owns
  PeerCheck check_peers(uint64_t mine) const { return ::dfx::check_peers(words + kRound1State, world, mine, message_words(world)); }
};

// what one rank sends and receives in round 2 (groups per peer, and where each peer's bucket begins), and whether some
// rank of the world has to allocate again first -- the same answer on every rank
struct PayloadPlan {
  std::vector<int64_t> send_counts, recv_counts;  // [W]
  std::vector<uint64_t> sbase, rbase;             // [W + 1] prefix sums
  bool need_more = false;
  uint64_t send_total() const { return sbase.back(); }
  uint64_t recv_total() const { return rbase.back(); }
};
inline PayloadPlan plan_payload(const Round1Matrix& M, int rank) {
  const int W = M.world;
  PayloadPlan p;
  p.send_counts.assign((size_t)W, 0);
  p.recv_counts.assign((size_t)W, 0);
  p.sbase.assign((size_t)W + 1, 0);
  p.rbase.assign((size_t)W + 1, 0);
  for (int r = 0; r < W; ++r) {
    uint64_t into_r = 0, from_r = 0;
    for (int q = 0; q < W; ++q) {
      into_r += M.count(q, r);
      from_r += M.count(r, q);
    }
    if (into_r > M.recv_capacity(r) || from_r > M.send_capacity(r)) p.need_more = true;
  }
  for (int r = 0; r < W; ++r) {
    p.send_counts[(size_t)r] = (int64_t)M.count(rank, r);
    p.recv_counts[(size_t)r] = (int64_t)M.count(r, rank);
    p.sbase[(size_t)r + 1] = p.sbase[(size_t)r] + (uint64_t)p.send_counts[(size_t)r];
    p.rbase[(size_t)r + 1] = p.rbase[(size_t)r] + (uint64_t)p.recv_counts[(size_t)r];
  }
  return p;
}

// ---- a payload buffer: room for `groups` rows of `row_words`, then one trailer word per rank ---------------------------
inline uint64_t payload_trailer_at(uint64_t groups, int row_words) { return groups * (uint64_t)row_words; }
inline uint64_t payload_buffer_words(uint64_t groups, int row_words, int world) { return payload_trailer_at(groups, row_words) + (uint64_t)world; }

}  // namespace dfx
