// exchange_plan_check.cpp -- the host arithmetic of the multi-GPU exchange (csrc/dfx_exchange_plan.hpp) against naive
// restatements, at worlds the GPU tests never reach: the slab's regions, what every rank plans to send and receive from
// round 1's count matrix and whether all of them take the extra allocation round, the verdict on the peers' state words.
// Stand-alone (tests/test_exchange_plan_host.py builds it with g++, once more with -fsanitize=address,undefined); fixed seed.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "../../datafusion_archive_amd/csrc/dfx_exchange_plan.hpp"

using namespace dfx;

static long long g_checks = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    ++g_checks;                                            \
    if (!(cond)) {                                         \
      printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); \
      printf(__VA_ARGS__);                                 \
      printf("\n");                                        \
      exit(1);                                             \
    }                                                      \
  } while (0)

// ---- slab ---------------------------------------------------------------------------------------------------------------
static void check_slab() {
  const size_t kMaxAggs = 8;  // (csrc/dfx_device.hpp)
  for (int W = 1; W <= 1024; ++W) {
    const SlabLayout L(W);
    const size_t w = (size_t)W;
    const size_t begin[] = {L.flags, L.dict_mine, L.dict_all, L.state_mine, L.state_all, L.round1_mine, L.round1_all, L.total};
    const size_t need[] = {2 * w, 3, 3 * w, 2 * kMaxAggs, 2 * kMaxAggs * w, w + 3, w * (w + 3)};
    for (int i = 0; i < 7; ++i) {
      CHECK(begin[i] < begin[i + 1], "W=%d region %d is not in front of the next", W, i);
      CHECK(begin[i + 1] - begin[i] >= need[i], "W=%d region %d holds %zu words, needs %zu", W, i, begin[i + 1] - begin[i], need[i]);
      CHECK(begin[i] + need[i] <= L.total, "W=%d region %d ends behind the slab", W, i);
    }
  }
}

// ---- plan ---------------------------------------------------------------------------------------------------------------
struct World {  // the naive form: a matrix and two capacity vectors
  int W;
  std::vector<std::vector<uint64_t>> cnt;  // cnt[a][b]: groups a holds that b owns
  std::vector<uint64_t> recv_cap, send_cap;
  uint64_t into(int r) const {
    uint64_t n = 0;
    for (int a = 0; a < W; ++a) n += cnt[(size_t)a][(size_t)r];
    return n;
  }
  uint64_t from(int r) const {
    uint64_t n = 0;
    for (int b = 0; b < W; ++b) n += cnt[(size_t)r][(size_t)b];
    return n;
  }
  bool naive_need_more() const {
    for (int r = 0; r < W; ++r)
      if (into(r) > recv_cap[(size_t)r] || from(r) > send_cap[(size_t)r]) return true;
    return false;
  }
  std::vector<uint64_t> messages(uint64_t state) const {  // as round 1's all-gather lays them out
    std::vector<uint64_t> m;
    for (int r = 0; r < W; ++r) {
      m.push_back(state);
      m.push_back(recv_cap[(size_t)r]);
      m.push_back(send_cap[(size_t)r]);
      for (int b = 0; b < W; ++b) m.push_back(cnt[(size_t)r][(size_t)b]);
    }
    return m;
  }
};

static void check_plans_of(const World& w, const char* what) {
  const int W = w.W;
  const std::vector<uint64_t> words = w.messages(rank_state_word(true, 0x200));
  CHECK(words.size() == (size_t)W * Round1Matrix::message_words(W), "%s W=%d: message size", what, W);
  const Round1Matrix M{words.data(), W};
  std::vector<PayloadPlan> plans;
  for (int r = 0; r < W; ++r) plans.push_back(plan_payload(M, r));
  const bool want_more = w.naive_need_more();
  for (int a = 0; a < W; ++a) {
    const PayloadPlan& p = plans[(size_t)a];
    CHECK(M.recv_capacity(a) == w.recv_cap[(size_t)a] && M.send_capacity(a) == w.send_cap[(size_t)a], "%s W=%d rank %d: capacities", what, W, a);
    CHECK(p.need_more == want_more, "%s W=%d rank %d: need_more %d, naive %d", what, W, a, (int)p.need_more, (int)want_more);
    CHECK(p.send_counts.size() == (size_t)W && p.recv_counts.size() == (size_t)W && p.sbase.size() == (size_t)W + 1 && p.rbase.size() == (size_t)W + 1,
          "%s W=%d rank %d: sizes", what, W, a);
    uint64_t s = 0, r = 0;
    for (int b = 0; b < W; ++b) {
      CHECK(M.count(a, b) == w.cnt[(size_t)a][(size_t)b], "%s W=%d: count(%d, %d)", what, W, a, b);
      CHECK((uint64_t)p.send_counts[(size_t)b] == w.cnt[(size_t)a][(size_t)b], "%s W=%d: %d sends to %d", what, W, a, b);
      CHECK(p.send_counts[(size_t)b] == plans[(size_t)b].recv_counts[(size_t)a], "%s W=%d: what %d sends to %d is not what %d receives from %d", what, W, a, b, b, a);
      CHECK(p.sbase[(size_t)b] == s && p.rbase[(size_t)b] == r, "%s W=%d rank %d: prefix sums at %d", what, W, a, b);
      s += w.cnt[(size_t)a][(size_t)b];
      r += w.cnt[(size_t)b][(size_t)a];
    }
    CHECK(p.sbase[(size_t)W] == s && p.rbase[(size_t)W] == r, "%s W=%d rank %d: totals", what, W, a);
    CHECK(p.send_total() == w.from(a) && p.recv_total() == w.into(a), "%s W=%d rank %d: totals against the row / column sums", what, W, a);
  }
}

static void check_plans(std::mt19937_64& rng) {
  const int worlds[] = {1, 2, 3, 8, 64};
  for (int W : worlds) {
    for (int trial = 0; trial < 60; ++trial) {
      World w;
      w.W = W;
      w.cnt.assign((size_t)W, std::vector<uint64_t>((size_t)W, 0));
      const int flavour = trial % 5;  // 0 all zeros, 1 small with zeros, 2 one rank owns almost everything, 3 near 2^40, 4 mixed
      const int owner = (int)(rng() % (uint64_t)W);
      for (int a = 0; a < W; ++a)
        for (int b = 0; b < W; ++b) {
          uint64_t v = 0;
          if (flavour == 1) v = rng() % 3 ? rng() % 1000 : 0;
          if (flavour == 2) v = b == owner ? 100000 + rng() % 100000 : rng() % 2;
          if (flavour == 3) v = (1ull << 40) - rng() % 5;
          if (flavour == 4) v = rng() % 4 == 0 ? (1ull << 40) + rng() % 7 : rng() % 50;
          w.cnt[(size_t)a][(size_t)b] = v;
        }
      // capacities exactly met: nobody needs more
      w.recv_cap.resize((size_t)W);
      w.send_cap.resize((size_t)W);
      for (int r = 0; r < W; ++r) {
        w.recv_cap[(size_t)r] = w.into(r);
        w.send_cap[(size_t)r] = w.from(r);
      }
      CHECK(!w.naive_need_more(), "exactly met");
      check_plans_of(w, "capacities exactly met");
      // ample, as the library announces them (twice the own groups + 4096 / the own groups + 64) -- whatever that gives
      World ample = w;
      for (int r = 0; r < W; ++r) {
        ample.recv_cap[(size_t)r] = 2 * w.from(r) + 4096;
        ample.send_cap[(size_t)r] = w.from(r) + 64;
      }
      check_plans_of(ample, "announced capacities");
      // one group over, on one rank, on the receive side alone / on the send side alone
      const int victim = (int)(rng() % (uint64_t)W);
      if (w.into(victim) > 0) {
        World over = w;
        over.recv_cap[(size_t)victim] -= 1;
        CHECK(over.naive_need_more(), "one over (receive)");
        check_plans_of(over, "one over on the receive side");
      }
      if (w.from(victim) > 0) {
        World over = w;
        over.send_cap[(size_t)victim] -= 1;
        CHECK(over.naive_need_more(), "one over (send)");
        check_plans_of(over, "one over on the send side");
      }
      // random capacities around the sums
      World any = w;
      for (int r = 0; r < W; ++r) {
        any.recv_cap[(size_t)r] = w.into(r) + rng() % 3 - (w.into(r) > 0 && rng() % 8 == 0 ? 1 : 0);
        any.send_cap[(size_t)r] = w.from(r) + rng() % 3 - (w.from(r) > 0 && rng() % 8 == 0 ? 1 : 0);
      }
      check_plans_of(any, "random capacities");
    }
  }
  CHECK(payload_buffer_words(1000, 7, 8) == 1000 * 7 + 8 && payload_trailer_at(1000, 7) == 7000, "payload buffer: rows, then a trailer word per rank");
  CHECK(payload_buffer_words((1ull << 40) + 3, 17, 64) == ((1ull << 40) + 3) * 17 + 64, "payload buffer beyond 2^32 words");
}

// ---- verdict ------------------------------------------------------------------------------------------------------------
// both forms: the contiguous words of agree() and the strided state words of round 1's messages
static PeerCheck verdict_both_ways(const std::vector<uint64_t>& said, uint64_t mine) {
  const int W = (int)said.size();
  const PeerCheck flat = check_peers(said.data(), W, mine);
  std::vector<uint64_t> words((size_t)W * Round1Matrix::message_words(W), 7);
  for (int r = 0; r < W; ++r) words[(size_t)r * Round1Matrix::message_words(W)] = said[(size_t)r];
  const Round1Matrix M{words.data(), W};
  const PeerCheck strided = M.check_peers(mine);
  CHECK(flat.verdict == strided.verdict && flat.rank == strided.rank, "W=%d: the two forms of the verdict differ", W);
  for (int r = 0; r < W; ++r) CHECK(M.state_word(r) == said[(size_t)r], "W=%d: state word of rank %d", W, r);
  return flat;
}

static void check_verdicts(std::mt19937_64& rng) {
  CHECK(rank_state_word(true, 0x2345) == (1ull | (0x2345ull << 8)) && rank_state_word(false, 0x2345) == kPeerFailed && kPeerFailed == ~0ull, "state word");
  const int worlds[] = {1, 2, 3, 8, 64};
  for (int W : worlds) {
    for (int trial = 0; trial < 50; ++trial) {
      const uint64_t mine = rank_state_word(true, rng() & 0xFFFFFFFFFFFFull);
      const uint64_t other = rank_state_word(true, (mine >> 8) ^ (1 + rng() % 1000));
      CHECK(other != mine && other != kPeerFailed, "a differing word");
      std::vector<uint64_t> well((size_t)W, mine);
      PeerCheck v = verdict_both_ways(well, mine);
      CHECK(v.verdict == PeerVerdict::Ok, "W=%d: all well", W);
      const int a = (int)(rng() % (uint64_t)W);
      {  // one failed rank is named
        std::vector<uint64_t> s = well;
        s[(size_t)a] = kPeerFailed;
        v = verdict_both_ways(s, mine);
        CHECK(v.verdict == PeerVerdict::Failed && v.rank == a, "W=%d: rank %d failed, verdict names %d", W, a, v.rank);
      }
      {  // a differing rank is named
        std::vector<uint64_t> s = well;
        s[(size_t)a] = other;
        v = verdict_both_ways(s, mine);
        CHECK(v.verdict == PeerVerdict::Differs && v.rank == a, "W=%d: rank %d differs, verdict names %d", W, a, v.rank);
      }
      if (W < 2) continue;
      int b = (int)(rng() % (uint64_t)(W - 1));
      if (b >= a) ++b;
      const int lo = a < b ? a : b, hi = a < b ? b : a;
      {  // two failed ranks: the lower
        std::vector<uint64_t> s = well;
        s[(size_t)a] = s[(size_t)b] = kPeerFailed;
        v = verdict_both_ways(s, mine);
        CHECK(v.verdict == PeerVerdict::Failed && v.rank == lo, "W=%d: ranks %d and %d failed, verdict names %d", W, lo, hi, v.rank);
      }
      {  // two differing ranks: the lower
        std::vector<uint64_t> s = well;
        s[(size_t)a] = s[(size_t)b] = other;
        v = verdict_both_ways(s, mine);
        CHECK(v.verdict == PeerVerdict::Differs && v.rank == lo, "W=%d: ranks %d and %d differ, verdict names %d", W, lo, hi, v.rank);
      }
      for (int order = 0; order < 2; ++order) {  // a failed rank beats a differing rank, whichever comes first
        const int failed = order ? lo : hi, differs = order ? hi : lo;
        std::vector<uint64_t> s = well;
        s[(size_t)failed] = kPeerFailed;
        s[(size_t)differs] = other;
        v = verdict_both_ways(s, mine);
        CHECK(v.verdict == PeerVerdict::Failed && v.rank == failed, "W=%d: rank %d failed and rank %d differs, verdict names %d", W, failed, differs, v.rank);
      }
    }
  }
}

int main() {
  std::mt19937_64 rng(20240611);
  check_slab();
  check_plans(rng);
  check_verdicts(rng);
  printf("ok: %lld checks (slab at worlds 1..1024; plans and verdicts at worlds 1, 2, 3, 8, 64)\n", g_checks);
  return 0;
}
