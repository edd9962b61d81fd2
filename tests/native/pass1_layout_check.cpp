// pass1_layout_check.cpp -- the routed layout of the partitioned GROUP BY (csrc/dfx_pass1_layout.hpp) as a stand-alone program:
// choose_routed_layout against tables written out by hand from the formulas of the ensure_partition it replaced (256 CUs, the
// default options, an LDS budget of 158 KB), then two properties over the tables' shapes x the three scratch layouts x two pads:
// launch_partition takes every accepted layout, and the regions lie inside the row buffer and share no byte.
// tests/test_pass1_layout.py builds it plain and with -fsanitize=address,undefined.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../../datafusion_archive_amd/csrc/dfx_pass1_layout.hpp"

using namespace dfx;

static int failures = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      printf("FAILED line %d: %s\n", __LINE__, #cond);               \
      ++failures;                                                    \
    }                                                                \
  } while (0)

static const char* name_of(RoutedLayoutKind k) {
  return k == RoutedLayoutKind::refused_pair_scan ? "refused: pair scan" : k == RoutedLayoutKind::refused_table_blocks ? "refused: table blocks" : kRoutedLayoutName[(int)k];
}

// One key, SUM(v) over 2^22 rows, 256 table blocks of 8192 slots, 256 CUs, the defaults of AggOptions (dfx_relation.hpp).
static RoutedLayoutQuery query(uint32_t n_parts = 256, int na = 1) {
  RoutedLayoutQuery q = {};
  q.rows = 1 << 22, q.kw = 1, q.na = na;
  q.block_slots = 8192, q.table_slots = (uint64_t)n_parts * 8192, q.cu_count = 256;
  q.phase = PairPhase::none;
  q.opt.narrow_keys = -1, q.opt.narrow_chunk16 = 1, q.opt.hot_keys = -1, q.opt.pass2_stream = 1;
  q.opt.pass1_ws = 8, q.opt.pass1_ws_dense = 0, q.opt.pass1_ws_dense_scanners = 4;
  q.opt.partition_mode = 2, q.opt.partition_layout = 1, q.opt.partition_block = 1024;
  return q;
}
static RoutedLayoutQuery narrow_query(uint32_t n_parts = 256, int na = 1) {
  RoutedLayoutQuery q = query(n_parts, na);
  q.narrow = true;
  return q;
}
// two or three aggregates of one operand (AVG = SUM + COUNT ...), narrow keys
static RoutedLayoutQuery shared_query(uint32_t n_parts, int na) {
  RoutedLayoutQuery q = narrow_query(n_parts, na);
  q.shared_operand = q.same_operand_all = true, q.split_distinct = 1;
  return q;
}
// the pair scan: na aggregates over two operands, accumulator 0 on operand 0, the others on operand 1
static RoutedLayoutQuery pair_query(int na) {
  RoutedLayoutQuery q = narrow_query(256, na);
  q.phase = PairPhase::pair, q.split_distinct = 2, q.split_ops = (1u << na) - 2u, q.split_arg1 = 1;
  return q;
}
// ... its shared-operand flavour: the planes
static RoutedLayoutQuery planes_query(int na) {
  RoutedLayoutQuery q = shared_query(256, na);
  q.phase = PairPhase::planes;
  return q;
}

// ---- the flavour: name, row form, launch shape -------------------------------------------------------------------------------
static void flavour(int line, const RoutedLayoutQuery& q, const char* name, uint32_t n_words, uint32_t mode, uint32_t block, uint32_t stage_rows,
                    uint32_t n_producers, uint32_t flags, uint32_t ws_scanners) {
  const RoutedLayout r = choose_routed_layout(q);
  const DevPartition& p = r.PT;
  const bool ok = strcmp(name_of(r.kind), name) == 0 && p.n_parts == (uint32_t)(q.table_slots / q.block_slots) && p.part_shift == 13 && p.n_words == n_words &&
                  p.mode == mode && p.block == block && p.stage_rows == stage_rows && p.n_producers == n_producers && p.flags == flags && p.ws_scanners == ws_scanners &&
                  p.rows == nullptr && p.counts == nullptr && p.snap_host == nullptr && p.snap_done == nullptr;
  if (!ok) {
    printf("FAILED line %d: %s, n_parts %u, part_shift %u, n_words %u, mode 0x%x, block %u, stage_rows %u, n_producers %u, flags 0x%x, ws_scanners %u; expected %s, %u, 0x%x, %u, %u, %u, 0x%x, %u\n",
           line, name_of(r.kind), p.n_parts, p.part_shift, p.n_words, p.mode, p.block, p.stage_rows, p.n_producers, p.flags, p.ws_scanners, name, n_words, mode, block, stage_rows,
           n_producers, flags, ws_scanners);
    ++failures;
  }
}
#define FLAVOUR(...) flavour(__LINE__, __VA_ARGS__)

static void refused(int line, const RoutedLayoutQuery& q, const char* name) {
  const RoutedLayout r = choose_routed_layout(q);
  if (strcmp(name_of(r.kind), name) != 0) {
    printf("FAILED line %d: %s; expected %s\n", line, name_of(r.kind), name);
    ++failures;
  }
}
#define REFUSED(...) refused(__LINE__, __VA_ARGS__)

// ---- the geometry: capacities, strides, bytes ---------------------------------------------------------------------------------
static void geometry(int line, const RoutedLayoutQuery& q, uint32_t cap_rows, uint32_t worst, uint64_t part_stride, uint64_t prod_stride, uint64_t win_stride, size_t row_bytes,
                     size_t cnt_bytes) {
  const RoutedLayout r = choose_routed_layout(q);
  const DevPartition& p = r.PT;
  if ((int)r.kind < 0 || p.cap_rows != cap_rows || r.worst != worst || p.part_stride != part_stride || p.prod_stride != prod_stride || p.win_stride != win_stride ||
      r.row_bytes != row_bytes || r.cnt_bytes != cnt_bytes) {
    printf("FAILED line %d: %s, cap_rows %u, worst %u, part_stride %llu, prod_stride %llu, win_stride %llu, row_bytes %zu, cnt_bytes %zu; expected %u, %u, %llu, %llu, %llu, %zu, %zu\n", line,
           name_of(r.kind), p.cap_rows, r.worst, (unsigned long long)p.part_stride, (unsigned long long)p.prod_stride, (unsigned long long)p.win_stride, r.row_bytes, r.cnt_bytes, cap_rows,
           worst, (unsigned long long)part_stride, (unsigned long long)prod_stride, (unsigned long long)win_stride, row_bytes, cnt_bytes);
    ++failures;
  }
}
#define GEOMETRY(...) geometry(__LINE__, __VA_ARGS__)
static void capacity(int line, const RoutedLayoutQuery& q, uint32_t cap_rows, uint32_t worst) {
  const RoutedLayout r = choose_routed_layout(q);
  if ((int)r.kind < 0 || r.PT.cap_rows != cap_rows || r.worst != worst) {
    printf("FAILED line %d: %s, cap_rows %u, worst %u; expected %u, %u\n", line, name_of(r.kind), r.PT.cap_rows, r.worst, cap_rows, worst);
    ++failures;
  }
}
#define CAPACITY(...) capacity(__LINE__, __VA_ARGS__)

// ---- the address rule (dfx_device.hpp: DevPartition, the chunk geometries; dfx_k_partition_inl.hpp: region_row, region_row12,
// region_row12g), restated: the bytes [first, first + size) of row slot `row` of the region producer `producer` fills for partition `part`
struct Bytes {
  uint64_t first, size;
};
static Bytes row_slot(const DevPartition& p, uint32_t part, uint32_t producer, uint32_t row) {
  const uint64_t region = 8 * ((uint64_t)part * p.part_stride + (uint64_t)producer * p.prod_stride);
  if (p.flags & PTF_PAIR) return {region + (uint64_t)(row / 6) * 128 + (uint64_t)(row % 6) * 20, 20};    // six 20-byte rows per 128-byte line
  if (p.flags & PTF_CHUNK16) return {region + (uint64_t)(row / 10) * 128 + (uint64_t)(row % 10) * 12, 12};  // ten 12-byte rows per line
  const uint64_t window = region + 8 * (uint64_t)(row >> 6) * p.win_stride;  // 64-row windows, win_stride words apart
  if (p.flags & PTF_NARROW) return {window + (uint64_t)(row & 63u) * 12, 12};
  return {window + (uint64_t)(row & 63u) * p.n_words * 8, (uint64_t)p.n_words * 8};
}

static long property_cells = 0;
static void properties(const RoutedLayoutQuery& q0) {
  for (int layout = 0; layout < 3; ++layout)
    for (int pad = 0; pad <= 100; pad += 100) {
      RoutedLayoutQuery q = q0;
      q.opt.partition_layout = layout, q.opt.partition_pad = pad;
      const RoutedLayout r = choose_routed_layout(q);
      if ((int)r.kind < 0) continue;  // (the pair scan has no windowed layout)
      const DevPartition& p = r.PT;
      ++property_cells;
      bool ok = partition_launchable(p);  // launch_partition takes it
      ok = ok && partition_stage_bytes(p) <= kPass1LdsLimit;
      // capacities: whole 64-row windows; LINE chunks: whole lines AND whole windows (320 rows -- not whole 60-row trips of pass 2: an
      // oddity that stays, the last trip of a full region is a short one); pair rows: whole lines and whole 60-row trips
      const uint32_t quantum = (p.flags & PTF_PAIR) ? 60u : (p.flags & PTF_CHUNK16) ? 320u : 64u;
      ok = ok && p.cap_rows >= quantum && p.cap_rows % quantum == 0 && r.worst >= quantum && r.worst % quantum == 0 && r.worst <= p.cap_rows;
      ok = ok && r.cnt_bytes == (size_t)4 * p.n_parts * p.n_producers;
      // containment: the first and the last row slot of the first, a middle and the last region
      const uint32_t parts[3] = {0, p.n_parts / 2, p.n_parts - 1}, prods[3] = {0, p.n_producers / 2, p.n_producers - 1};
      for (uint32_t pa : parts)
        for (uint32_t pr : prods)
          for (uint32_t row : {0u, p.cap_rows - 1}) {
            const Bytes b = row_slot(p, pa, pr, row);
            ok = ok && b.first + b.size <= r.row_bytes;
          }
      // separation: every row slot of a region, of its producer's next one and of the next partition's -- no two share a byte
      if (ok) {
        const uint32_t pa = p.n_parts / 2, pr = p.n_producers / 2;
        std::vector<std::pair<uint64_t, uint64_t>> spans;
        const auto add = [&](uint32_t part, uint32_t producer) {
          for (uint32_t row = 0; row < p.cap_rows; ++row) {
            const Bytes b = row_slot(p, part, producer, row);
            spans.push_back({b.first, b.first + b.size});
          }
        };
        add(pa, pr);
        if (pr + 1 < p.n_producers) add(pa, pr + 1);
        if (pa + 1 < p.n_parts) add(pa + 1, pr);
        std::sort(spans.begin(), spans.end());
        for (size_t i = 1; i < spans.size(); ++i) ok = ok && spans[i - 1].second <= spans[i].first;
      }
      if (!ok) {
        printf("FAILED properties: %s, n_parts %u, n_words %u, flags 0x%x, layout %d, pad %d, cap_rows %u\n", name_of(r.kind), p.n_parts, p.n_words, p.flags, layout, pad, p.cap_rows);
        ++failures;
      }
    }
}

// flag words, written out
static const uint32_t kStream = 2, kHot = 4, kNarrow = 8, kChunk16 = 16, kShared = 32, kWs = 64, kPair = 128, kPlanes = 256;

int main() {
  static_assert(kNarrowLine, "the tables below are the LINE-chunk geometry");
  CHECK(kStream == PTF_STREAM_PASS2 && kHot == PTF_HOT && kNarrow == PTF_NARROW && kChunk16 == PTF_CHUNK16 && kShared == PTF_SHARED && kWs == PTF_WS && kPair == PTF_PAIR &&
        kPlanes == PTF_PLANES);
  // ---- the list ----
  const int kLayouts = (int)(sizeof(kRoutedLayoutName) / sizeof(kRoutedLayoutName[0]));
  CHECK(kLayouts == 7 && (int)RoutedLayoutKind::shared_ring == 0 && (int)RoutedLayoutKind::direct == 6 && (int)RoutedLayoutKind::refused_pair_scan < 0 &&
        (int)RoutedLayoutKind::refused_table_blocks < 0);
  for (int i = 0; i < kLayouts; ++i)
    for (int j = 0; j < i; ++j) CHECK(strcmp(kRoutedLayoutName[i], kRoutedLayoutName[j]) != 0);
  CHECK(strcmp(kRoutedLayoutName[(int)RoutedLayoutKind::ring16], "ring16") == 0 && strcmp(kRoutedLayoutName[(int)RoutedLayoutKind::sort], "sort") == 0);

  // ---- the LDS arithmetic, by hand (bytes; the budget is 158 KB = 161792) ----
  CHECK(kPass1LdsBudget == 161792 && kPass1LdsLimit == 163840);
  // wave-specialised: 412 per partition (384 of ring, 28 of counters) + 8256 + queues of 256 x (4 + 8 operands) + 16 each
  CHECK(partition_ws_bytes(256, 8) == 138432 && partition_ws_bytes(256, 4) == 150784 && partition_ws_bytes(256, 8, 2) == 154816 && partition_ws_bytes(512, 8) == 243904);
  // 16-row rings of 16-byte rows: 292 per partition + 57408; three words: 420 + 81984; four: 548 + 106560
  CHECK(partition_ring_bytes(2, 256, 16) == 132160 && partition_ring_bytes(2, 512, 16) == 206912);
  CHECK(partition_ring_bytes(3, 128, 16) == 135744 && partition_ring_bytes(3, 256, 16) == 189504 && partition_ring_bytes(4, 64, 16) == 141632 && partition_ring_bytes(4, 128, 16) == 176704);
  // 8-row rings: three words 228 per partition + 53312, four words 292 + 69696
  CHECK(partition_ring_bytes(3, 256, 8) == 111680 && partition_ring_bytes(3, 512, 8) == 170048 && partition_ring_bytes(4, 128, 8) == 107072 && partition_ring_bytes(4, 256, 8) == 144448);
  // narrow rows: three 128-byte line slots, 128-row queues; 16-row rings of 12-byte rows with 2048 hot-key pairs; the shared operand's
  CHECK(partition_ring_bytes(2, 256, 30, false, true) == 148544 && partition_ring_bytes(2, 256, 16, true, true) == 148544);
  CHECK(partition_ring_bytes(2, 256, 16, false, true, 128) == 99392 && partition_ring_bytes(2, 512, 16, false, true, 128) == 157760 && partition_ring_bytes(2, 1024, 16, false, true, 128) == 274496);
  // the counting sort (156 KB = 159744, block 512: 79 KB = 80896): (budget - 12 per partition - 88) / (8 per word + 4), whole workgroups of rows, 8192 at the most
  CHECK(partition_sort_capacity(2, 512, 1024, 159744) == 7168 && partition_sort_capacity(2, 1024, 1024, 159744) == 7168);
  CHECK(partition_sort_capacity(2, 512, 512, 80896) == 3584 && partition_sort_capacity(3, 512, 1024, 159744) == 5120);
  CHECK(partition_sort_capacity(1, 1, 1024, 159744) == 8192 && partition_sort_capacity(2, 8192, 1024, 98392) == 0);

  // ---- one aggregate, two-word rows, by partition count ----
  for (uint32_t parts : {1u, 64u, 256u}) FLAVOUR(query(parts), "ring16", 2, 2, 1024, 0, 256, kStream, 0);
  // An oddity, kept: the 8-row rings, written for rows of three and more words, also take two-word rows at 512 blocks -- 16-row rings
  // need 206912 bytes there, 8-row rings 512 x (128 + 36) + 16 x 128 x 16 + 4096 + 64 = 120896 -- so the counting sort starts at 1024
  CHECK(partition_ring_bytes(2, 512, 8) == 120896 && partition_ring_bytes(2, 1024, 8) == 204864);
  FLAVOUR(query(512), "ring8", 2, 0x102, 1024, 0, 256, kStream, 0);
  FLAVOUR(query(1024), "sort", 2, 1, 1024, 7168, 256, kStream, 0);
  for (uint32_t parts : {2048u, 4096u}) FLAVOUR(query(parts), "direct", 2, 0, 1024, 0, 256, kStream, 0);
  REFUSED(query(8192), "refused: table blocks");
  {  // what the refusal leaves in the DevPartition
    const RoutedLayout r = choose_routed_layout(query(8192));
    CHECK(r.PT.n_parts == 8192 && r.PT.n_words == 2 && r.PT.part_shift == 13 && r.PT.mode == 0 && r.PT.block == 0 && r.PT.n_producers == 0 && r.PT.cap_rows == 0 && r.row_bytes == 0);
  }
  {  // agg.partition_mode = 1: the sort wherever it fits, = 0: direct routing everywhere
    RoutedLayoutQuery q = query(256);
    q.opt.partition_mode = 1;
    FLAVOUR(q, "sort", 2, 1, 1024, 7168, 256, kStream, 0);
    q.opt.partition_mode = 0;
    FLAVOUR(q, "direct", 2, 0, 1024, 0, 256, kStream, 0);
  }
  {  // blocks of 4096 slots: the shift
    RoutedLayoutQuery q = query(256);
    q.block_slots = 4096, q.table_slots = 256 * 4096;
    const RoutedLayout r = choose_routed_layout(q);
    CHECK(r.kind == RoutedLayoutKind::ring16 && r.PT.n_parts == 256 && r.PT.part_shift == 12);
  }

  // ---- the ring family at 256 blocks ----
  {
    RoutedLayoutQuery q = narrow_query();
    FLAVOUR(q, "ring16", 2, 2, 1024, 0, 256, kNarrow | kChunk16 | kWs | kStream, 8);  // large chunks, wave specialisation, 8 scanners
    q.mostly_seen = true;
    FLAVOUR(q, "ring16", 2, 2, 1024, 0, 256, kNarrow | kChunk16 | kWs | kStream, 4);
    q.opt.pass1_ws_dense_scanners = 8;
    FLAVOUR(q, "ring16", 2, 2, 1024, 0, 256, kNarrow | kChunk16 | kWs | kStream, 8);
    q = narrow_query();
    q.opt.pass1_ws = 4;
    FLAVOUR(q, "ring16", 2, 2, 1024, 0, 256, kNarrow | kChunk16 | kWs | kStream, 4);
    q.opt.pass1_ws = 0;
    FLAVOUR(q, "ring16", 2, 2, 1024, 0, 256, kNarrow | kChunk16 | kStream, 0);
    q = narrow_query();
    q.skew_seen = true;  // hot-key pairs, and neither of the other two
    FLAVOUR(q, "ring16", 2, 2, 1024, 0, 256, kNarrow | kHot | kStream, 0);
    q.opt.hot_keys = 0;
    FLAVOUR(q, "ring16", 2, 2, 1024, 0, 256, kNarrow | kChunk16 | kWs | kStream, 8);
    q = query();
    q.opt.hot_keys = 1;  // 16-byte rows: 1024 pairs, 132160 + 16384 bytes
    FLAVOUR(q, "ring16", 2, 2, 1024, 0, 256, kHot | kStream, 0);
    q = narrow_query();
    q.opt.partition_layout = 2;  // windowed regions: narrow rows without the large chunks
    FLAVOUR(q, "ring16", 2, 2, 1024, 0, 256, kNarrow | kStream, 0);
    q = narrow_query();
    q.opt.partition_mode = 2 | 0x80;  // 16-byte rows
    FLAVOUR(q, "ring16", 2, 0x82, 1024, 0, 256, kStream, 0);
    CHECK(choose_routed_layout(q).want_flags == kNarrow);  // (the oddity: wanted, never set)
    q = narrow_query();
    q.dense_seen = true;
    FLAVOUR(q, "ring16", 2, 2, 1024, 0, 256, kNarrow | kChunk16 | kWs | kStream, 8);
    q.opt.pass1_ws_dense = -1;  // no wave specialisation above one half
    FLAVOUR(q, "ring16", 2, 2, 1024, 0, 256, kNarrow | kChunk16 | kStream, 0);
    q = narrow_query();
    q.opt.narrow_chunk16 = 0;
    FLAVOUR(q, "ring16", 2, 2, 1024, 0, 256, kNarrow | kStream, 0);
    q = narrow_query();
    q.opt.narrow_keys = 0;
    FLAVOUR(q, "ring16", 2, 2, 1024, 0, 256, kStream, 0);
    q = narrow_query();
    q.opt.pass2_stream = 0;
    FLAVOUR(q, "ring16", 2, 2, 1024, 0, 256, kNarrow | kChunk16 | kWs, 8);
    q = narrow_query(512);  // narrow keys do not help the partition count: 16-byte rows from here on, wanted narrow all the same
    FLAVOUR(q, "ring8", 2, 0x102, 1024, 0, 256, kStream, 0);
    CHECK(choose_routed_layout(q).want_flags == kNarrow);
    q = narrow_query(1024);
    FLAVOUR(q, "sort", 2, 1, 1024, 7168, 256, kStream, 0);
    q = narrow_query();
    q.kw = 2;  // two key words: three-word rows, nothing narrow
    FLAVOUR(q, "ring8", 3, 0x102, 1024, 0, 256, 0, 0);
  }

  // ---- rows of three and four words (two and three aggregates of different operands, one scan) ----
  for (uint32_t parts : {1u, 128u}) FLAVOUR(query(parts, 2), "ring16", 3, 2, 1024, 0, 256, 0, 0);
  FLAVOUR(query(256, 2), "ring8", 3, 0x102, 1024, 0, 256, 0, 0);
  FLAVOUR(query(512, 2), "sort", 3, 1, 1024, 5120, 256, 0, 0);
  for (uint32_t parts : {1u, 64u}) FLAVOUR(query(parts, 3), "ring16", 4, 2, 1024, 0, 256, 0, 0);
  for (uint32_t parts : {128u, 256u}) FLAVOUR(query(parts, 3), "ring8", 4, 0x102, 1024, 0, 256, 0, 0);
  FLAVOUR(narrow_query(256, 2), "ring8", 3, 0x102, 1024, 0, 256, 0, 0);  // (narrow keys: no narrow form for two operands outside the pair scan)

  // ---- the shared-operand ring ----
  for (int na = 2; na <= 3; ++na)
    for (uint32_t parts : {256u, 512u}) {  // (it fits 512 blocks: 157760 bytes; the wave-specialised forms do not)
      FLAVOUR(shared_query(parts, na), "shared_ring", 2, 2, 1024, 0, 256, kNarrow | kShared, 0);
      CHECK(choose_routed_layout(shared_query(parts, na)).want_flags == (kNarrow | kShared));
    }
  FLAVOUR(shared_query(1024, 2), "sort", 3, 1, 1024, 5120, 256, 0, 0);
  {
    RoutedLayoutQuery q = shared_query(256, 2);
    q.nulls_now = true;  // a raw operand has no validity: every aggregate's own operand then
    FLAVOUR(q, "ring8", 3, 0x102, 1024, 0, 256, 0, 0);
    q.has_pred = true;  // (an absorbed predicate helps the planes only)
    FLAVOUR(q, "ring8", 3, 0x102, 1024, 0, 256, 0, 0);
    q = shared_query(512, 2);
    q.nulls_now = true;
    FLAVOUR(q, "sort", 3, 1, 1024, 5120, 256, 0, 0);
    q = shared_query(256, 2);
    q.narrow = false;
    FLAVOUR(q, "ring8", 3, 0x102, 1024, 0, 256, 0, 0);
    q = shared_query(256, 2);
    q.opt.partition_mode = 1;
    FLAVOUR(q, "sort", 3, 1, 1024, 5120, 256, 0, 0);
    q = shared_query(256, 3);
    q.shared_operand = false;  // (four and more aggregates, or agg.shared_operand = 0: the operator says no)
    FLAVOUR(q, "ring8", 4, 0x102, 1024, 0, 256, 0, 0);
  }

  // ---- planes and pair rows at 256 blocks ----
  for (int na = 2; na <= 8; ++na) {
    RoutedLayoutQuery q = planes_query(na);
    q.split_ops = 0x55, q.split_arg1 = 7;  // (the planes do not look at them)
    FLAVOUR(q, "planes", 2, 2, 1024, 0, 256, kNarrow | kChunk16 | kWs | kShared | kPlanes, 8);
    const RoutedLayout r = choose_routed_layout(q);
    CHECK(r.PT.pair_ops == 0 && r.PT.pair_arg1 == 0 && r.want_flags == (kNarrow | kShared | kPlanes));
  }
  {
    RoutedLayoutQuery q = planes_query(3);
    q.mostly_seen = true;
    FLAVOUR(q, "planes", 2, 2, 1024, 0, 256, kNarrow | kChunk16 | kWs | kShared | kPlanes, 4);
    q = planes_query(3);
    q.nulls_now = true;
    REFUSED(q, "refused: pair scan");
    q.has_pred = true;  // absorbed: every surviving slot is valid
    FLAVOUR(q, "planes", 2, 2, 1024, 0, 256, kNarrow | kChunk16 | kWs | kShared | kPlanes, 8);
    q.unfused_now = true;
    REFUSED(q, "refused: pair scan");
    q = planes_query(3);
    q.same_operand_all = false;
    REFUSED(q, "refused: pair scan");
  }
  for (int na = 2; na <= 8; ++na) {
    const RoutedLayoutQuery q = pair_query(na);
    FLAVOUR(q, "pair_rows", (uint32_t)(1 + na), 2, 1024, 0, 256, kNarrow | kChunk16 | kWs | kPair | (na > 2 ? kPlanes : 0u), 8);
    const RoutedLayout r = choose_routed_layout(q);
    CHECK(r.PT.pair_ops == (1u << na) - 2u && r.PT.pair_arg1 == 1 && r.want_flags == (kNarrow | kPair | (na > 2 ? kPlanes : 0u)));
  }
  {
    RoutedLayoutQuery q = pair_query(2);
    q.mostly_seen = true;  // (always 8 scanners)
    FLAVOUR(q, "pair_rows", 3, 2, 1024, 0, 256, kNarrow | kChunk16 | kWs | kPair, 8);
    q = pair_query(2);
    q.nulls_now = true;  // two aggregates: the scan transforms each operand, nulls are fine; three and more travel raw
    FLAVOUR(q, "pair_rows", 3, 2, 1024, 0, 256, kNarrow | kChunk16 | kWs | kPair, 8);
    q = pair_query(3);
    q.nulls_now = true;
    REFUSED(q, "refused: pair scan");
    q.has_pred = true;
    FLAVOUR(q, "pair_rows", 4, 2, 1024, 0, 256, kNarrow | kChunk16 | kWs | kPair | kPlanes, 8);
    q = pair_query(2);
    q.split_distinct = 3;
    REFUSED(q, "refused: pair scan");
    q = pair_query(2);
    q.kw = 2;
    REFUSED(q, "refused: pair scan");
    q = pair_query(2);
    q.narrow = false;
    REFUSED(q, "refused: pair scan");
  }
  // the conditions pair rows and planes share: any of them false refuses the pair phase
  for (int planes = 0; planes < 2; ++planes) {
    const RoutedLayoutQuery q0 = planes ? planes_query(2) : pair_query(2);
    CHECK(pair_layout_fits(q0.opt, 256, planes != 0) && !pair_layout_fits(q0.opt, 512, planes != 0));
    RoutedLayoutQuery q = q0;
    q.table_slots = 512 * 8192;  // 243904 bytes of LDS
    REFUSED(q, "refused: pair scan");
    q = q0, q.opt.narrow_keys = 0;
    REFUSED(q, "refused: pair scan");
    q = q0, q.opt.narrow_chunk16 = 0;
    REFUSED(q, "refused: pair scan");
    q = q0, q.opt.pass1_ws = 0;
    REFUSED(q, "refused: pair scan");
    q = q0, q.opt.partition_layout = 2;
    REFUSED(q, "refused: pair scan");
    q = q0, q.opt.partition_mode = 1;
    REFUSED(q, "refused: pair scan");
    q = q0, q.opt.partition_mode = 2 | 0x80;
    REFUSED(q, "refused: pair scan");
    q = q0, q.opt.partition_mode = 2 | 0x100;  // (a bit the test does not mask: 0x8F)
    CHECK((int)choose_routed_layout(q).kind >= 0);
    for (int bit = 0; bit < 6; ++bit) {
      Pass1LayoutOptions o = q0.opt;
      if (bit == 0) o.narrow_keys = 0;
      if (bit == 1) o.narrow_chunk16 = 0;
      if (bit == 2) o.pass1_ws = 0;
      if (bit == 3) o.partition_layout = 2;
      if (bit == 4) o.partition_mode = 1;
      if (bit == 5) o.partition_mode = 0x82;
      CHECK(!pair_layout_fits(o, 256, planes != 0));
    }
  }

  // ---- agg.partition_block = 512: a budget of 79 KB, twice the producers ----
  {
    RoutedLayoutQuery q = query(512);
    q.opt.partition_block = 512, q.opt.partition_mode = 1;
    FLAVOUR(q, "sort", 2, 1, 512, 3584, 512, kStream, 0);
    {  // 1024 blocks: (80896 - 12376) / 20 = 3426 -> 3072 rows, fewer than four per partition: direct routing
      RoutedLayoutQuery q1 = query(1024);
      q1.opt.partition_block = 512;
      CHECK(partition_sort_capacity(2, 1024, 512, 80896) == 3072);
      FLAVOUR(q1, "direct", 2, 0, 1024, 0, 256, kStream, 0);
    }
    q.cu_count = 304;
    FLAVOUR(q, "sort", 2, 1, 512, 3584, 608, kStream, 0);
    q.cu_count = 600;
    FLAVOUR(q, "sort", 2, 1, 512, 3584, 1024, kStream, 0);
    q = query(256);
    q.opt.partition_block = 512;  // (the rings do not look at it)
    FLAVOUR(q, "ring16", 2, 2, 1024, 0, 256, kStream, 0);
  }
  // ---- agg.partition_producers: the five ring layouts honour it, sort and direct do not ----
  {
    RoutedLayoutQuery q = shared_query(256, 2);
    q.opt.partition_producers = 64;
    FLAVOUR(q, "shared_ring", 2, 2, 1024, 0, 64, kNarrow | kShared, 0);
    q = planes_query(2), q.opt.partition_producers = 64;
    FLAVOUR(q, "planes", 2, 2, 1024, 0, 64, kNarrow | kChunk16 | kWs | kShared | kPlanes, 8);
    q = pair_query(2), q.opt.partition_producers = 64;
    FLAVOUR(q, "pair_rows", 3, 2, 1024, 0, 64, kNarrow | kChunk16 | kWs | kPair, 8);
    q = narrow_query(), q.opt.partition_producers = 64;
    FLAVOUR(q, "ring16", 2, 2, 1024, 0, 64, kNarrow | kChunk16 | kWs | kStream, 8);
    q.opt.partition_producers = 4096;
    FLAVOUR(q, "ring16", 2, 2, 1024, 0, 1024, kNarrow | kChunk16 | kWs | kStream, 8);
    q = query(256, 2), q.opt.partition_producers = 64;
    FLAVOUR(q, "ring8", 3, 0x102, 1024, 0, 64, 0, 0);
    q = query(1024), q.opt.partition_producers = 64;
    FLAVOUR(q, "sort", 2, 1, 1024, 7168, 256, kStream, 0);
    q = query(2048), q.opt.partition_producers = 64;
    FLAVOUR(q, "direct", 2, 0, 1024, 0, 256, kStream, 0);
  }

  // ---- capacities.  256 x 256 regions: a batch of 2^20 rows is 16 rows per region, + 1; worst = 2 x that + 64, rounded up ----
  {
    struct Row {
      int log2_rows, defer;
      bool dense;
      uint32_t plain_cap, plain_worst, line_cap, line_worst, pair_cap, pair_worst;  // quanta of 64 / 320 / 60 rows
    };
    const Row rows[] = {
        // the window rule: as many batches as make up 2^27 rows, at most 8; agg.partition_defer: that many; dense scans: 1
        {20, 0, false, 1024, 128, 2560, 320, 960, 120},    // 98 rows -> 128 / 320 / 120, 8 batches
        {26, 0, false, 4352, 2176, 4480, 2240, 4320, 2160},  // 2 x 1025 + 64 = 2114 -> 2176 / 2240 / 2160, 2 batches
        {27, 0, false, 4224, 4224, 4480, 4480, 4200, 4200},  // 2 x 2049 + 64 = 4162 -> 4224 / 4480 / 4200, 1 batch
        {20, 1, false, 128, 128, 320, 320, 120, 120},
        {20, 4, false, 512, 128, 1280, 320, 480, 120},
        {26, 1, false, 2176, 2176, 2240, 2240, 2160, 2160},
        {26, 4, false, 8704, 2176, 8960, 2240, 8640, 2160},
        {27, 4, false, 16896, 4224, 17920, 4480, 16800, 4200},
        {20, 0, true, 128, 128, 320, 320, 120, 120},
        {26, 4, true, 2176, 2176, 2240, 2240, 2160, 2160},
    };
    for (const Row& w : rows) {
      RoutedLayoutQuery q = query();
      q.rows = (int64_t)1 << w.log2_rows, q.opt.partition_defer = w.defer, q.dense_seen = w.dense;
      CAPACITY(q, w.plain_cap, w.plain_worst);
      q = narrow_query();
      q.rows = (int64_t)1 << w.log2_rows, q.opt.partition_defer = w.defer, q.dense_seen = w.dense;
      CHECK(choose_routed_layout(q).PT.flags & kChunk16);
      CAPACITY(q, w.line_cap, w.line_worst);
      q = pair_query(2);
      q.rows = (int64_t)1 << w.log2_rows, q.opt.partition_defer = w.defer, q.dense_seen = w.dense;
      CAPACITY(q, w.pair_cap, w.pair_worst);
    }
    RoutedLayoutQuery q = query();  // 2^22 rows: 2 x 65 + 64 = 194 -> 256
    q.opt.partition_defer = 100;    // sixteen batches at the most
    CAPACITY(q, 4096, 256);
    q = query(1024);  // the sort: 256 x 1024 regions, 2 x 17 + 64 = 98 -> 128, 8 batches
    CAPACITY(q, 1024, 128);
    // agg.partition_cap_rows (tests: tiny regions): rounded up to the quantum, worst follows, no window
    const uint32_t asked[4] = {64, 100, 128, 640}, plain[4] = {64, 128, 128, 640}, line[4] = {320, 320, 320, 640}, pair[4] = {120, 120, 180, 660};
    for (int i = 0; i < 4; ++i) {
      q = query(), q.opt.partition_cap_rows = (int)asked[i], q.opt.partition_defer = 4;
      CAPACITY(q, plain[i], plain[i]);
      q = narrow_query(), q.opt.partition_cap_rows = (int)asked[i];
      CAPACITY(q, line[i], line[i]);
      q = pair_query(2), q.opt.partition_cap_rows = (int)asked[i];
      CAPACITY(q, pair[i], pair[i]);
    }
  }

  // ---- strides and bytes: 2^20 rows, 256 producers x 256 partitions, the three scratch layouts, agg.partition_pad = 0 and 100 ----
  {
    const size_t cnt = 262144;  // 4 x 256 x 256
    // 16-byte rows, 1024 per region: 2048 words, windows of 128; the pad: 12 words
    RoutedLayoutQuery q = query();
    q.rows = 1 << 20;
    GEOMETRY(q, 1024, 128, 2048, 524288, 128, 1073741824, cnt);  // producer-major: 256 regions of a producer side by side
    q.opt.partition_pad = 100;
    GEOMETRY(q, 1024, 128, 2048, 524300, 128, 1073766400, cnt);
    q.opt.partition_layout = 0;  // partition-major
    GEOMETRY(q, 1024, 128, 524300, 2048, 128, 1073766400, cnt);
    q.opt.partition_pad = 0;
    GEOMETRY(q, 1024, 128, 524288, 2048, 128, 1073741824, cnt);
    q.opt.partition_layout = 2;  // windowed: window w of the 256 partitions side by side, 16 windows per producer
    GEOMETRY(q, 1024, 128, 128, 524288, 32768, 1073741824, cnt);
    q.opt.partition_pad = 100;
    GEOMETRY(q, 1024, 128, 128, 524300, 32768, 1073766400, cnt);
    q.opt.partition_pad = -8;  // (negative: none)
    GEOMETRY(q, 1024, 128, 128, 524288, 32768, 1073741824, cnt);
    // LINE chunks, 2560 rows per region: 256 lines = 4096 words, trips of six lines = 96 words; the pad: whole lines, 16 words
    q = narrow_query();
    q.rows = 1 << 20;
    GEOMETRY(q, 2560, 320, 4096, 1048576, 96, 2147483648, cnt);
    q.opt.partition_pad = 100;
    GEOMETRY(q, 2560, 320, 4096, 1048592, 96, 2147516416, cnt);
    q.opt.partition_layout = 0;
    GEOMETRY(q, 2560, 320, 1048592, 4096, 96, 2147516416, cnt);
    q.opt.partition_pad = 0;
    GEOMETRY(q, 2560, 320, 1048576, 4096, 96, 2147483648, cnt);
    q.opt.partition_layout = 2;  // no LINE chunks in windows: 12-byte rows, 1024 per region = 1536 words, windows of 96
    GEOMETRY(q, 1024, 128, 96, 393216, 24576, 805306368, cnt);
    q.opt.partition_pad = 100;
    GEOMETRY(q, 1024, 128, 96, 393228, 24576, 805330944, cnt);
    // pair rows, 960 per region: 160 lines = 2560 words, trips of ten lines = 160 words
    q = pair_query(2);
    q.rows = 1 << 20;
    GEOMETRY(q, 960, 120, 2560, 655360, 160, 1342177280, cnt);
    q.opt.partition_pad = 100;
    GEOMETRY(q, 960, 120, 2560, 655376, 160, 1342210048, cnt);
    q.opt.partition_layout = 0;
    GEOMETRY(q, 960, 120, 655376, 2560, 160, 1342210048, cnt);
    q.opt.partition_pad = 0;
    GEOMETRY(q, 960, 120, 655360, 2560, 160, 1342177280, cnt);
    // fewer producers, more partitions: the counts
    q = query(512), q.opt.partition_block = 512, q.opt.partition_mode = 1;
    CHECK(choose_routed_layout(q).cnt_bytes == (size_t)4 * 512 * 512);
  }

  // ---- the properties, over the shapes of the tables above ----
  {
    std::vector<RoutedLayoutQuery> shapes;
    for (uint32_t parts : {1u, 64u, 256u, 512u, 1024u, 2048u, 4096u}) {
      shapes.push_back(query(parts));
      shapes.push_back(narrow_query(parts));
      shapes.push_back(query(parts, 2));
      shapes.push_back(query(parts, 3));
      shapes.push_back(shared_query(parts, 2));
      shapes.push_back(shared_query(parts, 3));
    }
    for (int na : {2, 3, 8}) shapes.push_back(pair_query(na)), shapes.push_back(planes_query(na));
    RoutedLayoutQuery q = narrow_query();
    q.skew_seen = true, shapes.push_back(q);
    q = narrow_query(), q.mostly_seen = true, shapes.push_back(q);
    q = narrow_query(), q.opt.partition_mode = 2 | 0x80, shapes.push_back(q);
    q = narrow_query(), q.opt.narrow_chunk16 = 0, shapes.push_back(q);
    q = query(512), q.opt.partition_block = 512, q.opt.partition_mode = 1, shapes.push_back(q);
    q = query(256), q.opt.partition_mode = 1, shapes.push_back(q);
    q = query(256), q.opt.partition_mode = 0, shapes.push_back(q);
    q = narrow_query(), q.kw = 2, shapes.push_back(q);
    const size_t n_base = shapes.size();
    for (size_t i = 0; i < n_base; ++i) {  // ... each with the capacities of the tables: other batch lengths, a window, tiny regions, fewer producers
      if ((uint32_t)(shapes[i].table_slots / shapes[i].block_slots) < 256) continue;  // (few regions: a 2^27-row batch makes them long, nothing else)
      q = shapes[i], q.rows = 1 << 18, shapes.push_back(q);
      q = shapes[i], q.rows = ((int64_t)1 << 27) - 12345, shapes.push_back(q);
      q = shapes[i], q.rows = 1 << 26, q.opt.partition_defer = 4, shapes.push_back(q);
      for (int cap : {64, 100, 640}) q = shapes[i], q.opt.partition_cap_rows = cap, shapes.push_back(q);
      q = shapes[i], q.opt.partition_producers = 64, q.cu_count = 304, shapes.push_back(q);
    }
    int seen[7] = {};
    for (const RoutedLayoutQuery& s : shapes) {
      const RoutedLayout r = choose_routed_layout(s);
      CHECK((int)r.kind >= 0);
      if ((int)r.kind >= 0) ++seen[(int)r.kind];
      properties(s);
    }
    for (int i = 0; i < kLayouts; ++i) CHECK(seen[i] > 0);  // every layout is reached
    // the launch predicate itself: what launch_partition refuses
    DevPartition p = choose_routed_layout(query(1024)).PT;  // the sort
    CHECK(partition_launchable(p));
    DevPartition bad = p;
    bad.stage_rows = 0;
    CHECK(!partition_launchable(bad));
    bad = p, bad.stage_rows = 8193;
    CHECK(!partition_launchable(bad));
    bad = p, bad.block = 256;
    CHECK(!partition_launchable(bad));
    bad = p, bad.n_parts = 4097;
    CHECK(!partition_launchable(bad));
    bad = p, bad.n_words = 3;  // 7168 x 28 + 1024 x 12 + 88 = 213080 bytes
    CHECK(!partition_launchable(bad));
    p = choose_routed_layout(query(4096)).PT;  // direct: 4 bytes per partition + 16, 64 KB at the most
    CHECK(partition_stage_bytes(p) == 16400 && partition_launchable(p));
    bad = p, bad.n_parts = 16381;
    CHECK(!partition_launchable(bad));
    p = choose_routed_layout(narrow_query()).PT;  // rings: 160 KB
    CHECK(partition_stage_bytes(p) == 138432 && partition_launchable(p));
    bad = p, bad.n_parts = 512;
    CHECK(!partition_launchable(bad));
    bad.flags &= ~PTF_WS;  // (what select_pass1 does for the run-time decoded shapes: the ring kernel's bytes, three line slots)
    bad.n_parts = 256;
    CHECK(partition_stage_bytes(bad) == 148544 && partition_launchable(bad));
  }

  if (failures) {
    printf("%d failure(s)\n", failures);
    return 1;
  }
  printf("ok: %d layouts, %ld cells of the region properties\n", kLayouts, property_cells);
  return 0;
}
