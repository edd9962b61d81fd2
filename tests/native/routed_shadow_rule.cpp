// routed_shadow_rule.cpp -- the decision rule of a table's routed shadow (csrc/dfx_routed_shadow.hpp) and the choice of pass 2's scan
// form (choose_pass2_scan, csrc/dfx_pass2_forms.hpp) as a stand-alone program, with the device stubbed: the option's three values,
// the build point (a query that bound the operand's shadow), the memory rule on both sides of its edge, silent drops, the refusal
// for good after a spilled row, bind / no-bind for aligned and unaligned slices, the tail window, a geometry mismatch and a second
// column pair.  tests/test_routed_shadow_host.py builds it plain and with -fsanitize=address,undefined.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../datafusion_archive_amd/csrc/dfx_pass2_forms.hpp"
#include "../../datafusion_archive_amd/csrc/dfx_routed_shadow.hpp"

using namespace dfx;

static int failures = 0;
#define CHECK(cond)                                    \
  do {                                                 \
    if (!(cond)) {                                     \
      printf("FAILED line %d: %s\n", __LINE__, #cond); \
      ++failures;                                      \
    }                                                  \
  } while (0)

constexpr int32_t kShift = 43;       // a table of 2^21 slots
constexpr uint32_t kBlock = 8192;    // ... in 256 blocks
constexpr uint32_t kParts = 256;
constexpr size_t kCountBytes = 4 * 256 * 4;  // 256 partitions x 4 producers

struct StubDevice {  // host memory stands in for HBM; "routing" records what it was asked for
  size_t free_now = 0;
  int allocs = 0, routes = 0, finishes = 0, fail_allocs = 0;
  bool refuse_route = false, refuse_finish = false, no_layout = false;
  uint64_t spilled = 0;
  uint32_t error = 0;
  int64_t routed_rows = 0;
  static size_t region_bytes(int64_t rows) { return (size_t)rows * 16; }  // (regions hold twice the average)
  RoutedShadowDevice ops() {
    RoutedShadowDevice d;
    d.free_bytes = [this]() { return free_now; };
    d.alloc = [this](size_t bytes) -> std::shared_ptr<void> {
      if (fail_allocs > 0) {
        --fail_allocs;
        return nullptr;
      }
      ++allocs;
      return std::shared_ptr<void>(malloc(bytes), free);
    };
    d.layout = [this](int64_t rows) {
      RoutedWindowLayout l;
      if (no_layout) return l;
      l.g.n_parts = kParts, l.g.n_producers = 4, l.g.cap_rows = (uint32_t)(rows / 512 + 64), l.g.n_words = 2, l.g.part_shift = 13;
      l.g.flags = PTF_NARROW | PTF_CHUNK16 | PTF_WS | PTF_ROW8;
      l.g.part_stride = l.g.cap_rows, l.g.prod_stride = (uint64_t)kParts * l.g.cap_rows, l.g.win_stride = 64;
      l.g.shift = kShift, l.g.block_slots = kBlock;
      l.region_bytes = region_bytes(rows), l.count_bytes = kCountBytes;
      return l;
    };
    d.route = [this](int64_t row0, int64_t rows, const RoutedGeometry& g, void* regions, void* counts) -> bool {
      if (refuse_route) return false;
      ++routes;
      routed_rows += rows;
      memset(regions, 0xFF, region_bytes(rows));  // (the whole allocation is the window's)
      memset(counts, 0, kCountBytes);
      return g.n_parts == kParts && row0 >= 0;
    };
    d.finish = [this](uint64_t* sp, uint32_t* err) -> bool {
      if (refuse_finish) return false;
      ++finishes;
      *sp = spilled, *err = error;
      return true;
    };
    return d;
  }
};

static size_t shadow_bytes(int64_t rows, int64_t w) {
  size_t b = 0;
  for (int64_t at = 0; at < rows; at += w) b += StubDevice::region_bytes(rows - at < w ? rows - at : w) + kCountBytes;
  return b;
}

int main() {
  const int64_t W = 1 << 16;
  const int64_t rows = 3 * W + 1000 + 37;  // three windows and a tail
  static uint64_t keys[8], values[8], other[8];  // (the rule only compares the columns' bases)
  const size_t bytes = shadow_bytes(rows, W);
  RoutedWindow w;
  {  // the option: 0 never builds and never binds; -1 builds only for a query that bound the operand's shadow; 1 builds
    RoutedShadows rs;
    StubDevice dev;
    dev.free_now = (size_t)1 << 30;
    CHECK(!rs.build(keys, values, rows, 0, true, W, 0, dev.ops()) && dev.allocs == 0 && rs.state_of(keys, values) == -1);
    CHECK(!rs.build(keys, values, rows, -1, false, W, 0, dev.ops()) && dev.allocs == 0 && dev.routes == 0);
    CHECK(rs.build(keys, values, rows, -1, true, W, 0, dev.ops()));
    int n_windows = 0;
    CHECK(rs.state_of(keys, values, &n_windows) == 1 && n_windows == 4 && dev.routes == 4 && dev.finishes == 1 && dev.allocs == 8);
    CHECK(dev.routed_rows == rows && rs.bytes_held() == bytes && rs.window_rows_of(keys, values) == W);
    CHECK(!rs.build(keys, values, rows, -1, true, W, 0, dev.ops()) && dev.routes == 4);  // once
    CHECK(!rs.build(keys, values, rows, 1, true, W, 0, dev.ops()) && dev.routes == 4);
    // bind: exactly one window, on the grid, for the geometry it was routed for
    CHECK(rs.bind(keys, values, 0, W, -1, kShift, kBlock, kParts, &w) && w.row0 == 0 && w.rows == W && w.regions && w.counts && w.g.n_producers == 4);
    CHECK(rs.bind(keys, values, 2 * W, W, 1, kShift, kBlock, kParts, &w) && w.row0 == 2 * W);
    CHECK(rs.bind(keys, values, 3 * W, 1037, -1, kShift, kBlock, kParts, &w) && w.rows == 1037);  // the tail window
    CHECK(!rs.bind(keys, values, 3 * W, 1000, -1, kShift, kBlock, kParts, &w));                    // ... but not a part of it
    CHECK(!rs.bind(keys, values, 0, W, 0, kShift, kBlock, kParts, &w));                            // the option says never: not even read
    CHECK(!rs.bind(keys, values, 64, W, -1, kShift, kBlock, kParts, &w));                          // off the grid
    CHECK(!rs.bind(keys, values, 0, W - 64, -1, kShift, kBlock, kParts, &w));                      // a part of a window
    CHECK(!rs.bind(keys, values, 0, 2 * W, -1, kShift, kBlock, kParts, &w));                       // two windows
    CHECK(!rs.bind(keys, values, 4 * W, W, -1, kShift, kBlock, kParts, &w));                       // past the table
    CHECK(!rs.bind(keys, values, 0, W, -1, kShift - 2, kBlock, 4 * kParts, &w));                   // a table that grew
    CHECK(!rs.bind(keys, values, 0, W, -1, kShift, kBlock / 2, 2 * kParts, &w));                   // another block size
    CHECK(!rs.bind(keys, other, 0, W, -1, kShift, kBlock, kParts, &w));                            // another operand column
    CHECK(!rs.bind(nullptr, values, 0, W, -1, kShift, kBlock, kParts, &w));
    // a second pair of the same table: its own shadow
    CHECK(rs.state_of(keys, other) == -1 && rs.window_rows_of(keys, other) == 0);
    CHECK(rs.build(keys, other, rows, 1, true, 2 * W, 0, dev.ops()) && rs.window_rows_of(keys, other) == 2 * W);
    CHECK(rs.bind(keys, other, 2 * W, rows - 2 * W, -1, kShift, kBlock, kParts, &w) && !rs.bind(keys, other, W, W, -1, kShift, kBlock, kParts, &w));
    CHECK(rs.bind(keys, values, W, W, -1, kShift, kBlock, kParts, &w) && rs.bytes_held() == bytes + shadow_bytes(rows, 2 * W));
  }
  {  // the memory rule on both sides of its edge: after the build as much must stay free as the query holds PLUS the shadow itself
    RoutedShadows rs;
    StubDevice dev;
    const size_t query = 5000;
    dev.free_now = 2 * bytes + query - 1;
    CHECK(!rs.build(keys, values, rows, 1, true, W, query, dev.ops()) && dev.allocs == 0 && rs.state_of(keys, values) == 0);
    dev.free_now = bytes - 1;
    CHECK(!rs.build(keys, values, rows, 1, true, W, 0, dev.ops()) && dev.allocs == 0);
    dev.free_now = 2 * bytes + query;  // (dropped silently: the next query asks again)
    CHECK(rs.build(keys, values, rows, 1, true, W, query, dev.ops()) && rs.state_of(keys, values) == 1);
  }
  {  // silent drops: an allocation that fails, a device that refuses, a table without the layout -- the pair stays eligible
    RoutedShadows rs;
    StubDevice dev;
    dev.free_now = (size_t)1 << 30;
    dev.fail_allocs = 1;
    CHECK(!rs.build(keys, values, rows, 1, true, W, 0, dev.ops()) && rs.state_of(keys, values) == 0 && rs.bytes_held() == 0);
    dev.refuse_route = true;
    CHECK(!rs.build(keys, values, rows, 1, true, W, 0, dev.ops()) && rs.state_of(keys, values) == 0);
    dev.refuse_route = false, dev.refuse_finish = true;
    CHECK(!rs.build(keys, values, rows, 1, true, W, 0, dev.ops()) && rs.state_of(keys, values) == 0);
    dev.refuse_finish = false, dev.no_layout = true;
    CHECK(!rs.build(keys, values, rows, 1, true, W, 0, dev.ops()) && rs.state_of(keys, values) == 0);
    dev.no_layout = false;
    CHECK(!rs.build(keys, values, rows, 1, true, 100, 0, dev.ops()) && !rs.build(keys, values, rows, 1, true, 0, 0, dev.ops()));  // (W: a multiple of 64)
    CHECK(rs.build(keys, values, rows, 1, true, W, 0, dev.ops()) && !rs.bind(keys, values, 0, W, -1, kShift, kBlock, kParts + 1, &w));
  }
  for (int which = 0; which < 2; ++which) {  // one spilled row (or an error): refused for good, the memory freed, never tried again
    RoutedShadows rs;
    StubDevice dev;
    dev.free_now = (size_t)1 << 30;
    dev.spilled = which == 0 ? 1 : 0;
    dev.error = which == 0 ? 0 : 4;
    CHECK(!rs.build(keys, values, rows, 1, true, W, 0, dev.ops()) && rs.state_of(keys, values) == 2 && rs.bytes_held() == 0 && dev.routes == 4);
    dev.spilled = 0, dev.error = 0;
    CHECK(!rs.build(keys, values, rows, 1, true, W, 0, dev.ops()) && dev.routes == 4 && rs.state_of(keys, values) == 2);
    CHECK(!rs.bind(keys, values, 0, W, -1, kShift, kBlock, kParts, &w) && rs.window_rows_of(keys, values) == 0);
    CHECK(rs.build(keys, other, rows, 1, true, W, 0, dev.ops()));  // (the other pair is its own)
  }
  {  // a table of exactly one window is served; a table shorter than a window is not shadowed
    RoutedShadows rs;
    StubDevice dev;
    dev.free_now = (size_t)1 << 30;
    int n_windows = 0;
    CHECK(rs.build(keys, values, W, -1, true, W, 0, dev.ops()) && rs.state_of(keys, values, &n_windows) == 1 && n_windows == 1);
    CHECK(rs.bind(keys, values, 0, W, -1, kShift, kBlock, kParts, &w) && !rs.bind(keys, values, W, 64, -1, kShift, kBlock, kParts, &w));
    CHECK(!rs.build(other, values, W - 64, 1, true, W, 0, dev.ops()) && !rs.build(other, values, 40, -1, true, W, 0, dev.ops()));
    CHECK(rs.state_of(other, values) == -1 && !rs.bind(other, values, 0, 40, -1, kShift, kBlock, kParts, &w) && dev.routes == 1);
  }
  {  // choose_pass2_scan against a table written out by hand: {flags, na, kw, sum, slots, producers, line, np, m0, inv0, m1, inv1} -> scan, LDS
    const uint32_t R8 = PTF_NARROW | PTF_CHUNK16 | PTF_WS | PTF_ROW8;
    const size_t lds = 8192 * 12 + 16 * 128 * 12 + 16 * 192 * 8;
    CHECK(lds == 147456 && lds <= kP2LdsLimit && pass2_scan_lds_bytes(8192) == lds);
    struct Case {
      uint32_t flags;
      int na, kw;
      bool sum;
      uint32_t slots, producers;
      bool line;
      uint32_t np, m0, inv0, m1, inv1;
      int scan;  // -2: refused
    };
    const Case cases[] = {
        {R8, 1, 1, true, 8192, 256, true, 0, 0, 0, 0, 0, kP2ScanAll},
        {R8, 1, 1, true, 8192, 256, true, 2, 4, 0, 1, 0, 4 | (1 << 3)},  // x >  a AND x <  b
        {R8, 1, 1, true, 8192, 256, true, 2, 6, 0, 1, 0, 6 | (1 << 3)},  // x >= a AND x <  b
        {R8, 1, 1, true, 8192, 256, true, 2, 4, 0, 3, 0, 4 | (3 << 3)},  // x >  a AND x <= b
        {R8, 1, 1, true, 8192, 256, true, 2, 6, 0, 3, 0, 6 | (3 << 3)},  // x >= a AND x <= b
        {R8, 1, 1, true, 8192, 256, true, 2, 1, 0, 4, 0, kP2ScanRuntime},  // the terms the other way round
        {R8, 1, 1, true, 8192, 256, true, 2, 2, 1, 1, 0, kP2ScanRuntime},  // x != a
        {R8, 1, 1, true, 8192, 256, true, 2, 4, 0, 7, 0, kP2ScanRuntime},  // (a term that passes everything: an open side)
        {R8 | PTF_STREAM_PASS2, 1, 1, true, 4096, 1024, true, 2, 4, 0, 1, 0, 4 | (1 << 3)},
        {R8, 1, 1, true, 8192, 256, true, 1, 4, 0, 0, 0, -2},   // one term: no such signature
        {R8, 1, 1, true, 8192, 256, true, 3, 4, 0, 1, 0, -2},
        {R8, 2, 1, true, 8192, 256, true, 0, 0, 0, 0, 0, -2},   // two aggregates
        {R8, 1, 2, true, 8192, 256, true, 0, 0, 0, 0, 0, -2},   // two key words
        {R8, 1, 1, false, 8192, 256, true, 0, 0, 0, 0, 0, -2},  // MIN / MAX / COUNT
        {R8 & ~PTF_ROW8, 1, 1, true, 8192, 256, true, 0, 0, 0, 0, 0, -2},  // 12-byte rows
        {R8 | PTF_SHARED, 1, 1, true, 8192, 256, true, 0, 0, 0, 0, 0, -2},
        {R8 | PTF_PAIR, 1, 1, true, 8192, 256, true, 0, 0, 0, 0, 0, -2},
        {R8, 1, 1, true, 8192, 256, false, 0, 0, 0, 0, 0, -2},  // not the whole-line geometry
        {R8, 1, 1, true, 8192, 1025, true, 0, 0, 0, 0, 0, -2},  // more producers than a wave's lanes x 16
        {R8, 1, 1, true, 16384, 256, true, 0, 0, 0, 0, 0, -2},  // a block that does not fit the LDS
        {R8, 1, 1, true, 6000, 256, true, 0, 0, 0, 0, 0, -2},
    };
    for (const Case& c : cases) {
      const Pass2ScanChoice got = choose_pass2_scan(c.flags, c.na, c.kw, c.sum, c.slots, c.producers, c.line, c.np, c.m0, c.inv0, c.m1, c.inv1);
      if (c.scan == -2) {
        CHECK(got.rows != Pass2Rows::narrow8_pred && got.scan == kP2ScanNone && got.lds_bytes == 0);
      } else {
        CHECK(got.rows == Pass2Rows::narrow8_pred && got.scan == c.scan);
        CHECK(got.lds_bytes == (size_t)c.slots * 12 + 16 * 128 * 12 + 16 * 192 * 8);
      }
    }
    // the existing forms are what they were: 8-byte rows through choose_pass2 are narrow8, never the scan
    const Pass2Choice old = choose_pass2(R8, 1, 1, 2, 8192, 256, 0, true);
    CHECK(old.form == Pass2Form::narrow && old.launch[0].rows == Pass2Rows::narrow8 && old.lds_bytes == 8192 * 12 + 16 * 128 * 12);
  }
  if (failures) return 1;
  printf("ok: routed shadow rule\n");
  return 0;
}
