// dfx_routed_shadow.hpp -- the ROUTED shadow of a resident table's (key column, operand column) pair: pass 1's
// unfiltered output, kept.  Which partition a row is routed to is a function of its key alone, so for a table that is queried again
// with the same GROUP BY key and the same operand -- any predicate on the operand, or none -- the routing is the same work every
// time.  The shadow keeps it: windows of W consecutive rows (agg.routed_shadow_window_rows, 2^27; the last window holds the table's
// tail; a table shorter than W has none), each with regions and counts in exactly the layout a dense PTF_ROW8 | PTF_NARROW | PTF_CHUNK16 pass 1 leaves -- producer-
// major, 8-byte rows {hash image, Float32 bits of the raw operand}, sixteen to a line, partial chunks padded with kTagEmpty,
// counts[partition x producers + producer] -- and the geometry it was routed for.  A launch whose rows are exactly one window then
// is ONE kernel (Pass2Rows::narrow8_pred, dfx_k_pass2.hip) that reads the window and evaluates the predicate itself.
// Who reads it: only a launch that would bind BOTH column shadows itself (launch_rows asks both_shadows_bind before routed_shadow_launch).
// So agg.key_shadow = 0, agg.value_shadow = 0 and agg.routed_row8 = 0 each switch the reads off for that query exactly as
// agg.routed_shadow = 0 does -- the two passes run over the 8-byte columns -- and none of them frees or rebuilds anything: the next
// query under -1 / 1 scans the same windows again.  A pair is built once: a shadow routed for another table geometry than later
// queries ask with (agg.capacity_log2) stays and serves none of them.  tests/test_gpu_table_query_sequences.py flips each option
// on a table that holds the shadow.
// Host only and free of HIP, like dfx_key_shadow.hpp, whose rules these are: the option -1 / 0 / 1, the memory rule on the shadow's
// full size, one lock per table held across the build, silent drops, refusal for good.  The device work comes in through
// RoutedShadowDevice: tests/native/routed_shadow_rule.cpp runs the rule with the device stubbed, under the host sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <functional>
#include <memory>
#include <mutex>
#include <vector>

namespace dfx {

// What a window was routed for: the regions' layout (DevPartition's fields, pointers aside) and the table geometry that maps a
// hash image to a partition -- slot = image >> (shift - 32), partition = slot / block_slots.
struct RoutedGeometry {
  uint32_t n_parts = 0, n_producers = 0, cap_rows = 0, n_words = 0, part_shift = 0, flags = 0;
  uint64_t part_stride = 0, prod_stride = 0, win_stride = 0;
  int32_t shift = 0;         // the table's
  uint32_t block_slots = 0;  // slots of a table block
  // the query's table maps images to partitions as the window's did
  bool serves(int32_t table_shift, uint32_t table_block_slots, uint32_t table_parts) const {
    return n_parts != 0 && shift == table_shift && block_slots == table_block_slots && n_parts == table_parts;
  }
};
struct RoutedWindowLayout {
  RoutedGeometry g;
  size_t region_bytes = 0, count_bytes = 0;
};
struct RoutedWindow {
  int64_t row0 = 0, rows = 0;  // the table rows it holds
  RoutedGeometry g;
  std::shared_ptr<void> regions, counts;
};

struct RoutedShadowDevice {
  std::function<size_t()> free_bytes;                  // device memory that an allocation can still have
  std::function<std::shared_ptr<void>(size_t)> alloc;  // null: not to be had
  std::function<RoutedWindowLayout(int64_t rows)> layout;  // the dense 8-byte layout of a window of `rows` rows (n_parts == 0: there is none)
  // routes rows [row0, row0 + rows) of both column shadows into the window's regions; false: the device refused (dropped)
  std::function<bool(int64_t row0, int64_t rows, const RoutedGeometry& g, void* regions, void* counts)> route;
  // after the last window: the build's control block, read once.  *spilled: rows that found no place in a region (a reserved image,
  // a region overflow); *error: its error word.  false: the device refused
  std::function<bool(uint64_t* spilled, uint32_t* error)> finish;
};

constexpr int64_t kRoutedWindowRows = (int64_t)1 << 27;

class RoutedShadows {
 public:
  // The end of a query (after its last batch) over the columns `keys` / `values` (their bases: `rows` rows each).  option:
  // agg.routed_shadow (-1 auto: a query that bound the operand's shadow in at least one pass-1 launch builds -- bound_value_shadow --;
  // 0 never; 1: the first query that qualifies).  window_rows: W, a multiple of 64.  query_bytes: what the asking aggregate holds;
  // after the build at least that much PLUS the shadow's own size must still be free.  true: built here.
  bool build(const void* keys, const void* values, int64_t rows, int option, bool bound_value_shadow, int64_t window_rows, size_t query_bytes,
             const RoutedShadowDevice& dev) {
    if (option == 0 || !keys || !values || rows <= 0 || window_rows < 64 || (window_rows & 63)) return false;
    if (option < 0 && !bound_value_shadow) return false;
    // A table shorter than one window is not shadowed: a window's regions have a fixed floor (every producer x partition region holds
    // at least one 64-row trip: 33 MB at 256 x 256) whatever the table holds, and such a table is one launch of each pass anyway.
    if (rows < window_rows) return false;
    std::lock_guard<std::mutex> lk(mu_);  // (one lock per table, held across the build: other queries wait once and then find the shadow)
    Pair* p = find(keys, values);
    if (!p) {
      pairs_.push_back(Pair());
      p = &pairs_.back();
      p->keys = keys, p->values = values, p->rows = rows;
    }
    if (p->refused || !p->windows.empty() || p->rows != rows) return false;
    std::vector<RoutedWindow> ws;
    std::vector<RoutedWindowLayout> ls;
    size_t bytes = 0;
    for (int64_t at = 0; at < rows; at += window_rows) {
      RoutedWindow w;
      w.row0 = at, w.rows = rows - at < window_rows ? rows - at : window_rows;
      const RoutedWindowLayout l = dev.layout(w.rows);
      if (l.g.n_parts == 0 || l.region_bytes == 0 || l.count_bytes == 0) return false;  // (no such layout for this table: asked again by the next query)
      w.g = l.g;
      bytes += l.region_bytes + l.count_bytes;
      ws.push_back(w);
      ls.push_back(l);
    }
    const size_t free_now = dev.free_bytes();
    if (free_now < bytes || free_now - bytes < query_bytes || free_now - bytes - query_bytes < bytes) return false;  // memory is short: silently
    for (size_t i = 0; i < ws.size(); ++i) {
      ws[i].regions = dev.alloc(ls[i].region_bytes);
      ws[i].counts = ws[i].regions ? dev.alloc(ls[i].count_bytes) : nullptr;
      if (!ws[i].regions || !ws[i].counts) return false;  // (what was allocated is freed on return)
    }
    for (RoutedWindow& w : ws)
      if (!dev.route(w.row0, w.rows, w.g, w.regions.get(), w.counts.get())) return false;
    uint64_t spilled = 0;
    uint32_t error = 0;
    if (!dev.finish(&spilled, &error)) return false;
    if (spilled != 0 || error != 0) {
      p->refused = true;  // skewed keys, a reserved image: this pair keeps the two-pass path for good (the memory is freed on return)
      return false;
    }
    p->windows = std::move(ws);
    p->window_rows = window_rows;
    p->bytes = bytes;
    return true;
  }
  // The window that holds EXACTLY the rows [row0, row0 + n) of the pair -- a slice off the window grid, a part of a window, finds
  // none -- and was routed for this table geometry.  Copies it out (the buffers stay alive while the copy does).
  bool bind(const void* keys, const void* values, int64_t row0, int64_t n, int option, int32_t table_shift, uint32_t table_block_slots,
            uint32_t table_parts, RoutedWindow* out) const {
    if (option == 0 || !keys || !values || n <= 0) return false;
    std::lock_guard<std::mutex> lk(mu_);
    const Pair* p = find(keys, values);
    if (!p || p->refused || p->windows.empty() || row0 % p->window_rows != 0) return false;
    const size_t i = (size_t)(row0 / p->window_rows);
    if (i >= p->windows.size()) return false;
    const RoutedWindow& w = p->windows[i];
    if (w.row0 != row0 || w.rows != n || !w.g.serves(table_shift, table_block_slots, table_parts)) return false;
    *out = w;
    return true;
  }
  // W of the pair's shadow if it is built (a scan then asks for launches of whole windows), 0 otherwise
  int64_t window_rows_of(const void* keys, const void* values) const {
    std::lock_guard<std::mutex> lk(mu_);
    const Pair* p = find(keys, values);
    return (p && !p->refused && !p->windows.empty()) ? p->window_rows : 0;
  }
  size_t bytes_held() const {
    std::lock_guard<std::mutex> lk(mu_);
    size_t b = 0;
    for (const Pair& p : pairs_) b += p.windows.empty() ? 0 : p.bytes;
    return b;
  }
  // (tests) -1 unknown pair, 0 nothing built, 1 built, 2 refused; *windows: how many
  int state_of(const void* keys, const void* values, int* windows = nullptr) const {
    std::lock_guard<std::mutex> lk(mu_);
    const Pair* p = find(keys, values);
    if (!p) return -1;
    if (windows) *windows = (int)p->windows.size();
    return p->refused ? 2 : !p->windows.empty() ? 1 : 0;
  }

 private:
  struct Pair {
    const void* keys = nullptr;    // the columns' bases
    const void* values = nullptr;
    int64_t rows = 0, window_rows = 0;
    bool refused = false;          // a build saw a spilled row.  Never tried again
    size_t bytes = 0;
    std::vector<RoutedWindow> windows;
  };
  Pair* find(const void* keys, const void* values) {
    for (Pair& p : pairs_)
      if (p.keys == keys && p.values == values) return &p;
    return nullptr;
  }
  const Pair* find(const void* keys, const void* values) const { return const_cast<RoutedShadows*>(this)->find(keys, values); }
  mutable std::mutex mu_;
  std::vector<Pair> pairs_;
};

}  // namespace dfx
