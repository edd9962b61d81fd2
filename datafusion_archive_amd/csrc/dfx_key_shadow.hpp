// dfx_key_shadow.hpp -- the Int32 shadow of a resident Int64 key column: when it is built, when it is
// refused, and the memory rule.  Host only and free of HIP: the device work comes in through KeyShadowDevice, so the rule
// runs under a sanitizer with the device stubbed (tests/native/key_shadow_rule.cpp).
//
// A resident table is immutable.  A GROUP BY whose key is a plain null-free Int64 column of it, on the narrow partitioned
// strategy, reads 16 bytes per row in pass 1 of which 4 are the upper halves of keys that are all below 2^32.  The table
// therefore may own, per such column, a 4-byte copy made ONCE: by the second query that qualifies (agg.key_shadow = -1; a
// table queried once never pays), or by the first (= 1).  The copy is made from the WHOLE column and OR-reduces the dropped
// halves: a non-zero result (a key >= 2^32, or negative) frees the copy and marks the column for good.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <functional>
#include <memory>
#include <mutex>
#include <vector>

namespace dfx {

struct KeyShadowDevice {
  std::function<size_t()> free_bytes;                       // device memory that an allocation can still have
  std::function<std::shared_ptr<void>(size_t)> alloc;       // null: not to be had (no retry, nothing trimmed for it)
  // narrows rows keys from src into dst on the query's stream and returns the OR of the dropped upper halves in *dropped;
  // false: the device refused (the attempt is dropped, the column stays eligible)
  std::function<bool(const void* src, int64_t rows, void* dst, uint32_t* dropped)> narrow;
};

constexpr size_t kKeyShadowPad = 64;  // bytes behind the last key: the scanners' pair loads read one key past an odd row count

struct KeyShadow {
  const void* base = nullptr;    // the Int64 column's values (16-byte aligned) and its row count
  int64_t rows = 0;
  int queries = 0;               // qualifying queries that asked so far (saturates at 2)
  bool refused = false;          // the whole column was looked at: some key has no 32-bit form.  Never tried again
  std::shared_ptr<void> narrow;  // rows x 4 bytes + kKeyShadowPad
};

class KeyShadows {
 public:
  // a null-free Int64 column of the table being made (before any scan can ask)
  void add_column(const void* values, int64_t rows) {
    if (!values || rows <= 0 || ((uintptr_t)values & 15u)) return;
    KeyShadow k;
    k.base = values;
    k.rows = rows;
    cols_.push_back(std::move(k));
  }
  // The shadow words of the key rows that start at `values` (a slice of a registered column), or null.
  // first_ask: this is the query's first question about this column -- it counts, and it alone may build.
  // option: agg.key_shadow (-1 auto: the second qualifying query builds; 0 never; 1 the first builds).
  // query_bytes: what the asking aggregate holds for its routing scratch, spill list and table; after the copy's rows x 4 bytes
  // at least as much must still be free (the next query of this shape allocates the same again while this one's result lives).
  const uint32_t* acquire(const void* values, int option, bool first_ask, size_t query_bytes, const KeyShadowDevice& dev, bool* built) {
    if (built) *built = false;
    if (option == 0 || !values) return nullptr;
    // One lock for the table's columns, held across the build (allocation, one kernel of ~2.7 ms per 10^9 rows, the read-back of
    // the dropped-halves word): queries of other threads on this table wait for it once, and then find the copy instead of
    // making a second one.  Nothing else is ever done under it.
    std::lock_guard<std::mutex> lk(mu_);
    KeyShadow* k = nullptr;
    for (KeyShadow& c : cols_) {
      const uint8_t* b = (const uint8_t*)c.base;
      if ((const uint8_t*)values >= b && (const uint8_t*)values < b + (size_t)c.rows * 8) k = &c;
    }
    if (!k || k->refused) return nullptr;
    const size_t off = (size_t)((const uint8_t*)values - (const uint8_t*)k->base);
    if (off & 511u) return nullptr;  // (slices start on multiples of 64 rows: the shadow words stay 8-byte aligned, pairs whole)
    if (first_ask && k->queries < 2) ++k->queries;  // (saturates: only "the second" matters)
    if (!k->narrow && first_ask && (option > 0 || k->queries >= 2)) {
      const size_t bytes = (size_t)k->rows * 4 + kKeyShadowPad;
      const size_t free_now = dev.free_bytes();
      if (free_now < bytes || free_now - bytes < query_bytes) return nullptr;  // memory is short: silently, asked again by the next query
      std::shared_ptr<void> copy = dev.alloc(bytes);
      if (!copy) return nullptr;
      uint32_t dropped = 0;
      if (!dev.narrow(k->base, k->rows, copy.get(), &dropped)) return nullptr;
      if (dropped != 0) {
        k->refused = true;  // (copy freed on return)
        return nullptr;
      }
      k->narrow = std::move(copy);
      if (built) *built = true;
    }
    if (!k->narrow) return nullptr;
    return (const uint32_t*)k->narrow.get() + off / 8;
  }
  // ... as they stand: the words if the copy exists, null otherwise.  Counts nothing, builds nothing.
  const uint32_t* peek(const void* values) const {
    if (!values) return nullptr;
    std::lock_guard<std::mutex> lk(mu_);
    for (const KeyShadow& c : cols_) {
      const uint8_t* b = (const uint8_t*)c.base;
      if ((const uint8_t*)values < b || (const uint8_t*)values >= b + (size_t)c.rows * 8) continue;
      const size_t off = (size_t)((const uint8_t*)values - b);
      if (c.refused || !c.narrow || (off & 511u)) return nullptr;
      return (const uint32_t*)c.narrow.get() + off / 8;
    }
    return nullptr;
  }
  // the registered column that holds `values`: its base, *rows its length, *row the row `values` is (null: none)
  const void* column_of(const void* values, int64_t* rows, int64_t* row) const {
    if (!values) return nullptr;
    std::lock_guard<std::mutex> lk(mu_);
    for (const KeyShadow& c : cols_) {
      const uint8_t* b = (const uint8_t*)c.base;
      if ((const uint8_t*)values < b || (const uint8_t*)values >= b + (size_t)c.rows * 8) continue;
      *rows = c.rows;
      *row = (int64_t)(((const uint8_t*)values - b) / 8);
      return c.base;
    }
    return nullptr;
  }
  size_t bytes_held() const {
    std::lock_guard<std::mutex> lk(mu_);
    size_t b = 0;
    for (const KeyShadow& c : cols_)
      if (c.narrow) b += (size_t)c.rows * 4 + kKeyShadowPad;
    return b;
  }
  // (tests) state of the column that holds `values`: -1 unknown, 0 nothing built, 1 built, 2 refused; *queries: askers so far
  int state_of(const void* values, int* queries = nullptr) const {
    std::lock_guard<std::mutex> lk(mu_);
    for (const KeyShadow& c : cols_)
      if (c.base == values) {
        if (queries) *queries = c.queries;
        return c.refused ? 2 : c.narrow ? 1 : 0;
      }
    return -1;
  }

 private:
  mutable std::mutex mu_;
  std::vector<KeyShadow> cols_;
};

}  // namespace dfx
