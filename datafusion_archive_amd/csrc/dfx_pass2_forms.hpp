// dfx_pass2_forms.hpp -- pass 2 of the partitioned GROUP BY: THE list of its forms and which one a launch takes.
// choose_pass2 is everything launch_partition_agg (dfx_k_pass2.hip) decides before it launches: the form or a refusal, the
// dynamic LDS bytes, the number of launches and what each is launched with.  A new form is one name here, its place in
// choose_pass2 and its case in launch_partition_agg.
// Host only and free of HIP: tests/native/pass2_forms_check.cpp holds choose_pass2 against a table written out by hand.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "dfx_device.hpp"

namespace dfx {

// flat_*: k_partition_agg, the producers' rows as one flattened index space (one 16-byte value / any row width).  The others are
// k_partition_agg_lean, a wave per region: stream_wide 16-byte rows and keys in LDS; narrow 12-byte rows and tags; shared_operand
// narrow rows, 2..kSharedMaxAggs accumulators of the one raw operand in ONE launch; planes the same rows, one launch per
// accumulator plane; pair 20-byte rows of two operands, one launch per plane; pair_planes both.  (The 8-byte rows of PTF_ROW8 are
// the narrow FORM -- same block, same LDS, one launch -- with a row of their own: Pass2Rows::narrow8.)
enum class Pass2Form : int { refused = -1, flat_one, flat_any, stream_wide, narrow, shared_operand, planes, pair, pair_planes };
constexpr const char* kPass2FormName[] = {"flat_one", "flat_any", "stream_wide", "narrow", "shared_operand", "planes", "pair", "pair_planes"};

// The eight, twelve or sixteen bytes of a routed row that a lane of k_partition_agg_lean loads (the Rows* policies of dfx_k_pass2.hip):
// wide {key, operand}, the block holds keys; narrow {image, operand}, the block holds 32-bit tags; pair0 {operand lo, operand hi,
// image}: operand 0 of a 20-byte pair row; *_xf: the operand is raw, the launch applies its plane's transform; narrow8 {image,
// Float32 bits}: the decode widens the bits (shadow_widen), everything behind it is narrow's.
// narrow8_pred: narrow8's rows read from a window of a table's routed shadow (dfx_routed_shadow.hpp), EVERY row of the window -- the
// launch evaluates the query's predicate on the widened operand and stages the passing rows in LDS; choose_pass2_scan below.
enum class Pass2Rows : int { wide, narrow, pair0, narrow_xf, pair0_xf, narrow8, narrow8_pred };

constexpr int kP2Waves = 16;          // waves of a pass-2 workgroup (kABlock / 64)
constexpr int kP2RetryRows = 128;     // per-wave queue of rows that missed their home group (narrow rows: 12 bytes each)
constexpr int kP2RetryRowsWide = 96;  // ... 16-byte rows: 128 KB of block + 16 x 96 x 16 B = 152 KB of LDS
constexpr int kSharedMaxAggs = 3;     // PTF_SHARED: 4096 slots x (4-byte tag + 3 accumulators) = 112 KB of LDS
constexpr size_t kP2LdsLimit = 160 * 1024 - 256;
constexpr int kP2StageRows = 192;     // narrow8_pred: per-wave ring of passing rows (8 bytes each): 127 left over + the 64 of one trip
constexpr uint32_t kP2MaxProducers = 1024;  // (k_partition_agg scans the producer counts one per thread)

struct Pass2Launch {
  Pass2Rows rows = Pass2Rows::wide;
  uint32_t operand = 0;       // pair forms: DevPartition::pair_operand
  uint32_t plane_spills = 0;  // one launch per plane: DevPartition::plane_spills
  bool keeps_snap = true;     // false: snap_host = nullptr (only a window's last launch publishes the control block)
};
struct Pass2Choice {
  Pass2Form form = Pass2Form::refused;
  size_t lds_bytes = 0;
  int n_launches = 0;  // one, or one per accumulator plane: launch a aggregates plane a
  Pass2Launch launch[kMaxAggs];
};

constexpr bool pass2_is_pair(Pass2Form f) { return f == Pass2Form::pair || f == Pass2Form::pair_planes; }
constexpr bool pass2_per_plane(Pass2Form f) { return f == Pass2Form::planes || pass2_is_pair(f); }

// Dynamic LDS of a launch.  flat_*: the block's key and accumulator planes, the prefix of the producer counts.  The others: the
// block -- keys or 4-byte tags, and the accumulator planes of ONE launch -- and sixteen per-wave queues of parked rows (narrow8 rows:
// a parked row is widened first and stays twelve bytes, so its bytes are narrow's).
constexpr size_t pass2_lds_bytes(Pass2Form f, uint32_t slots, int na, uint32_t n_producers) {
  if (f == Pass2Form::flat_one || f == Pass2Form::flat_any) return (size_t)slots * (size_t)(1 + na) * 8 + (size_t)(n_producers + 1) * 4 + 16;
  if (f == Pass2Form::stream_wide) return (size_t)slots * 16 + (size_t)kP2Waves * kP2RetryRowsWide * 16;
  return (size_t)slots * (size_t)(4 + 8 * (f == Pass2Form::shared_operand ? na : 1)) + (size_t)kP2Waves * kP2RetryRows * 12;
}

// flags: PT.flags; na, kw: T's; slots: of a table block (T.block_mask + 1); narrow_line: kNarrowLine.
inline Pass2Choice choose_pass2(uint32_t flags, int na, int kw, uint32_t n_words, uint32_t slots, uint32_t n_producers, uint32_t pair_ops,
                                bool narrow_line) {
  const Pass2Choice refused;
  Pass2Choice c;
  const auto take = [&](Pass2Form f, int n_launches) {
    c.form = f;
    c.lds_bytes = pass2_lds_bytes(f, slots, na, n_producers);
    c.n_launches = n_launches;
  };
  // An oddity, kept: the FLAT forms' bytes are checked whatever form follows, except under PTF_PAIR / PTF_PLANES (one-plane blocks
  // fit where na planes would not) -- and a launch with one of those two flags then has no check of its own form's bytes at all.
  if ((pass2_lds_bytes(Pass2Form::flat_any, slots, na, n_producers) > kP2LdsLimit && !(flags & (PTF_PAIR | PTF_PLANES))) || n_producers > kP2MaxProducers)
    return refused;
  if (!(flags & PTF_NARROW)) {
    take(na != 1 ? Pass2Form::flat_any : ((flags & PTF_STREAM_PASS2) && n_words == 2) ? Pass2Form::stream_wide : Pass2Form::flat_one, 1);
  } else if ((flags & PTF_SHARED) && !(flags & PTF_PLANES)) {
    take(Pass2Form::shared_operand, 1);
    if (na < 2 || na > kSharedMaxAggs || kw != 1 || c.lds_bytes > kP2LdsLimit) return refused;
    c.launch[0].rows = Pass2Rows::narrow;
  } else if (flags & PTF_SHARED) {
    // aggregates of one operand, one launch of the one-value kernel per accumulator plane (the plane's own transform and atomic)
    if (na < 2 || na > kMaxAggs || kw != 1) return refused;
    take(Pass2Form::planes, na);
    for (int a = 0; a < na; ++a) c.launch[a] = {Pass2Rows::narrow_xf, 0u, a + 1 == na ? 1u : 0u, a + 1 == na};
  } else if (flags & PTF_PAIR) {
    // launches of the one-value kernel over the same regions, one per accumulator plane, each on its operand; the first claims
    // the window's new keys, the others find them, the last resets CTRL_MAX_FILL and publishes the control block
    if (na < 2 || na > kMaxAggs || kw != 1 || !narrow_line) return refused;
    const bool raw_ops = (flags & PTF_PLANES) != 0;  // (three and more aggregates: the launch applies the accumulator's transform)
    take(raw_ops ? Pass2Form::pair_planes : Pass2Form::pair, na);
    for (int a = 0; a < na; ++a) {
      Pass2Launch& l = c.launch[a];
      l.operand = (pair_ops >> a) & 1u;
      l.rows = l.operand == 0u ? (raw_ops ? Pass2Rows::pair0_xf : Pass2Rows::pair0) : (raw_ops ? Pass2Rows::narrow_xf : Pass2Rows::narrow);
      l.plane_spills = 1u;  // the last accumulator of this operand?
      for (int b = a + 1; b < na; ++b)
        if (((pair_ops >> b) & 1u) == l.operand) l.plane_spills = 0u;
      l.keeps_snap = a + 1 == na;
    }
  } else if (flags & PTF_ROW8) {
    if (na != 1 || kw != 1 || !narrow_line || !(flags & PTF_CHUNK16)) return refused;
    take(Pass2Form::narrow, 1);
    c.launch[0].rows = Pass2Rows::narrow8;
  } else {
    if (na != 1 || kw != 1) return refused;
    take(Pass2Form::narrow, 1);
    c.launch[0].rows = Pass2Rows::narrow;
  }
  return c;
}

// ---- the scan over a routed shadow (Pass2Rows::narrow8_pred) ---------------------------------------------------------------------
// The comparison form of a launch, k_partition_agg_lean's SCAN: none (every other row form), the run-time form, no predicate, or the
// two terms' three-way masks m0 | m1 << 3 for the four range forms pass 1 instantiates too (launch_partition_ws).
constexpr int kP2ScanNone = -1, kP2ScanRuntime = 0, kP2ScanAll = 1;
constexpr int pass2_scan_form(uint32_t np, uint32_t m0, uint32_t inv0, uint32_t m1, uint32_t inv1) {
  if (np == 0) return kP2ScanAll;
  if (np != 2 || inv0 || inv1) return kP2ScanRuntime;
  if ((m0 == 4 || m0 == 6) && (m1 == 1 || m1 == 3)) return (int)(m0 | (m1 << 3));
  return kP2ScanRuntime;
}
// LDS: narrow's block and parked-row queues, and sixteen stages
constexpr size_t pass2_scan_lds_bytes(uint32_t slots) { return pass2_lds_bytes(Pass2Form::narrow, slots, 1, 0) + (size_t)kP2Waves * kP2StageRows * 8; }

struct Pass2ScanChoice {
  Pass2Rows rows = Pass2Rows::wide;  // narrow8_pred, or (refused) anything else
  int scan = kP2ScanNone;
  size_t lds_bytes = 0;
};
// flags: the window's layout flags; na, kw: T's; sum_f64: the one accumulator adds Float64; np ... inv1: the predicate's terms.
// Refused: anything but one SUM over 8-byte rows in whole-line chunks, a predicate of one or three and more terms, a block that
// does not fit.
inline Pass2ScanChoice choose_pass2_scan(uint32_t flags, int na, int kw, bool sum_f64, uint32_t slots, uint32_t n_producers, bool narrow_line, uint32_t np,
                                         uint32_t m0, uint32_t inv0, uint32_t m1, uint32_t inv1) {
  Pass2ScanChoice c;
  const uint32_t need = PTF_NARROW | PTF_CHUNK16 | PTF_ROW8;
  if ((flags & need) != need || (flags & (PTF_SHARED | PTF_PAIR | PTF_PLANES | PTF_HOT)) || !narrow_line) return c;
  if (na != 1 || kw != 1 || !sum_f64 || (np != 0 && np != 2) || n_producers == 0 || n_producers > kP2MaxProducers) return c;
  if (slots < 64 || (slots & (slots - 1)) || pass2_scan_lds_bytes(slots) > kP2LdsLimit) return c;
  c.rows = Pass2Rows::narrow8_pred;
  c.scan = pass2_scan_form(np, m0, inv0, m1, inv1);
  c.lds_bytes = pass2_scan_lds_bytes(slots);
  return c;
}

}  // namespace dfx
