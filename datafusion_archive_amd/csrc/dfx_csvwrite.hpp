// dfx_csvwrite.hpp -- what the CSV writer's host code (dfx_csv_write.cpp) and its kernels (dfx_k_csvwrite.hip) share.
//
// One batch of rows becomes CSV text in two kernels, a wave per tile of 64 rows in both:
//   format   every lane formats the fixed-width cells of its row ONCE (dfx_numfmt.hpp) into the row's SLOT, a fixed-stride record
//            in the wave's LDS: [cell length bytes][Utf8 descriptors][cell text at fixed offsets]; Utf8 cells are only measured
//            (quotes counted, quoting decided; a long string by the whole wave).  The tile's slots leave as one contiguous,
//            aligned span with 16-byte stores; the tile's text length goes to tile_bytes[tile].
//   (scan)   tile_bytes -> tile_base (64-bit byte offsets), tile_base[n_tiles] = the batch's text length
//   assemble the tile's slots come back into LDS with 16-byte loads, the lanes lay their rows out back to back in an LDS window
//            (cell text from the slot, Utf8 bytes from the column, quoted and doubled as the descriptor says), and the window
//            leaves for its FINAL position tile_base[tile] as one contiguous span: aligned 16-byte stores, the unaligned head and
//            tail byte-wise.  A tile whose text does not fit the window takes the general path: a lane per row straight to
//            global memory, the wave together on every Utf8 cell longer than kCwLongCell.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace dfx {

constexpr int kCwMaxCols = 32;
constexpr uint32_t kCwWindowMin = 8192, kCwWindowMax = 32768;  // bytes of a tile's text a wave lays out in LDS: 64 rows of the longest
                                                               // fixed-width cells + 2 KB for Utf8, within these (DevCwPlan::window)
constexpr uint32_t kCwLongCell = 256;  // a Utf8 cell longer than this is measured / copied by the whole wave
constexpr int64_t kCwBatchRows = 1 << 20;  // rows formatted per launch: larger input batches are split

struct DevCwCol {
  const void* values;       // fixed width: row 0 of the launch; Boolean: bitmap base (bit_offset)
  const uint8_t* validity;  // null: no nulls
  const int32_t* offsets;   // Utf8: row 0 of the launch (rows + 1 entries)
  const uint8_t* data;      // Utf8: indexed by the raw offsets
  int64_t bit_offset;       // of row 0 in validity / Boolean values
  uint32_t slot;            // where the column's text (fixed width) / descriptor (Utf8) lies in a row's slot
  uint8_t dtype;            // DevType
};
struct DevCwPlan {
  int32_t n_cols;
  uint32_t stride;  // bytes of a row's slot, a multiple of 16
  uint32_t window;  // bytes of the LDS window of the assemble kernel, a multiple of 16
  DevCwCol col[kCwMaxCols];
};
// slot layout for a schema: fills slot of every column and the window, returns the stride
uint32_t csvw_layout(DevCwPlan* plan);
// LDS a wave needs in the assemble kernel (the format kernel needs the slots only); a workgroup has csvw_waves() waves
size_t csvw_wave_lds(const DevCwPlan& plan);

// ctrl: two zeroed words -- [0] set when the two kernels disagree about a length or a tile would leave the buffer (nothing is
// written then), [1] tiles that took the general path
hipError_t launch_csvw_format(const DevCwPlan& plan, int64_t n, uint8_t* slots, uint64_t* tile_bytes, hipStream_t s);
hipError_t launch_csvw_scan(const uint64_t* tile_bytes, int64_t n_tiles, uint64_t* tile_base, hipStream_t s);
hipError_t launch_csvw_assemble(const DevCwPlan& plan, int64_t n, const uint8_t* slots, const uint64_t* tile_base, uint8_t* out,
                                uint64_t out_bytes, uint64_t* ctrl, double algo_bytes, hipStream_t s);

}  // namespace dfx
