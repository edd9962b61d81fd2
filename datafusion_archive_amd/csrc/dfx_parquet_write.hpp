// dfx_parquet_write.hpp -- what the Parquet writer's host code (dfx_parquet_write.cpp) and its kernels (dfx_k_parquet_write.hip)
// share beyond the HIP-free rules of dfx_parquet_enc.hpp: the launch plan and the launchers.
//
// One launch chain encodes the rows of one piece (at most pqw::launch_rows(page_rows) of them, a whole number of pages) of up to
// kPqwMaxCols columns: measure (a wave per tile) -> scan (a wave per page) -> bases (one workgroup) -> [host reads the page table back,
// sizes the output buffer] -> encode (a wave per tile).  The output buffer holds the page bodies column by column, page by page, each
// 8-byte aligned.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "dfx_parquet_enc.hpp"

namespace dfx {

constexpr int kPqwMaxCols = 32;  // columns of one launch chain: a wider schema takes several

struct DevPqwCol {
  const void* values;       // fixed width: row 0 of the launch; Boolean: bitmap base (bit_offset)
  const uint8_t* validity;  // null: no nulls
  const int32_t* offsets;   // Utf8: row 0 of the launch (rows + 1 entries)
  const uint8_t* data;      // Utf8: indexed by the raw offsets
  int64_t bit_offset;       // of row 0 in validity / Boolean values
  uint8_t dtype;            // DevType
  uint8_t optional;
};
struct DevPqwPlan {
  int32_t n_cols;
  int64_t rows, page_rows;
  int64_t n_tiles, n_pages;  // per column
  DevPqwCol col[kPqwMaxCols];
};

// ctrl: one zeroed word -- bit 0 set when a tile's recount disagrees with the scan or its span would leave its page or the buffer
// (that tile stores nothing)
hipError_t launch_pqw_measure(const DevPqwPlan& plan, pqw::PqwTile* tiles, hipStream_t s);
hipError_t launch_pqw_scan(const DevPqwPlan& plan, pqw::PqwTile* tiles, pqw::PqwPage* pages, hipStream_t s);  // pages: n_cols * n_pages + 1
hipError_t launch_pqw_encode(const DevPqwPlan& plan, const pqw::PqwTile* tiles, const pqw::PqwPage* pages, uint8_t* out, uint64_t out_bytes,
                             uint64_t* ctrl, hipStream_t s);

}  // namespace dfx
