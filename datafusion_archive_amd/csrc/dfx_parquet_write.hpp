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

#include "dfx_parquet_dict_enc.hpp"
#include "dfx_parquet_lz4_enc.hpp"

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

hipError_t launch_pqw_bases(pqw::PqwPage* pages, int64_t n, hipStream_t s);  // the bases kernel alone (pages: n + 1)

// ---- the "dictionary" option (dfx_k_parquet_write_dict.hip; the format and the decision: dfx_parquet_dict_enc.hpp) -------------------
// One launch chain over the columns of a launch whose chunks are in dictionary mode:
//   insert (a lane per valid row: the row's slot in its chunk's table) -> mark (a wave per tile: the rows that introduce an entry, the
//   Utf8 compare against the slot's representative) -> decide (a workgroup per column: the launch's new entries and body bytes, the
//   rule, the chunk's state) -> scan (a wave per page: the run kind and sizes into the PqwPage table) -> bases -> [host reads the page
//   table and the states back, sizes the output buffer and the dictionary bodies] -> commit (a wave per tile: ids, the entries appended
//   to the body) -> encode (a wave per tile: levels, width byte, run header, indices).
// No lane waits for another lane's store inside a launch: what one kernel leaves for another is read by a later launch on the same
// stream; inside a launch lanes meet only through agent-scope atomics (CAS on a key word, min on first_row, or on a flag or an output
// word) whose returned value is all they use.
constexpr uint64_t kPqwdEmpty = ~0ull;        // a key word no row has claimed; a row whose key IS this value uses the slot after the table
constexpr uint32_t kPqwdNone = 0xFFFFFFFFu;   // id: unassigned; first_row: none yet; slot_of_row: null row, or no slot found
constexpr uint32_t kPqwdMaxProbe = 1024;      // slots a row looks at before it gives up (the launch then falls back)
struct PqwdSlot {      // 16 bytes; a chunk's table is memset to 0xFF when its row group opens: {empty, none, unassigned}
  uint64_t key;        // fixed width: the stored bits; Utf8: the masked 64-bit hash of the bytes
  uint32_t first_row;  // the launch-local row that introduces the entry: the least row of the launch that reached the slot
  uint32_t id;         // assigned by the commit of the launch that introduced the entry
};
enum : uint32_t { PQWD_MODE_DICT = 0, PQWD_MODE_PLAIN = 1 };
enum : uint32_t { PQWD_OVERFLOW = 1u, PQWD_COLLISION = 2u };  // a probe ran out or the claims exceed N - E; two Utf8 values share a hash
struct PqwdState {     // per chunk, zeroed when the row group opens; written by decide, read back with the page table
  uint64_t entries, body_bytes;  // E and B after the last launch held in dictionary mode
  uint64_t entries_before, body_before;  // ... and before it: where commit appends
  uint32_t mode;       // PQWD_MODE_*
  uint32_t flags;      // PQWD_OVERFLOW / PQWD_COLLISION, raised by insert / mark of the launch that then fell back
  uint32_t width;      // index width of the last launch held
  uint32_t claimed;    // insert: key words claimed in the running launch; decide zeroes it
};
struct PqwdTile {      // per column and tile of a launch
  uint32_t non_null, rank_base;    // mark / scan, as PqwTile
  uint32_t entries, entry_base;    // mark: rows of the tile that introduce an entry; decide: ... of the launch's tiles before it
  uint32_t min_slot, max_slot;     // mark: over the tile's valid rows (kPqwdNone / 0 without one)
  uint64_t bytes, byte_base;       // mark / decide: dictionary body bytes of the introduced entries
};
// the index run's kind (pqw::DICT_RUN_*) rides in PqwPage::kind above the level kind
constexpr uint32_t kPqwdRunShift = 8;
struct DevPqwdCol {
  PqwdSlot* slots;     // mask + 2 slots: the table, then the slot of the key that equals kPqwdEmpty
  PqwdState* state;
  uint8_t* body;       // the dictionary page's body: [0, body_cap)
  uint32_t* entry_off; // Utf8: byte of every entry's length prefix in body, by id
  uint64_t body_cap;
  uint32_t mask;       // table slots - 1
  uint32_t limit;      // N
};
struct DevPqwdPlan {
  DevPqwPlan base;
  DevPqwdCol dict[kPqwMaxCols];
  uint64_t hash_mask;  // Utf8 hashes are cut to "dictionary_hash_bits" bits
};
static_assert(sizeof(DevPqwdPlan) <= 4096, "the plan is a kernel argument");

// slot_of_row: n_cols * rows words; tiles: n_cols * n_tiles; pages: n_cols * n_pages + 1; ctrl as above
hipError_t launch_pqwd_measure(const DevPqwdPlan& plan, uint32_t* slot_of_row, PqwdTile* tiles, pqw::PqwPage* pages, hipStream_t s);
hipError_t launch_pqwd_encode(const DevPqwdPlan& plan, const uint32_t* slot_of_row, const PqwdTile* tiles, const pqw::PqwPage* pages, uint8_t* out,
                              uint64_t out_bytes, uint64_t* ctrl, hipStream_t s);

// ---- the "compression" option (dfx_k_parquet_write_lz4.hip; the block rule: dfx_parquet_lz4_enc.hpp) ---------------------------------
// After a chain's encode kernel the host, which has read the chain's page table back, names every body of the launch to k_pqw_lz4 (a
// wave per page: the body as one raw LZ4 block in a slot of its own) -> k_pqw_lz4_bases (the sizes into 8-byte-aligned bases) ->
// [host reads the sizes and bases back, sizes the packed buffer] -> k_pqw_lz4_compact (every block to its base).
struct PqwLz4In {      // per page, built by the host
  const uint8_t* src;  // the body on the device
  uint64_t slot_off;   // of its slot of lz4_bound(len) bytes in the slot buffer, 8-byte aligned
  uint32_t len;        // bytes of the body
  uint32_t pad;
};
struct PqwLz4Out {     // per page, read back; entry [pages] holds the packed buffer's length in `base`
  uint64_t base;       // of the block in the packed buffer, 8-byte aligned (k_pqw_lz4_bases)
  uint32_t bytes;      // of the block
  uint32_t sequences;
};
// ctrl: bit 1 set when a sequence would leave its slot, or a slot or a base lies outside its buffer (that wave stores nothing more)
hipError_t launch_pqw_lz4(const PqwLz4In* in, int64_t n_pages, uint8_t* slots, uint64_t slots_bytes, PqwLz4Out* out, uint64_t* ctrl, hipStream_t s);  // out: n_pages + 1
hipError_t launch_pqw_lz4_compact(const PqwLz4In* in, const PqwLz4Out* out, int64_t n_pages, const uint8_t* slots, uint64_t slots_bytes, uint8_t* packed,
                                  uint64_t packed_bytes, uint64_t* ctrl, hipStream_t s);

}  // namespace dfx
