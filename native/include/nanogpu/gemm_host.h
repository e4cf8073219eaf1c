// What the host and gemm_bf16_kernel (native/hip/probe_gemm.inc) share: the tile sizes, the shapes the kernel
// takes, the workgroup-to-tile map, and every index the kernel forms, into A, B and C and into LDS. The kernel has
// no tail code, so that each of these indices lies inside its array is a property of these functions alone:
// native/tests/gemm_host_main.cpp asserts it on the CPU, and replays a small product through them.
#pragma once

#include <cstddef>
#include <cstdint>

#if !defined(NANOGPU_HD)
#if defined(__HIPCC__)
#define NANOGPU_HD __host__ __device__
#else
#define NANOGPU_HD
#endif
#endif

namespace nanogpu {
namespace gemm {

// One workgroup of 4 waves owns a 128 x 128 tile of C, wave w the 64 x 64 quadrant (w >> 1, w & 1) as 2 x 2 MFMA
// tiles of 32 x 32; K goes through LDS in tiles of 64, four k-steps of 16.
constexpr int kBM = 128, kBN = 128, kBK = 64;
constexpr int kThreads = 256;
constexpr int kStages = 2;
constexpr int kXcds = 8;
constexpr int kChunk = 8;   // bf16 elements of a 16-byte access
constexpr uint64_t kWorkItemLimit = uint64_t(1) << 32;

// LDS, in 16-bit elements. A stage of A is 128 rows of 64 k (128 bytes), unpadded: the 16-byte chunk c of row r
// lies at chunk c ^ ((r >> 1) & 7). Sixteen lanes that read one chunk index of 16 consecutive rows (the operand
// read) then touch 16 different chunks of a 256-byte line pair, and the sixteen lanes that write two whole rows do
// too. A stage of B is 64 k-rows of 128 columns, row-major as in memory, each row padded by 64 bytes to 320: the
// transposed read addresses 4 rows x 32 bytes per 16 lanes, and 80 dwords a row put the 4 rows of two neighbouring
// groups onto 64 different banks.
constexpr int kAStageElems = kBM * kBK;
constexpr int kBRowElems = kBN + 32;
constexpr int kBStageElems = kBK * kBRowElems;
constexpr int kBAt = kStages * kAStageElems;
constexpr int kLdsElems = kBAt + kStages * kBStageElems;
constexpr int kLdsBytes = 2 * kLdsElems;
static_assert(kLdsBytes == 73728 && 2 * kLdsBytes <= 160 * 1024, "two workgroups share a CU's 160 KiB");

// M and N are multiples of the tile, K of the K tile, and the launch stays below HIP's 2^32 work-items.
NANOGPU_HD inline uint64_t tiles(int64_t m, int64_t n) { return static_cast<uint64_t>(m / kBM) * static_cast<uint64_t>(n / kBN); }
NANOGPU_HD inline bool shape_ok(int64_t m, int64_t n, int64_t k) {
  if (m <= 0 || n <= 0 || k <= 0 || m % kBM || n % kBN || k % kBK) return false;
  if (m > (int64_t(1) << 30) || n > (int64_t(1) << 30) || k > (int64_t(1) << 30)) return false;
  return tiles(m, n) * kThreads < kWorkItemLimit;
}

// A dispatch deals its workgroups to the XCDs in turn, and each XCD has an L2 of its own. Block b of G becomes
// tile (b % 8) * (G / 8) + min(b % 8, G % 8) + b / 8: XCD x works through one contiguous run of tiles, G / 8 long
// and one longer on the first G % 8 XCDs. A bijection of 0..G-1 for every G.
NANOGPU_HD inline uint32_t tile_of_block(uint32_t b, uint32_t g) {
  const uint32_t x = b % kXcds, rem = g % kXcds;
  return x * (g / kXcds) + (x < rem ? x : rem) + b / kXcds;
}
// Tiles are walked in bands of kBandRows row panels of A: down the band's rows first, then along N. The 64
// workgroups an XCD of 32 CUs holds at once then form an 8 x 8 square of tiles, which shares 8 panels of A and 8
// of B in that XCD's L2, where a walk along N alone shares 1 of A and needs 64 of B (measured: see
// profiles/gpu_calibration.md). The last band has the rows that are left.
constexpr int kBandRows = 8;
struct TileAt {
  int m, n;
};
NANOGPU_HD inline TileAt tile_at(uint32_t tile, int m, int n) {
  const uint32_t tiles_m = static_cast<uint32_t>(m / kBM), band_tiles = kBandRows * static_cast<uint32_t>(n / kBN);
  const uint32_t first = tile / band_tiles * kBandRows, in_band = tile % band_tiles;
  const uint32_t rows = tiles_m - first < kBandRows ? tiles_m - first : kBandRows;
  return TileAt{static_cast<int>(first + in_band % rows), static_cast<int>(in_band / rows)};
}

// ---- global to LDS: pass i = 0..3 of thread t moves 16 bytes of A and 16 bytes of B -------------------------
constexpr int kLoadPasses = 4;
NANOGPU_HD inline int a_load_row(int t, int i) { return (t >> 3) + 32 * i; }
NANOGPU_HD inline int a_load_chunk(int t) { return t & 7; }
NANOGPU_HD inline int b_load_row(int t, int i) { return (t >> 4) + 16 * i; }
NANOGPU_HD inline int b_load_chunk(int t) { return t & 15; }
NANOGPU_HD inline size_t a_global_index(int tm, int kt, int k, int t, int i) {
  return static_cast<size_t>(tm * kBM + a_load_row(t, i)) * static_cast<size_t>(k) + static_cast<size_t>(kt) * kBK +
         static_cast<size_t>(kChunk * a_load_chunk(t));
}
NANOGPU_HD inline size_t b_global_index(int tn, int kt, int n, int t, int i) {
  return (static_cast<size_t>(kt) * kBK + static_cast<size_t>(b_load_row(t, i))) * static_cast<size_t>(n) +
         static_cast<size_t>(tn * kBN + kChunk * b_load_chunk(t));
}
NANOGPU_HD inline int a_lds_index(int stage, int row, int chunk) {
  return stage * kAStageElems + row * kBK + kChunk * (chunk ^ ((row >> 1) & 7));
}
NANOGPU_HD inline int b_lds_index(int stage, int krow, int col) { return kBAt + stage * kBStageElems + krow * kBRowElems + col; }

// ---- LDS to operands, k-step s = 0..3 ----------------------------------------------------------------------
// mfma_f32_32x32x16_bf16: lane l holds A[l & 31][8 (l >> 5) + j] and B[8 (l >> 5) + j][l & 31], j = 0..7.
// A, M tile i = 0..1 of the wave: one 16-byte read.
NANOGPU_HD inline int a_read_index(int stage, int wave, int lane, int s, int i) {
  return a_lds_index(stage, (wave >> 1) * 64 + 32 * i + (lane & 31), 2 * s + (lane >> 5));
}
// B, N tile j = 0..1 of the wave, half h = 0..1 of the eight k: one ds_read_b64_tr_b16. Lane 4q + p of a 16-lane
// group addresses k-row q of four and columns 4p .. 4p + 3; lane c of the group receives column c of the four rows.
NANOGPU_HD inline int b_read_index(int stage, int wave, int lane, int s, int j, int h) {
  const int group = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  return b_lds_index(stage, 16 * s + 8 * (group >> 1) + 4 * h + q, (wave & 1) * 64 + 32 * j + 16 * (group & 1) + 4 * p);
}
// The lane of the same group whose address supplies element e of `lane`'s result, and the element of its four.
NANOGPU_HD inline int tr_source_lane(int lane, int e) { return (lane & ~15) + 4 * e + ((lane & 15) >> 2); }
NANOGPU_HD inline int tr_source_elem(int lane) { return lane & 3; }

// ---- accumulators to C: register reg = 0..15 of tile (i, j) is row (reg & 3) + 8 (reg >> 2) + 4 (l >> 5) ---
NANOGPU_HD inline size_t c_index(int tm, int tn, int n, int wave, int lane, int i, int j, int reg) {
  const int row = tm * kBM + (wave >> 1) * 64 + 32 * i + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
  return static_cast<size_t>(row) * static_cast<size_t>(n) + static_cast<size_t>(tn * kBN + (wave & 1) * 64 + 32 * j + (lane & 31));
}

// What a launch must move at the least: A and B read once, C written once. A lower bound on HBM traffic.
NANOGPU_HD inline double compulsory_bytes(double m, double n, double k) { return 2.0 * k * (m + n) + 4.0 * m * n; }

}  // namespace gemm
}  // namespace nanogpu
