// What the host and gemm_fp8_kernel (native/hip/probe_gemm_fp8.inc) share: the tile sizes, the shapes the kernel
// takes, and every index the kernel forms, into A, B and C and into LDS. C[M][N] (fp32) = A[M][K] . B^T with A
// e4m3 [M][K] and B e4m3 [N][K], both K-contiguous, so one set of functions serves both operands. The
// workgroup-to-tile map is the bf16 tenant's (nanogpu/gemm_host.h). The kernel has no tail code, so that each index
// lies inside its array is a property of these functions alone: native/tests/gemm_fp8_host_main.cpp asserts it on
// the CPU, and replays a small product through them.
#pragma once

#include <cstddef>
#include <cstdint>

#include "nanogpu/gemm_host.h"

namespace nanogpu {
namespace gemm_fp8 {

// One workgroup of 4 waves owns a 128 x 128 tile of C, wave w the 64 x 64 quadrant (w >> 1, w & 1) as 2 x 2 MFMA
// tiles of 32 x 32; K goes through LDS in tiles of 128, two k-steps of 64 (one v_mfma_scale_f32_32x32x64_f8f6f4).
constexpr int kBM = gemm::kBM, kBN = gemm::kBN, kBK = 128;
constexpr int kThreads = gemm::kThreads;
constexpr int kStages = 2;
constexpr int kKSteps = kBK / 64;
constexpr int kChunk = 16;   // e4m3 elements of a 16-byte access
constexpr int kOperands = 2;   // 0: A, 1: B
static_assert(kBM == 128 && kBN == kBM && kThreads == 256, "one row map serves A's rows and B's columns");

// LDS, in bytes. A stage of an operand is 128 rows (of A) or columns (of B) of 128 k, 128 bytes each, unpadded:
// exactly the bf16 kernel's A stage, so the 16-byte chunk c of row r lies at chunk c ^ ((r >> 1) & 7). The lanes
// that read one chunk index of 16 consecutive rows then touch 16 different chunks of a 256-byte line pair, and so
// do the sixteen lanes that write two whole rows. Both stages of A come first, then both of B.
constexpr int kStageBytes = kBM * kBK;
constexpr int kLdsBytes = kOperands * kStages * kStageBytes;
static_assert(kLdsBytes == 65536 && 2 * kLdsBytes <= 160 * 1024, "two workgroups share a CU's 160 KiB");

// M and N are multiples of the tile, K of the K tile, and the launch stays below HIP's 2^32 work-items.
NANOGPU_HD inline bool shape_ok(int64_t m, int64_t n, int64_t k) {
  return k > 0 && k % kBK == 0 && gemm::shape_ok(m, n, k);
}

// ---- global to LDS: pass i = 0..3 of thread t moves 16 bytes of A and 16 bytes of B --------------------------
// `tile` is the row tile of A or the column tile of B, `ld` the operand's row length, K.
constexpr int kLoadPasses = 4;
NANOGPU_HD inline int load_row(int t, int i) { return (t >> 3) + 32 * i; }
NANOGPU_HD inline int load_chunk(int t) { return t & 7; }
NANOGPU_HD inline size_t global_index(int tile, int kt, int ld, int t, int i) {
  return static_cast<size_t>(tile * kBM + load_row(t, i)) * static_cast<size_t>(ld) + static_cast<size_t>(kt) * kBK +
         static_cast<size_t>(kChunk * load_chunk(t));
}
NANOGPU_HD inline int lds_index(int operand, int stage, int row, int chunk) {
  return (operand * kStages + stage) * kStageBytes + row * kBK + kChunk * (chunk ^ ((row >> 1) & 7));
}

// ---- LDS to operands, k-step s = 0..1 -----------------------------------------------------------------------
// v_mfma_scale_f32_32x32x64_f8f6f4 with e4m3 operands (cbsz = blgp = 0), as measured (profiles/gpu_calibration.md):
// lane l holds row / column l & 31; byte b of its 32 operand bytes is k = mfma_k(l, b): dwords 0..3 are
// k = 16 (l >> 5) + j and dwords 4..7 are k = 32 + 16 (l >> 5) + j, j = 0..15. The kernel does not follow that map.
// It gives lane l the 32 consecutive bytes k = 64 s + 32 (l >> 5) .. + 31 of its row, two 16-byte reads (half h =
// 0..1), for A and for B alike. Both operands then put the same k into the same slot of the instruction, and a dot
// product does not care in which order k is summed. That holds only because every scale is one: the instruction's
// scale blocks are 32 consecutive k of the measured map, of which a lane's bytes here are not one. Per-block
// scales cannot be added on top of this read; they need the measured map.
NANOGPU_HD inline int mfma_k(int lane, int byte) { return 32 * (byte >> 4) + 16 * (lane >> 5) + (byte & 15); }
// `row_base` is the first row of the MFMA tile in the stage: (w >> 1) * 64 + 32 i for A, (w & 1) * 64 + 32 j for B.
NANOGPU_HD inline int tile_row_base(int operand, int wave, int ij) { return (operand == 0 ? wave >> 1 : wave & 1) * 64 + 32 * ij; }
NANOGPU_HD inline int read_index(int operand, int stage, int wave, int lane, int s, int ij, int h) {
  return lds_index(operand, stage, tile_row_base(operand, wave, ij) + (lane & 31), 4 * s + 2 * (lane >> 5) + h);
}
// The k inside the K tile of byte `byte` = 0..31 of what read_index's two reads give a lane.
NANOGPU_HD inline int read_k(int lane, int s, int byte) { return 64 * s + 32 * (lane >> 5) + byte; }

// ---- accumulators to C: the bf16 instruction's map and the bf16 kernel's quadrants ---------------------------
NANOGPU_HD inline size_t c_index(int tm, int tn, int n, int wave, int lane, int i, int j, int reg) {
  return gemm::c_index(tm, tn, n, wave, lane, i, j, reg);
}

// What a launch must move at the least: A and B read once, a byte an element, C written once.
NANOGPU_HD inline double compulsory_bytes(double m, double n, double k) { return k * (m + n) + 4.0 * m * n; }

}  // namespace gemm_fp8
}  // namespace nanogpu
