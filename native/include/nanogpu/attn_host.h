// What the host and attn_bf16_kernel (native/hip/probe_attn.inc) share: the tile sizes of its two instantiations,
// the shapes the kernel takes, the workgroup-to-(head, query tile) map, and every index the kernel forms, into Q, K,
// V and O and into LDS. The kernel has no tail code, so that each of these indices lies inside its array is a
// property of these functions alone: native/tests/attn_host_main.cpp asserts it on the CPU, and replays a small
// attention through them, the permutation of the kv index between P's registers and V's transposed read included.
#pragma once

#include <cstddef>
#include <cstdint>

#include "nanogpu/gemm_host.h"   // tile_of_block, tr_source_lane, kWorkItemLimit

namespace nanogpu {
namespace attn {

// O[b] = softmax(Q[b] K[b]^T / sqrt(128)) V[b], head dimension 128, computed transposed: S^T = K_blk . Q^T puts one
// query in one lane column, so the softmax state of a query is per-lane. A block is 32 kv rows, one MFMA tile.
//   wide  (sq a multiple of 128): a workgroup owns 128 queries, wave w queries 32w .. 32w+31; all four waves share
//         K/V tiles of 64 rows (two blocks), in two LDS stages.
//   split (sq a multiple of 32 below 128): a workgroup owns 32 queries; its waves split K/V tiles of 128 rows, wave
//         w block w, each with a softmax state of its own, merged through LDS at the end. One LDS stage: the form is
//         memory-bound, and one stage of 72 KiB lets two workgroups a CU keep twice the loads in flight.
constexpr int kD = 128;
constexpr int kThreads = 256;
constexpr int kChunk = 8;        // bf16 elements of a 16-byte access
constexpr int kRowChunks = kD / kChunk;
constexpr int kBlockRows = 32;
constexpr int kWideQ = 128;      // the smallest sq of the wide kernel
NANOGPU_HD constexpr bool is_split(int64_t sq) { return sq < kWideQ; }
NANOGPU_HD constexpr int q_tile(bool split) { return split ? 32 : 128; }
NANOGPU_HD constexpr int kv_tile(bool split) { return split ? 128 : 64; }
NANOGPU_HD constexpr int stages(bool split) { return split ? 1 : 2; }
NANOGPU_HD constexpr int blocks_per_wave(bool split) { return split ? 1 : 2; }
NANOGPU_HD constexpr int load_passes(bool split) { return kv_tile(split) * kRowChunks / kThreads; }

// LDS, in 16-bit elements. A stage of K is kv_tile rows of 128 d (256 bytes, all 64 banks), unpadded: the 16-byte
// chunk c of row r lies at chunk c ^ (r & 15), so the sixteen lanes that read one chunk index of 16 consecutive rows
// touch 16 different chunks, and the sixteen that write one whole row do too. A stage of V is kv_tile rows of 128 d,
// row-major as in memory, each padded by 64 bytes to 320 as the GEMM pads B: the transposed read addresses 4 rows x
// 32 bytes per 16 lanes.
constexpr int kVRowElems = kD + 32;
NANOGPU_HD constexpr int k_stage_elems(bool split) { return kv_tile(split) * kD; }
NANOGPU_HD constexpr int v_stage_elems(bool split) { return kv_tile(split) * kVRowElems; }
NANOGPU_HD constexpr int v_at(bool split) { return stages(split) * k_stage_elems(split); }
constexpr int kLdsElems = 36864;
constexpr int kLdsBytes = 2 * kLdsElems;
static_assert(v_at(false) + stages(false) * v_stage_elems(false) == kLdsElems &&
                  v_at(true) + stages(true) * v_stage_elems(true) == kLdsElems && 2 * kLdsBytes <= 160 * 1024,
              "both instantiations hold 72 KiB, and two workgroups share a CU's 160 KiB");

// The split kernel's merge, over the same LDS once the tiles are done, in 32-bit words: wave w's partial O as
// [query][d], rows padded to 132 words so that sixteen lanes' 16-byte stores of one d of sixteen queries fall on 64
// different banks, then each wave's running max and sum per query.
constexpr int kMergeRow = kD + 4;
constexpr int kMergeWaveWords = 32 * kMergeRow;
constexpr int kMergeMlAt = 4 * kMergeWaveWords;
constexpr int kMergeWords = kMergeMlAt + 4 * 32 * 2;
static_assert(4 * kMergeWords <= kLdsBytes, "the merge fits the tile stages");

// sq and skv are multiples of their tiles, and the launch stays below HIP's 2^32 work-items.
NANOGPU_HD inline uint64_t workgroups(int64_t heads, int64_t sq) {
  return static_cast<uint64_t>(heads) * static_cast<uint64_t>(sq / q_tile(is_split(sq)));
}
NANOGPU_HD inline bool shape_ok(int64_t heads, int64_t sq, int64_t skv) {
  if (heads <= 0 || sq <= 0 || skv <= 0) return false;
  if (heads > (int64_t(1) << 24) || sq > (int64_t(1) << 30) || skv > (int64_t(1) << 30)) return false;
  const bool split = is_split(sq);
  if (sq % q_tile(split) || skv % kv_tile(split)) return false;
  return workgroups(heads, sq) * kThreads < gemm::kWorkItemLimit;
}

// Block b of G takes pair gemm::tile_of_block(b, G), so one XCD works through a contiguous run of (head, query tile)
// pairs with the query tile fastest: the workgroups of one head meet in one L2.
struct PairAt {
  int head, qt;
};
NANOGPU_HD inline PairAt pair_at(uint32_t pair, int sq) {
  const uint32_t q_tiles = static_cast<uint32_t>(sq / q_tile(is_split(sq)));
  return PairAt{static_cast<int>(pair / q_tiles), static_cast<int>(pair % q_tiles)};
}

// The first of the 32 queries of wave `wave`, as a row of Q and of O.
NANOGPU_HD inline size_t query_row(bool split, int head, int qt, int sq, int wave) {
  return static_cast<size_t>(head) * static_cast<size_t>(sq) + static_cast<size_t>(qt * q_tile(split) + (split ? 0 : kBlockRows * wave));
}

// ---- Q: the B operand of k-step s = 0..7 of the scores, one 16-byte global load, kept in registers ----------
// mfma_f32_32x32x16_bf16: lane l holds A[l & 31][8 (l >> 5) + j] and B[8 (l >> 5) + j][l & 31], j = 0..7.
NANOGPU_HD inline size_t q_global_index(bool split, int head, int qt, int sq, int wave, int lane, int s) {
  return (query_row(split, head, qt, sq, wave) + static_cast<size_t>(lane & 31)) * kD + static_cast<size_t>(16 * s + kChunk * (lane >> 5));
}

// ---- K and V, global to LDS: pass i of thread t moves 16 bytes of each ---------------------------------------
NANOGPU_HD inline int kv_load_row(int t, int i) { return (t >> 4) + 16 * i; }
NANOGPU_HD inline int kv_load_chunk(int t) { return t & 15; }
NANOGPU_HD inline size_t kv_global_index(bool split, int head, int kt, int skv, int t, int i) {
  return (static_cast<size_t>(head) * static_cast<size_t>(skv) + static_cast<size_t>(kt) * kv_tile(split) + static_cast<size_t>(kv_load_row(t, i))) * kD +
         static_cast<size_t>(kChunk * kv_load_chunk(t));
}
NANOGPU_HD inline int k_lds_index(bool split, int stage, int row, int chunk) {
  return stage * k_stage_elems(split) + row * kD + kChunk * (chunk ^ (row & 15));
}
NANOGPU_HD inline int v_lds_index(bool split, int stage, int row, int col) {
  return v_at(split) + stage * v_stage_elems(split) + row * kVRowElems + col;
}

// ---- LDS to operands --------------------------------------------------------------------------------------
// The first row, in the tile, of block b = 0 .. blocks_per_wave - 1 of wave `wave`.
NANOGPU_HD inline int block_row(bool split, int wave, int b) { return kBlockRows * (split ? wave : b); }
// Scores, k-step s = 0..7 over d: the A operand is eight consecutive d of one K row, one 16-byte read.
NANOGPU_HD inline int k_read_index(bool split, int stage, int wave, int lane, int b, int s) {
  return k_lds_index(split, stage, block_row(split, wave, b) + (lane & 31), 2 * s + (lane >> 5));
}
// By the C map lane l holds in register reg the score of query l & 31 and this kv row of the block.
NANOGPU_HD inline int score_kv_row(int lane, int reg) { return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5); }
// Registers 8u .. 8u+7, cast to bf16, are the B operand of k-step u = 0, 1 of O^T += V^T . P^T as they stand: its
// element j stands for kv row 16u + 8 (j >> 2) + 4 (l >> 5) + (j & 3) = score_kv_row(l, p_reg(u, j)).
NANOGPU_HD inline int p_reg(int u, int j) { return 8 * u + j; }
// V^T's A operand under the same permutation, d block db = 0..3, half hp = 0..1 of the eight kv: one
// ds_read_b64_tr_b16. Lane 4q + p of a 16-lane group addresses kv row q of four and d 4p .. 4p + 3; lane c of the group
// receives d c of the four rows (gemm::tr_source_lane, tr_source_elem).
NANOGPU_HD inline int v_read_index(bool split, int stage, int wave, int lane, int b, int u, int db, int hp) {
  const int group = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  return v_lds_index(split, stage, block_row(split, wave, b) + 16 * u + 8 * hp + 4 * (lane >> 5) + q, 32 * db + 16 * (group & 1) + 4 * p);
}

// ---- O ------------------------------------------------------------------------------------------------------
// Accumulator db = 0..3 holds O^T: register reg of lane l is d 32 db + (reg & 3) + 8 (reg >> 2) + 4 (l >> 5) of query
// l & 31, so registers 4g .. 4g+3 are four consecutive d: one 16-byte store, g = 0..3. The wide kernel stores to O,
// the split kernel to its wave's part of the merge.
NANOGPU_HD inline int o_col(int lane, int db, int g) { return 32 * db + 8 * g + 4 * (lane >> 5); }
NANOGPU_HD inline size_t o_index(bool split, int head, int qt, int sq, int wave, int lane, int db, int g) {
  return (query_row(split, head, qt, sq, wave) + static_cast<size_t>(lane & 31)) * kD + static_cast<size_t>(o_col(lane, db, g));
}
NANOGPU_HD inline int merge_o_index(int wave, int query, int d) { return wave * kMergeWaveWords + query * kMergeRow + d; }
NANOGPU_HD inline int merge_ml_index(int wave, int query, int which) { return kMergeMlAt + (wave * 32 + query) * 2 + which; }
// The merge: wave w combines d 32w .. 32w+31 of all 32 queries, pass i = 0..3 of lane l four consecutive d of one query.
NANOGPU_HD inline int merge_query(int lane, int i) { return 8 * i + (lane >> 3); }
NANOGPU_HD inline int merge_d(int wave, int lane) { return 32 * wave + 4 * (lane & 7); }

// 4 heads sq skv 128 FLOP a launch: two products of 2 sq skv 128 a head.
NANOGPU_HD inline double flop(double heads, double sq, double skv) { return 4.0 * heads * sq * skv * kD; }
// What a launch must move at the least: Q, K and V read once, O written once. A lower bound on HBM traffic.
NANOGPU_HD inline double compulsory_bytes(double heads, double sq, double skv) {
  return 2.0 * kD * heads * (sq + 2.0 * skv) + 4.0 * kD * heads * sq;
}

}  // namespace attn
}  // namespace nanogpu
