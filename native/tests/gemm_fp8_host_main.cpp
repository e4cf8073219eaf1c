// Stand-alone check of the FP8 GEMM tenant's host definitions (nanogpu/gemm_fp8_host.h), with no GPU code involved:
// `python native/build.py --selftest-host gemmfp8-asan` builds it under ASan + UBSan. gemm_fp8_kernel has no tail
// code and forms every address from the header's index functions, so before anything runs on a GPU this program
// asserts that every global and LDS index lies inside its array, that the swizzle is a bijection of a stage, and
// replays one product of 15 workgroups through those functions with the instruction's measured operand map (a wrong
// or incomplete map gives a wrong product). The tile map it shares with the bf16 tenant is gemm_host_main.cpp's.
#include <cstdio>
#include <vector>

#include "nanogpu/gemm_fp8_host.h"

namespace gm = nanogpu::gemm;
namespace g8 = nanogpu::gemm_fp8;

static int failures = 0;

#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);  \
      if (++failures > 20) return;                                     \
    }                                                                  \
  } while (0)

// A stage's writes cover it exactly once and stay off every other stage; every read lies in what was written.
static void check_lds() {
  for (int op = 0; op < g8::kOperands; ++op)
    for (int stage = 0; stage < g8::kStages; ++stage) {
      const int lo = (op * g8::kStages + stage) * g8::kStageBytes;
      std::vector<int> written(g8::kLdsBytes, 0);
      for (int t = 0; t < g8::kThreads; ++t)
        for (int i = 0; i < g8::kLoadPasses; ++i) {
          const int at = g8::lds_index(op, stage, g8::load_row(t, i), g8::load_chunk(t));
          CHECK(at % g8::kChunk == 0 && at >= lo && at + g8::kChunk <= lo + g8::kStageBytes);
          for (int e = 0; e < g8::kChunk; ++e) ++written[at + e];
        }
      for (int x = 0; x < g8::kLdsBytes; ++x) CHECK(written[x] == (x >= lo && x < lo + g8::kStageBytes));
      for (int wave = 0; wave < 4; ++wave)
        for (int lane = 0; lane < 64; ++lane)
          for (int s = 0; s < g8::kKSteps; ++s)
            for (int ij = 0; ij < 2; ++ij)
              for (int h = 0; h < 2; ++h) {
                const int at = g8::read_index(op, stage, wave, lane, s, ij, h);
                CHECK(at % g8::kChunk == 0 && at >= lo && at + g8::kChunk <= lo + g8::kStageBytes);
              }
    }
}

// The kernel, on the CPU: the same loops over the same index functions, small integers for e4m3. One MFMA sums, for
// every k of its 64, A's lane byte that the measured map (g8::mfma_k) puts at k with B's.
static void replay(int m, int n, int k) {
  CHECK(g8::shape_ok(m, n, k));
  std::vector<int> A(static_cast<size_t>(m) * k), B(static_cast<size_t>(n) * k);
  std::vector<long> C(static_cast<size_t>(m) * n, -1);
  std::vector<int> stores(C.size(), 0);
  for (size_t x = 0; x < A.size(); ++x) A[x] = static_cast<int>((x * 2654435761u >> 7) % 17) - 8;
  for (size_t x = 0; x < B.size(); ++x) B[x] = static_cast<int>((x * 40503u >> 5) % 13) - 6;
  const uint32_t grid = static_cast<uint32_t>(gm::tiles(m, n));
  std::vector<int> lds(g8::kLdsBytes);
  for (uint32_t block = 0; block < grid; ++block) {
    const gm::TileAt at = gm::tile_at(gm::tile_of_block(block, grid), m, n);
    const int tm = at.m, tn = at.n;
    CHECK(tm >= 0 && tm < m / g8::kBM && tn >= 0 && tn < n / g8::kBN);
    std::vector<long> acc(static_cast<size_t>(g8::kThreads) * 64, 0);   // [thread][i][j][reg]
    for (int kt = 0; kt < k / g8::kBK; ++kt) {
      const int stage = kt & 1;
      for (int t = 0; t < g8::kThreads; ++t)
        for (int i = 0; i < g8::kLoadPasses; ++i) {
          const size_t ga = g8::global_index(tm, kt, k, t, i), gb = g8::global_index(tn, kt, k, t, i);
          CHECK(ga + g8::kChunk <= A.size() && gb + g8::kChunk <= B.size());
          for (int e = 0; e < g8::kChunk; ++e) {
            lds[g8::lds_index(0, stage, g8::load_row(t, i), g8::load_chunk(t)) + e] = A[ga + e];
            lds[g8::lds_index(1, stage, g8::load_row(t, i), g8::load_chunk(t)) + e] = B[gb + e];
          }
        }
      for (int wave = 0; wave < 4; ++wave)
        for (int s = 0; s < g8::kKSteps; ++s)
          for (int i = 0; i < 2; ++i)
            for (int j = 0; j < 2; ++j) {
              int a[32][64], b[32][64];   // the instruction's view: [row | column][k]
              for (int lane = 0; lane < 64; ++lane)
                for (int byte = 0; byte < 32; ++byte) {
                  a[lane & 31][g8::mfma_k(lane, byte)] = lds[g8::read_index(0, stage, wave, lane, s, i, byte >> 4) + (byte & 15)];
                  b[lane & 31][g8::mfma_k(lane, byte)] = lds[g8::read_index(1, stage, wave, lane, s, j, byte >> 4) + (byte & 15)];
                }
              for (int lane = 0; lane < 64; ++lane)
                for (int reg = 0; reg < 16; ++reg) {
                  const int row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5), col = lane & 31;
                  long sum = 0;
                  for (int x = 0; x < 64; ++x) sum += static_cast<long>(a[row][x]) * b[col][x];
                  acc[((static_cast<size_t>(wave) * 64 + lane) * 4 + i * 2 + j) * 16 + reg] += sum;
                }
            }
    }
    for (int t = 0; t < g8::kThreads; ++t)
      for (int ij = 0; ij < 4; ++ij)
        for (int reg = 0; reg < 16; ++reg) {
          const size_t c = g8::c_index(tm, tn, n, t >> 6, t & 63, ij >> 1, ij & 1, reg);
          CHECK(c < C.size());
          if (c >= C.size()) continue;
          C[c] = acc[(static_cast<size_t>(t) * 4 + ij) * 16 + reg];
          ++stores[c];
        }
  }
  for (int r = 0; r < m; ++r)
    for (int c = 0; c < n; ++c) {
      long want = 0;
      for (int x = 0; x < k; ++x) want += static_cast<long>(A[static_cast<size_t>(r) * k + x]) * B[static_cast<size_t>(c) * k + x];
      CHECK(stores[static_cast<size_t>(r) * n + c] == 1);
      CHECK(C[static_cast<size_t>(r) * n + c] == want);
    }
}

// The first and last blocks' first and last threads reach the end of A, B and C and no further, in 64 bits.
static void check_bounds(int m, int n, int k) {
  CHECK(g8::shape_ok(m, n, k) && !g8::shape_ok(m, n, k + 64) && !g8::shape_ok(m + 64, n, k) && !g8::shape_ok(m, n - 64, k));
  const uint32_t grid = static_cast<uint32_t>(gm::tiles(m, n));
  size_t top_a = 0, top_b = 0, top_c = 0;
  for (uint32_t block : {0u, grid - (grid > 8 ? 8 : 1), grid - 1}) {
    const gm::TileAt at = gm::tile_at(gm::tile_of_block(block, grid), m, n);
    for (int t : {0, g8::kThreads - 1}) {
      const size_t a = g8::global_index(at.m, k / g8::kBK - 1, k, t, g8::kLoadPasses - 1) + g8::kChunk;
      const size_t b = g8::global_index(at.n, k / g8::kBK - 1, k, t, g8::kLoadPasses - 1) + g8::kChunk;
      const size_t c = g8::c_index(at.m, at.n, n, t >> 6, t & 63, 1, 1, 15) + 1;
      CHECK(a <= static_cast<size_t>(m) * k && b <= static_cast<size_t>(n) * k && c <= static_cast<size_t>(m) * n);
      top_a = a > top_a ? a : top_a, top_b = b > top_b ? b : top_b, top_c = c > top_c ? c : top_c;
    }
  }
  CHECK(top_a == static_cast<size_t>(m) * k && top_b == static_cast<size_t>(n) * k && top_c == static_cast<size_t>(m) * n);
}

int main() {
  check_lds();
  for (int k : {128, 384}) check_bounds(128, 128, k), check_bounds(256, 128, k), check_bounds(384, 640, k);
  check_bounds(128 * 4096, 128 * 4095, 1 << 20);   // the largest launch the shape check admits
  if (g8::shape_ok(128 * 4096, 128 * 4096, 128) || g8::compulsory_bytes(128, 256, 384) != 384.0 * 384 + 4.0 * 128 * 256) ++failures;
  replay(384, 640, 384);   // 15 workgroups, row tiles unlike column tiles, a stage reused
  if (failures) return 1;
  std::printf("{\"ok\": true, \"lds_bytes\": %d, \"tile\": [%d, %d, %d]}\n", g8::kLdsBytes, g8::kBM, g8::kBN, g8::kBK);
  return 0;
}
