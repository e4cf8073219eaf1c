// Stand-alone check of the GEMM tenant's host definitions (nanogpu/gemm_host.h), with no GPU code involved:
// `python native/build.py --selftest-host gemm-asan` builds it under ASan + UBSan. gemm_bf16_kernel has no tail
// code and forms every address from the header's index functions, so before anything runs on a GPU this program
// asserts that the workgroup-to-tile map is a bijection for every grid of 1..4096 workgroups, that the shape check
// accepts exactly the multiples of the tile, and that every global and LDS index lies inside its array. It then
// replays products of up to 22 workgroups through those functions, lane by lane, with the transposed LDS read and the
// MFMA's lane maps written out, and compares it with the plain triple loop.
#include <cstdio>
#include <vector>

#include "nanogpu/gemm_host.h"

namespace gm = nanogpu::gemm;

static int failures = 0;

#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);  \
      if (++failures > 20) return;                                     \
    }                                                                  \
  } while (0)

static void check_tile_map() {
  std::vector<uint32_t> seen;
  for (uint32_t g = 1; g <= 4096; ++g) {
    seen.assign(g, 0);
    for (uint32_t b = 0; b < g; ++b) {
      const uint32_t t = gm::tile_of_block(b, g);
      CHECK(t < g);
      if (t < g) ++seen[t];
    }
    for (uint32_t t = 0; t < g; ++t) CHECK(seen[t] == 1);
  }
  // the blocks of one XCD take one contiguous run: 15 workgroups, XCD 0 has tiles 0 and 1, XCD 7 tile 14
  CHECK(gm::tile_of_block(0, 15) == 0 && gm::tile_of_block(8, 15) == 1 && gm::tile_of_block(1, 15) == 2 && gm::tile_of_block(7, 15) == 14);
  CHECK(gm::tile_of_block(9, 16) == 3 && gm::tile_of_block(4, 5) == 4);
  // bands of 8 row panels, walked down the rows first; 3 row panels make one band of 3, 11 a band of 8 and one of 3
  CHECK(gm::tile_at(7, 384, 640).m == 1 && gm::tile_at(7, 384, 640).n == 2 && gm::tile_at(9, 1408, 256).m == 1 && gm::tile_at(9, 1408, 256).n == 1);
  CHECK(gm::tile_at(16, 1408, 256).m == 8 && gm::tile_at(16, 1408, 256).n == 0 && gm::tile_at(21, 1408, 256).m == 10 && gm::tile_at(21, 1408, 256).n == 1);
}

static void check_shapes() {
  for (int m = -128; m <= 512; ++m)
    for (int k = -64; k <= 256; ++k) {
      CHECK(gm::shape_ok(m, 128, k) == (m > 0 && m % 128 == 0 && k > 0 && k % 64 == 0));
      CHECK(gm::shape_ok(128, m, k) == (m > 0 && m % 128 == 0 && k > 0 && k % 64 == 0));
    }
  // 2^24 tiles of 256 threads are 2^32 work-items
  CHECK(gm::shape_ok(128 * 4096, 128 * 4095, 64) && !gm::shape_ok(128 * 4096, 128 * 4096, 64));
  CHECK(gm::shape_ok(128, int64_t(128) * ((1 << 23) - 1), 64) && !gm::shape_ok(128, int64_t(1) << 31, 64) && !gm::shape_ok(128, 128, int64_t(1) << 31));
  CHECK(gm::tiles(384, 640) == 15 && gm::compulsory_bytes(128, 256, 64) == 2.0 * 64 * 384 + 4.0 * 128 * 256);
}

// Every LDS index of every thread, and that a stage's writes cover it exactly once and stay off the other stage.
static void check_lds() {
  for (int stage = 0; stage < gm::kStages; ++stage) {
    std::vector<int> written(gm::kLdsElems, 0);
    for (int t = 0; t < gm::kThreads; ++t)
      for (int i = 0; i < gm::kLoadPasses; ++i) {
        const int a = gm::a_lds_index(stage, gm::a_load_row(t, i), gm::a_load_chunk(t));
        const int b = gm::b_lds_index(stage, gm::b_load_row(t, i), gm::kChunk * gm::b_load_chunk(t));
        CHECK(a % gm::kChunk == 0 && a >= stage * gm::kAStageElems && a + gm::kChunk <= (stage + 1) * gm::kAStageElems);
        CHECK(b % gm::kChunk == 0 && b >= gm::kBAt + stage * gm::kBStageElems && b + gm::kChunk <= gm::kBAt + (stage + 1) * gm::kBStageElems);
        for (int e = 0; e < gm::kChunk; ++e) ++written[a + e], ++written[b + e];
      }
    int total = 0;
    for (int v : written) {
      CHECK(v <= 1);
      total += v;
    }
    CHECK(total == gm::kBM * gm::kBK + gm::kBK * gm::kBN);
    for (int wave = 0; wave < 4; ++wave)
      for (int lane = 0; lane < 64; ++lane)
        for (int s = 0; s < 4; ++s)
          for (int x = 0; x < 2; ++x) {
            const int a = gm::a_read_index(stage, wave, lane, s, x);
            CHECK(a % gm::kChunk == 0 && a >= 0 && a + gm::kChunk <= gm::kBAt);
            for (int e = 0; e < gm::kChunk; ++e) CHECK(written[a + e] == 1);
            for (int h = 0; h < 2; ++h) {
              const int b = gm::b_read_index(stage, wave, lane, s, x, h);
              CHECK(b % 4 == 0 && b >= gm::kBAt && b + 4 <= gm::kLdsElems);
              for (int e = 0; e < 4; ++e) CHECK(written[b + e] == 1);
              for (int e = 0; e < 4; ++e) CHECK((gm::tr_source_lane(lane, e) >> 4) == (lane >> 4));
            }
          }
  }
}

// The kernel, on the CPU: the same loops over the same index functions, integers for bf16.
static void replay(int m, int n, int k) {
  CHECK(gm::shape_ok(m, n, k));
  std::vector<int> A(static_cast<size_t>(m) * k), B(static_cast<size_t>(k) * n);
  std::vector<long> C(static_cast<size_t>(m) * n, -1);
  std::vector<int> stores(C.size(), 0);
  for (size_t x = 0; x < A.size(); ++x) A[x] = static_cast<int>((x * 2654435761u >> 7) % 17) - 8;
  for (size_t x = 0; x < B.size(); ++x) B[x] = static_cast<int>((x * 40503u >> 5) % 13) - 6;
  const uint32_t grid = static_cast<uint32_t>(gm::tiles(m, n));
  std::vector<int> lds(gm::kLdsElems);
  for (uint32_t block = 0; block < grid; ++block) {
    const uint32_t tile = gm::tile_of_block(block, grid);
    const gm::TileAt at = gm::tile_at(tile, m, n);
    const int tm = at.m, tn = at.n;
    CHECK(tm >= 0 && tm < m / gm::kBM && tn >= 0 && tn < n / gm::kBN);
    std::vector<long> acc(static_cast<size_t>(gm::kThreads) * 64, 0);   // [thread][i][j][reg]
    for (int kt = 0; kt < k / gm::kBK; ++kt) {
      const int stage = kt & 1;
      for (int t = 0; t < gm::kThreads; ++t)
        for (int i = 0; i < gm::kLoadPasses; ++i) {
          const size_t ga = gm::a_global_index(tm, kt, k, t, i), gb = gm::b_global_index(tn, kt, n, t, i);
          CHECK(ga + gm::kChunk <= A.size() && gb + gm::kChunk <= B.size());
          for (int e = 0; e < gm::kChunk; ++e) {
            lds[gm::a_lds_index(stage, gm::a_load_row(t, i), gm::a_load_chunk(t)) + e] = A[ga + e];
            lds[gm::b_lds_index(stage, gm::b_load_row(t, i), gm::kChunk * gm::b_load_chunk(t)) + e] = B[gb + e];
          }
        }
      for (int wave = 0; wave < 4; ++wave)
        for (int s = 0; s < 4; ++s)
          for (int i = 0; i < 2; ++i)
            for (int j = 0; j < 2; ++j) {
              // one MFMA: operands per lane, then C[row][col] += sum over the two lane halves' eight k
              int a[64][8], b[64][8];
              for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < 8; ++e) {
                  a[lane][e] = lds[gm::a_read_index(stage, wave, lane, s, i) + e];
                  const int src = gm::tr_source_lane(lane, e & 3);
                  b[lane][e] = lds[gm::b_read_index(stage, wave, src, s, j, e >> 2) + gm::tr_source_elem(lane)];
                }
              for (int lane = 0; lane < 64; ++lane)
                for (int reg = 0; reg < 16; ++reg) {
                  const int row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5), col = lane & 31;
                  long sum = 0;
                  for (int half = 0; half < 2; ++half)
                    for (int e = 0; e < 8; ++e) sum += static_cast<long>(a[row + 32 * half][e]) * b[col + 32 * half][e];
                  acc[((static_cast<size_t>(wave) * 64 + lane) * 4 + i * 2 + j) * 16 + reg] += sum;
                }
            }
    }
    for (int wave = 0; wave < 4; ++wave)
      for (int lane = 0; lane < 64; ++lane)
        for (int i = 0; i < 2; ++i)
          for (int j = 0; j < 2; ++j)
            for (int reg = 0; reg < 16; ++reg) {
              const size_t c = gm::c_index(tm, tn, n, wave, lane, i, j, reg);
              CHECK(c < C.size());
              if (c >= C.size()) continue;
              C[c] = acc[((static_cast<size_t>(wave) * 64 + lane) * 4 + i * 2 + j) * 16 + reg];
              ++stores[c];
            }
  }
  for (int r = 0; r < m; ++r)
    for (int c = 0; c < n; ++c) {
      long want = 0;
      for (int x = 0; x < k; ++x) want += static_cast<long>(A[static_cast<size_t>(r) * k + x]) * B[static_cast<size_t>(x) * n + c];
      CHECK(stores[static_cast<size_t>(r) * n + c] == 1);
      CHECK(C[static_cast<size_t>(r) * n + c] == want);
    }
}

// The largest shapes the check admits: the last thread's last index, in 64 bits.
static void check_large() {
  const int m = 128 * 4096, n = 128 * 4095, k = 1 << 20;
  CHECK(gm::shape_ok(m, n, k));
  const uint32_t grid = static_cast<uint32_t>(gm::tiles(m, n));
  size_t top_a = 0, top_b = 0, top_c = 0;
  for (uint32_t block : {0u, grid - 8, grid - 1}) {
    const uint32_t tile = gm::tile_of_block(block, grid);
    const gm::TileAt at = gm::tile_at(tile, m, n);
    const int tm = at.m, tn = at.n;
    for (int t : {0, gm::kThreads - 1}) {
      const size_t a = gm::a_global_index(tm, k / gm::kBK - 1, k, t, gm::kLoadPasses - 1) + gm::kChunk;
      const size_t b = gm::b_global_index(tn, k / gm::kBK - 1, n, t, gm::kLoadPasses - 1) + gm::kChunk;
      const size_t c = gm::c_index(tm, tn, n, t >> 6, t & 63, 1, 1, 15) + 1;
      CHECK(a <= static_cast<size_t>(m) * k && b <= static_cast<size_t>(k) * n && c <= static_cast<size_t>(m) * n);
      top_a = a > top_a ? a : top_a, top_b = b > top_b ? b : top_b, top_c = c > top_c ? c : top_c;
    }
  }
  CHECK(top_a == static_cast<size_t>(m) * k && top_b == static_cast<size_t>(k) * n && top_c == static_cast<size_t>(m) * n);
}

int main() {
  check_tile_map();
  check_shapes();
  check_lds();
  check_large();
  replay(128, 128, 192);   // one workgroup, a stage reused
  replay(384, 640, 128);   // 15 workgroups: the re-numbering, and row tiles unlike column tiles
  replay(1408, 256, 64);   // 22 workgroups: a whole band of 8 row panels and one of 3
  if (failures) return 1;
  std::printf("{\"ok\": true, \"lds_bytes\": %d, \"tile\": [%d, %d, %d]}\n", gm::kLdsBytes, gm::kBM, gm::kBN, gm::kBK);
  return 0;
}
