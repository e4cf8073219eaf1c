// Stand-alone check of the attention tenant's host definitions (nanogpu/attn_host.h), with no GPU code involved:
// `python native/build.py --selftest-host attn-asan` builds it under ASan + UBSan. attn_bf16_kernel has no tail code
// and forms every address from the header's index functions, so before anything runs on a GPU this program asserts
// the shape rules, that the block-to-(head, query tile) map is a bijection, and, while it replays small attentions
// through those functions lane by lane, that every global and LDS index lies inside its array and that every LDS read
// finds what the same tile wrote. The replay writes out the MFMA's lane maps, the transposed LDS read and the
// permutation of the kv index between P's registers and V's operand, and is compared with a direct softmax.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "nanogpu/attn_host.h"

namespace at = nanogpu::attn;
namespace gm = nanogpu::gemm;

static int failures = 0;

#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);  \
      if (++failures > 20) return;                                     \
    }                                                                  \
  } while (0)

static void check_shapes() {
  for (int sq = -32; sq <= 640; ++sq)
    for (int skv = -64; skv <= 512; skv += (skv % 64 == 0 || skv % 64 == -1 || skv % 64 == 63) ? 1 : 31) {
      const bool want = sq > 0 && skv > 0 && (sq < 128 ? sq % 32 == 0 && skv % 128 == 0 : sq % 128 == 0 && skv % 64 == 0);
      CHECK(at::shape_ok(1, sq, skv) == want);
    }
  CHECK(!at::shape_ok(0, 128, 64) && !at::shape_ok(-1, 128, 64) && !at::shape_ok(1, 160, 128));
  // 2^24 workgroups of 256 threads are 2^32 work-items
  CHECK(at::shape_ok((1 << 24) - 1, 32, 128) && !at::shape_ok(1 << 24, 32, 128) && at::shape_ok(1 << 12, 128 * 4095, 64) && !at::shape_ok(1 << 12, 128 * 4096, 64));
  CHECK(!at::shape_ok(1, int64_t(1) << 31, 64) && !at::shape_ok(1, 128, int64_t(1) << 31));
  CHECK(at::workgroups(5, 384) == 15 && at::workgroups(5, 96) == 15 && at::compulsory_bytes(2, 32, 128) == 256.0 * 2 * 288 + 512.0 * 2 * 32);
  CHECK(at::load_passes(false) == 4 && at::load_passes(true) == 8 && at::flop(1, 128, 64) == 4.0 * 128 * 64 * 128);
}

// Every (head, query tile) is some block's, once; and the largest admitted shapes' last indices, in 64 bits.
static void check_map_and_large() {
  for (int sq : {96, 384})
    for (int heads : {1, 3, 5, 11}) {
      const uint32_t grid = static_cast<uint32_t>(at::workgroups(heads, sq)), q_tiles = grid / heads;
      std::vector<int> seen(grid, 0);
      for (uint32_t b = 0; b < grid; ++b) {
        const at::PairAt p = at::pair_at(gm::tile_of_block(b, grid), sq);
        CHECK(p.head >= 0 && p.head < heads && p.qt >= 0 && static_cast<uint32_t>(p.qt) < q_tiles);
        ++seen[p.head * q_tiles + p.qt];
      }
      for (int v : seen) CHECK(v == 1);
    }
  CHECK(at::pair_at(7, 384).head == 2 && at::pair_at(7, 384).qt == 1);   // the query tile runs fastest
  struct Shape {
    int heads, sq, skv;
  };
  for (const Shape& s : {Shape{(1 << 24) - 1, 32, 1 << 30}, Shape{1 << 12, 128 * 4095, 1 << 30}}) {
    const bool split = at::is_split(s.sq);
    CHECK(at::shape_ok(s.heads, s.sq, s.skv));
    const size_t nq = static_cast<size_t>(s.heads) * s.sq * at::kD, nkv = static_cast<size_t>(s.heads) * s.skv * at::kD;
    const uint32_t grid = static_cast<uint32_t>(at::workgroups(s.heads, s.sq));
    const at::PairAt p = at::pair_at(grid - 1, s.sq);
    CHECK(at::q_global_index(split, p.head, p.qt, s.sq, 3, 63, 7) + at::kChunk == nq);
    CHECK(at::kv_global_index(split, p.head, s.skv / at::kv_tile(split) - 1, s.skv, 255, at::load_passes(split) - 1) + at::kChunk == nkv);
    CHECK(at::o_index(split, p.head, p.qt, s.sq, 3, 63, 3, 3) + 4 == nq);
  }
}

// The kernel, on the CPU: the same loops over the same index functions, doubles for bf16 and fp32.
static void replay(int heads, int sq, int skv) {
  CHECK(at::shape_ok(heads, sq, skv));
  const bool split = at::is_split(sq);
  const int blocks = at::blocks_per_wave(split), kv_tiles = skv / at::kv_tile(split);
  const size_t nq = static_cast<size_t>(heads) * sq * at::kD, nkv = static_cast<size_t>(heads) * skv * at::kD;
  std::vector<double> Q(nq), K(nkv), V(nkv), O(nq, -1.0);
  std::vector<int> stores(nq, 0);
  for (size_t x = 0; x < nq; ++x) Q[x] = (static_cast<int>((x * 2654435761u >> 7) % 17) - 8) / 4.0;
  for (size_t x = 0; x < nkv; ++x) K[x] = (static_cast<int>((x * 40503u >> 5) % 13) - 6) / 4.0, V[x] = (static_cast<int>((x * 69069u >> 3) % 15) - 7) / 8.0;
  const double scale = 1.0 / std::sqrt(128.0);
  const uint32_t grid = static_cast<uint32_t>(at::workgroups(heads, sq));
  std::vector<double> lds(at::kLdsElems), part(at::kMergeWords);
  std::vector<int> stamp(at::kLdsElems);   // the tile, plus one, that wrote the element
  for (uint32_t block = 0; block < grid; ++block) {
    const at::PairAt pr = at::pair_at(gm::tile_of_block(block, grid), sq);
    const int head = pr.head, qt = pr.qt;
    std::fill(stamp.begin(), stamp.end(), 0);
    auto at_lds = [&](int index, int kt, int lo, int hi) -> double {   // a read of tile kt inside [lo, hi)
      if (index < lo || index >= hi || stamp[index] != kt + 1) {
        ++failures;
        return 0.0;
      }
      return lds[index];
    };
    struct Lane {
      double m = -1e30, l = 0.0, o[4][16] = {};
    };
    std::vector<Lane> state(at::kThreads);
    for (int kt = 0; kt < kv_tiles; ++kt) {
      const int stage = at::stages(split) == 2 ? kt & 1 : 0;
      const int k_lo = stage * at::k_stage_elems(split), v_lo = at::v_at(split) + stage * at::v_stage_elems(split);
      for (int t = 0; t < at::kThreads; ++t)
        for (int i = 0; i < at::load_passes(split); ++i) {
          const size_t g = at::kv_global_index(split, head, kt, skv, t, i);
          const int k = at::k_lds_index(split, stage, at::kv_load_row(t, i), at::kv_load_chunk(t));
          const int v = at::v_lds_index(split, stage, at::kv_load_row(t, i), at::kChunk * at::kv_load_chunk(t));
          CHECK(g + at::kChunk <= nkv && g % at::kChunk == 0 && k % at::kChunk == 0 && v % at::kChunk == 0);
          CHECK(k >= k_lo && k + at::kChunk <= k_lo + at::k_stage_elems(split) && v >= v_lo && v + at::kChunk <= v_lo + at::v_stage_elems(split));
          for (int e = 0; e < at::kChunk; ++e) {
            CHECK(stamp[k + e] != kt + 1 && stamp[v + e] != kt + 1);
            lds[k + e] = K[g + e], lds[v + e] = V[g + e], stamp[k + e] = stamp[v + e] = kt + 1;
          }
        }
      for (int wave = 0; wave < 4; ++wave) {
        Lane* w = &state[wave * 64];
        std::vector<double> sc(static_cast<size_t>(blocks) * 64 * 16, 0.0);   // [b][lane][reg]
        for (int b = 0; b < blocks; ++b)
          for (int s = 0; s < 8; ++s) {
            double a[64][8], q[64][8];
            for (int lane = 0; lane < 64; ++lane) {
              const size_t g = at::q_global_index(split, head, qt, sq, wave, lane, s);
              CHECK(g + at::kChunk <= nq && g % at::kChunk == 0);
              for (int e = 0; e < 8; ++e) {
                a[lane][e] = at_lds(at::k_read_index(split, stage, wave, lane, b, s) + e, kt, k_lo, k_lo + at::k_stage_elems(split));
                q[lane][e] = Q[g + e];
              }
            }
            for (int lane = 0; lane < 64; ++lane)
              for (int reg = 0; reg < 16; ++reg)
                for (int half = 0; half < 2; ++half)
                  for (int e = 0; e < 8; ++e) sc[(b * 64 + lane) * 16 + reg] += a[at::score_kv_row(lane, reg) + 32 * half][e] * q[(lane & 31) + 32 * half][e];
          }
        for (int lane = 0; lane < 64; ++lane) {   // the maximum of a query over its two lanes, and the rescale
          double mx = w[lane].m;
          for (int b = 0; b < blocks; ++b)
            for (int reg = 0; reg < 16; ++reg) mx = std::max({mx, sc[(b * 64 + lane) * 16 + reg], sc[(b * 64 + (lane ^ 32)) * 16 + reg]});
          const double alpha = std::exp((w[lane].m - mx) * scale);
          w[lane].m = mx, w[lane].l *= alpha;
          for (auto& acc : w[lane].o)
            for (double& x : acc) x *= alpha;
        }
        for (int b = 0; b < blocks; ++b) {
          for (int lane = 0; lane < 64; ++lane)
            for (int reg = 0; reg < 16; ++reg) {
              double& p = sc[(b * 64 + lane) * 16 + reg];
              p = std::exp((p - w[lane].m) * scale);
              w[lane].l += p;
            }
          for (int u = 0; u < 2; ++u)
            for (int db = 0; db < 4; ++db) {
              double vt[64][8];
              for (int lane = 0; lane < 64; ++lane)
                for (int e = 0; e < 8; ++e)
                  vt[lane][e] = at_lds(at::v_read_index(split, stage, wave, gm::tr_source_lane(lane, e & 3), b, u, db, e >> 2) + gm::tr_source_elem(lane),
                                       kt, v_lo, v_lo + at::v_stage_elems(split));
              for (int lane = 0; lane < 64; ++lane)
                for (int reg = 0; reg < 16; ++reg)
                  for (int half = 0; half < 2; ++half)
                    for (int j = 0; j < 8; ++j)
                      w[lane].o[db][reg] += vt[at::score_kv_row(lane, reg) + 32 * half][j] * sc[(b * 64 + (lane & 31) + 32 * half) * 16 + at::p_reg(u, j)];
            }
        }
      }
    }
    auto store = [&](size_t index, double value) {
      if (index >= nq) {
        ++failures;
        return;
      }
      O[index] = value, ++stores[index];
    };
    for (int wave = 0; wave < 4; ++wave)
      for (int lane = 0; lane < 64; ++lane) {
        const Lane& s = state[wave * 64 + lane];
        const double l = s.l + state[wave * 64 + (lane ^ 32)].l;
        for (int db = 0; db < 4; ++db)
          for (int g = 0; g < 4; ++g)
            for (int x = 0; x < 4; ++x) {
              if (!split) {
                store(at::o_index(split, head, qt, sq, wave, lane, db, g) + x, s.o[db][4 * g + x] / l);
                continue;
              }
              const int at_part = at::merge_o_index(wave, lane & 31, at::o_col(lane, db, g)) + x;
              CHECK(at_part >= 0 && at_part < at::kMergeMlAt);
              part[at_part] = s.o[db][4 * g + x];
            }
        if (lane < 32) part[at::merge_ml_index(wave, lane, 0)] = s.m, part[at::merge_ml_index(wave, lane, 1)] = l;
        CHECK(at::merge_ml_index(wave, lane & 31, 1) < at::kMergeWords);
      }
    if (!split) continue;
    for (int wave = 0; wave < 4; ++wave)
      for (int lane = 0; lane < 64; ++lane)
        for (int i = 0; i < 4; ++i) {
          const int query = at::merge_query(lane, i), d = at::merge_d(wave, lane);
          double top = -1e30, sum = 0.0, acc[4] = {};
          for (int w = 0; w < 4; ++w) top = std::max(top, part[at::merge_ml_index(w, query, 0)]);
          for (int w = 0; w < 4; ++w) {
            const double weight = std::exp((part[at::merge_ml_index(w, query, 0)] - top) * scale);
            sum += weight * part[at::merge_ml_index(w, query, 1)];
            for (int x = 0; x < 4; ++x) acc[x] += weight * part[at::merge_o_index(w, query, d) + x];
          }
          for (int x = 0; x < 4; ++x) store((at::query_row(split, head, qt, sq, 0) + query) * at::kD + d + x, acc[x] / sum);
        }
  }
  for (int head = 0; head < heads; ++head)
    for (int q = 0; q < sq; ++q) {
      std::vector<double> p(skv);
      double top = -1e30, sum = 0.0;
      const double* qr = &Q[(static_cast<size_t>(head) * sq + q) * at::kD];
      for (int r = 0; r < skv; ++r) {
        p[r] = 0.0;
        for (int d = 0; d < at::kD; ++d) p[r] += qr[d] * K[(static_cast<size_t>(head) * skv + r) * at::kD + d];
        top = std::max(top, p[r]);
      }
      for (int r = 0; r < skv; ++r) sum += p[r] = std::exp((p[r] - top) * scale);
      for (int d = 0; d < at::kD; ++d) {
        double want = 0.0;
        for (int r = 0; r < skv; ++r) want += p[r] * V[(static_cast<size_t>(head) * skv + r) * at::kD + d];
        const size_t x = (static_cast<size_t>(head) * sq + q) * at::kD + d;
        CHECK(stores[x] == 1);
        CHECK(std::fabs(O[x] - want / sum) <= 1e-12);
      }
    }
}

int main() {
  check_shapes();
  check_map_and_large();
  replay(1, 128, 64);    // wide, the smallest: one workgroup, one tile
  replay(3, 256, 192);   // wide: 6 workgroups, a stage reused
  replay(1, 32, 128);    // split, the smallest
  replay(3, 96, 256);    // split: 9 workgroups, the re-numbering, two tiles and the merge
  if (failures) {
    std::fprintf(stderr, "%d failures\n", failures);
    return 1;
  }
  std::printf("{\"ok\": true, \"lds_bytes\": %d, \"wide\": [%d, %d, %d], \"split\": [%d, %d, %d]}\n", at::kLdsBytes, at::q_tile(false),
              at::kv_tile(false), at::stages(false), at::q_tile(true), at::kv_tile(true), at::stages(true));
  return 0;
}
