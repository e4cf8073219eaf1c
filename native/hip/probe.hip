// nanogpu._probe — MI355X (gfx950) calibration kernels for the node agent.
//
// The reference scheduler never touches a GPU; it trusts an external NVIDIA device plugin
// to realise "gpu-percent" (reference README.md:9, 30-34). On MI355X the agent realises a
// fractional grant spatially: a container with p% of a device gets a CU mask covering
// ceil(p/100 * CUs) compute units, XCD-aligned where possible (each XCD has its own 4 MiB
// L2, so a grant that owns whole XCDs keeps its L2 to itself). These kernels measure the
// facts that mapping needs, on the real device:
//   * cu_census   — which XCD / SE / CU each CU-mask bit enables (s_getreg XCC_ID, HW_ID);
//   * mfma_burn   — bf16 MFMA throughput of a masked stream (isolation check: TFLOP/s
//                   must scale with the CUs granted);
//   * hbm_copy    — streaming HBM3E bandwidth (16 B/lane, grid >> 256 WGs);
//   * peer_bandwidth — per-pair xGMI rate: copy kernel pulling over peer access, and SDMA
//   * cu_sweep_kernel, hbm_fill / hbm_verify — the agent's deep self-test: every CU's MFMA
//                   pipes and LDS (`cu_sweep`), and free HBM against an address-derived pattern.
//   * matrix_tile_kernel, cu_sweep_kernel<kPaths> — the same sweep over the rest of the matrix
//                   unit (`cu_sweep_paths`): f16, fp8 / bf8, i8, block-scaled fp8 / fp6 / fp4,
//                   f32 and f64 MFMA.
//   * cu_valu_kernel, cu_scalar_kernel — the sweep's further parts on the same grid and stream: the
//                   vector ALU with the VGPR file (`cu_sweep_valu`), and the scalar ALU, scalar loads
//                   and the SGPR file (`cu_sweep_scalar`).
//   * cu_mem_kernel — and the CU's memory pipeline (`cu_sweep_mem`): global and buffer loads and
//                   stores, the L1, LDS instruction forms, the transposed read, LDS-DMA, atomics.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cstdint>
#include <cstring>
#include <memory>
#include <new>
#include <optional>
#include <stdexcept>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "nanogpu/selftest_host.h"
#include "nanogpu/selftest_mem_host.h"
#include "nanogpu/selftest_paths_host.h"
#include "nanogpu/selftest_scalar_host.h"
#include "nanogpu/selftest_valu_host.h"

namespace py = pybind11;

#define HIP_OK(expr)                                                                    \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess)                                                               \
      throw std::runtime_error(std::string(#expr) + ": " + hipGetErrorString(e_));      \
  } while (0)

namespace {

namespace st = nanogpu::selftest;

// ---------------------------------------------------------------------------- kernels

// Streaming copy: each thread keeps kCopyUnroll 16-B loads in flight before its stores
// (one pass, no grid-stride loop: the grid is n / 4096 workgroups, >> 256 CUs), with
// non-temporal hints so the once-touched stream does not evict L2/MALL.
using f32x4 = __attribute__((ext_vector_type(4))) float;
constexpr int kCopyUnroll = 4;
constexpr int kCopyBlock = 256;

__global__ __launch_bounds__(kCopyBlock) void hbm_copy(const float4* __restrict__ src,
                                                       float4* __restrict__ dst, size_t n) {
  const size_t base = static_cast<size_t>(blockIdx.x) * (kCopyBlock * kCopyUnroll) + threadIdx.x;
  if (base + (kCopyUnroll - 1) * kCopyBlock < n) {
    const f32x4* s4 = reinterpret_cast<const f32x4*>(src) + base;
    f32x4* d4 = reinterpret_cast<f32x4*>(dst) + base;
    f32x4 v[kCopyUnroll];
#pragma unroll
    for (int u = 0; u < kCopyUnroll; ++u) v[u] = __builtin_nontemporal_load(s4 + u * kCopyBlock);
#pragma unroll
    for (int u = 0; u < kCopyUnroll; ++u) __builtin_nontemporal_store(v[u], d4 + u * kCopyBlock);
  } else {
    for (int u = 0; u < kCopyUnroll; ++u)
      if (base + u * kCopyBlock < n) dst[base + u * kCopyBlock] = src[base + u * kCopyBlock];
  }
}

static_assert(kCopyBlock == st::kLaunchThreads && kCopyBlock * kCopyUnroll == st::kBlockElements,
              "launch_spans counts blocks of this shape");

// HIP supports no launch of 2^32 work-items or more: with 256 threads a block, 2^24 blocks
// (256 GiB of float4). Nobody measures a copy that large, so it is refused, before any allocation.
inline unsigned copy_grid(size_t n) {
  const uint64_t blocks = st::span_blocks(n);
  if (blocks * st::kLaunchThreads >= st::kWorkItemLimit)
    throw std::invalid_argument("hbm_copy: " + std::to_string(n) + " elements need 2^32 work-items or more in one launch");
  return static_cast<unsigned>(blocks);
}

// mfma_burn's blocks of 256 threads, under the same limit.
inline void check_burn_blocks(int blocks) {
  if (blocks <= 0 || static_cast<uint64_t>(blocks) * 256 >= st::kWorkItemLimit)
    throw std::invalid_argument("mfma_burn: block count in 1..2^24 - 1");
}

// One record per workgroup: {xcc_id, hw_id, block}. A bounded sleep keeps each workgroup
// resident long enough that the dispatcher spreads the grid over every enabled CU.
__global__ __launch_bounds__(64) void cu_census(uint32_t* out, int sleep_iters) {
  if (threadIdx.x != 0) return;
  uint32_t xcc, hwid;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
  for (int i = 0; i < sleep_iters; ++i) __builtin_amdgcn_s_sleep(16);
  out[3 * blockIdx.x + 0] = xcc;
  out[3 * blockIdx.x + 1] = hwid;
  out[3 * blockIdx.x + 2] = blockIdx.x;
}

using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using f32x16 = __attribute__((ext_vector_type(16))) float;

// MFMA-bound burn: 4 independent 32x32x16 bf16 accumulator chains per wave hide the
// dependent-accumulator latency; each MFMA is 2*32*32*16 = 32768 FLOP.
__global__ __launch_bounds__(256) void mfma_burn(float* out, int iters) {
  const int lane = threadIdx.x & 63;
  bf16x8 a, b;
  for (int j = 0; j < 8; ++j) {
    a[j] = static_cast<__bf16>(0.001f * static_cast<float>((lane + j) & 7));
    b[j] = static_cast<__bf16>(0.002f * static_cast<float>((lane * 3 + j) & 7));
  }
  f32x16 c0 = {}, c1 = {}, c2 = {}, c3 = {};
  for (int i = 0; i < iters; ++i) {
    c0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c0, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b, a, c1, 0, 0, 0);
    c2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, a, c2, 0, 0, 0);
    c3 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b, b, c3, 0, 0, 0);
  }
  float s = 0.f;
  for (int r = 0; r < 16; ++r) s += c0[r] + c1[r] + c2[r] + c3[r];
  if (s == 12345.678f) out[blockIdx.x * blockDim.x + threadIdx.x] = s;  // keeps the chains live
}

// One wave computes C[32x32] = A[32x16] * B[16x32] with a single bf16 MFMA: the numerics
// self-test of the burn kernel's instruction (operand/accumulator lane maps per
// cdna_hip_programming.md §3: lane l holds A[l&31][8(l>>5)+j], B[8(l>>5)+j][l&31];
// C row = (reg&3) + 8(reg>>2) + 4(l>>5), col = l&31).
__global__ __launch_bounds__(64) void mfma_tile(const __bf16* __restrict__ A, const __bf16* __restrict__ B,
                                                float* __restrict__ C) {
  const int l = threadIdx.x, r = l & 31, h = l >> 5;
  bf16x8 a, b;
  for (int j = 0; j < 8; ++j) {
    a[j] = A[r * 16 + 8 * h + j];
    b[j] = B[(8 * h + j) * 32 + r];
  }
  f32x16 c = {};
  c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  for (int reg = 0; reg < 16; ++reg) C[((reg & 3) + 8 * (reg >> 2) + 4 * h) * 32 + r] = c[reg];
}

// ---------------------------------------------------------------------------- deep self-test

constexpr int kSweepBlock = 256;               // 4 waves: one per SIMD's MFMA pipe
constexpr uint32_t kLdsDwordsFull = 40960;     // 160 KiB: the whole LDS of a gfx950 CU
enum : int { kInjectNone = 0, kInjectMfma = 1, kInjectLds = 2, kInjectPath = 3 };

// Test hook: the workgroup running on CU (xcc, cu_key) flips one bit of data it owns: of the
// bf16 accumulator, of LDS dword `lds_off`, or of path `path`'s accumulator (cu_sweep_paths only).
struct SweepInject {
  int xcc = -1, cu_key = -1, kind = kInjectNone;
  uint32_t lds_off = 0;
  int path = -1;
};

// ---- matrix paths (selftest_paths_host.h) ----
namespace sp = nanogpu::selftest::paths;

using u32x4v = __attribute__((ext_vector_type(4))) uint32_t;
using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
using i32x4 = __attribute__((ext_vector_type(4))) int;
using i32x8 = __attribute__((ext_vector_type(8))) int;
using i32x16 = __attribute__((ext_vector_type(16))) int;
using f64x4 = __attribute__((ext_vector_type(4))) double;

template <int P> struct AccOf { using type = f32x16; };
template <> struct AccOf<sp::kI8> { using type = i32x16; };
template <> struct AccOf<sp::kF64> { using type = f64x4; };

// Operand lane maps, confirmed on MI355X with matrix_tile on asymmetric random codes and
// scales (tests/test_gpu_selftest_paths.py). Lane l of a 32x32 path holds row (A) or column
// (B) l & 31; its operand dwords are dwords of the row's little-endian code string, code j of
// a dword string in bits [j * code_bits, (j + 1) * code_bits).
//   f16 / fp8 / bf8 32x32x16: k = 8 (l >> 5) + j, j = 0..7;  i8 32x32x32: k = 16 (l >> 5) + j;
//   f32 32x32x2: k = l >> 5;  f64 16x16x4: lane l holds A[l & 15][l >> 4] and B[l >> 4][l & 15].
//   Scaled 32x32x64, e2m3 and e2m1: k = 32 (l >> 5) + j, j = 0..31, in 6 resp. 4 of the 8
//   operand dwords (the rest 0): the lane holds one whole 32-element scale block.
//   Scaled 32x32x64, e4m3: NOT consecutive. Dwords 0..3 hold k = 16 (l >> 5) + j and dwords
//   4..7 hold k = 32 + 16 (l >> 5) + j, j = 0..15: a lane holds half of each scale block.
//   Scales, every format: the lane with l >> 5 == b supplies row / column (l & 31)'s E8M0
//   scale of k block b (k = 32 b .. 32 b + 31), in byte `opsel` (0..3) of its scale register.
// C / D: 32x32 row = (reg & 3) + 8 (reg >> 2) + 4 (l >> 5), col = l & 31, whatever the
// format; f64: row = (l >> 4) + 4 reg, col = l & 15.
template <int P> struct LaneMap {
  static constexpr int kGroupShift = P == sp::kF64 ? 4 : 5;
  static constexpr int kDwords = sp::path_row_dwords(P) >> (6 - kGroupShift);   // per lane and operand
  static constexpr int kRegs = P == sp::kF64 ? 4 : 16;
  // which dword of the row's code string is dword j of the lane in group g
  __device__ static constexpr int dword(int g, int j) {
    return P == sp::kMxFp8 ? 8 * (j >> 2) + 4 * g + (j & 3) : g * kDwords + j;
  }
  __device__ static int idx(int lane) { return lane & ((1 << kGroupShift) - 1); }
  __device__ static int group(int lane) { return lane >> kGroupShift; }
  __device__ static int row(int lane, int reg) {
    return P == sp::kF64 ? group(lane) + 4 * reg : (reg & 3) + 8 * (reg >> 2) + 4 * group(lane);
  }
};

// One instruction of path P on the lane's packed operand dwords (plain C++ packing).
template <int P, int OA, int OB>
__device__ __forceinline__ typename AccOf<P>::type path_mfma(const uint32_t (&a)[8], const uint32_t (&b)[8], uint32_t sa,
                                                             uint32_t sb, typename AccOf<P>::type c) {
  if constexpr (P == sp::kF16) {
    const u32x4v av = {a[0], a[1], a[2], a[3]}, bv = {b[0], b[1], b[2], b[3]};
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, av), __builtin_bit_cast(f16x8, bv), c, 0, 0, 0);
  } else if constexpr (P == sp::kFp8 || P == sp::kBf8) {
    const long av = static_cast<long>((static_cast<uint64_t>(a[1]) << 32) | a[0]);
    const long bv = static_cast<long>((static_cast<uint64_t>(b[1]) << 32) | b[0]);
    if constexpr (P == sp::kFp8)
      return __builtin_amdgcn_mfma_f32_32x32x16_fp8_fp8(av, bv, c, 0, 0, 0);
    else
      return __builtin_amdgcn_mfma_f32_32x32x16_bf8_bf8(av, bv, c, 0, 0, 0);
  } else if constexpr (P == sp::kI8) {
    const i32x4 av = {int(a[0]), int(a[1]), int(a[2]), int(a[3])}, bv = {int(b[0]), int(b[1]), int(b[2]), int(b[3])};
    return __builtin_amdgcn_mfma_i32_32x32x32_i8(av, bv, c, 0, 0, 0);
  } else if constexpr (sp::path_scaled(P)) {
    const i32x8 av = {int(a[0]), int(a[1]), int(a[2]), int(a[3]), int(a[4]), int(a[5]), int(a[6]), int(a[7])};
    const i32x8 bv = {int(b[0]), int(b[1]), int(b[2]), int(b[3]), int(b[4]), int(b[5]), int(b[6]), int(b[7])};
    constexpr int kFmt = sp::path_fmt_select(P);   // cbsz and blgp are immediates
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(av, bv, c, kFmt, kFmt, OA, static_cast<int>(sa), OB,
                                                           static_cast<int>(sb));
  } else if constexpr (P == sp::kF32) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a[0]), __uint_as_float(b[0]), c, 0, 0, 0);
  } else {
    static_assert(P == sp::kF64, "unknown path");
    const double av = __longlong_as_double(static_cast<long long>((static_cast<uint64_t>(a[1]) << 32) | a[0]));
    const double bv = __longlong_as_double(static_cast<long long>((static_cast<uint64_t>(b[1]) << 32) | b[0]));
    return __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, c, 0, 0, 0);
  }
}

// The accumulator's register `reg` as the 32-bit words the expected tile holds at `at`.
template <int P>
__device__ __forceinline__ bool acc_differs(const typename AccOf<P>::type& c, int reg, const uint32_t* __restrict__ tile,
                                            int at, uint32_t flip) {
  if constexpr (P == sp::kF64) {
    const uint64_t got = static_cast<uint64_t>(__double_as_longlong(c[reg])) ^ flip;
    return got != ((static_cast<uint64_t>(tile[2 * at + 1]) << 32) | tile[2 * at]);
  } else if constexpr (P == sp::kI8) {
    return (static_cast<uint32_t>(c[reg]) ^ flip) != tile[at];
  } else {
    return (__float_as_uint(c[reg]) ^ flip) != tile[at];
  }
}

// One wave, one instruction on the caller's packed codes: A and B hold path_row_dwords(P)
// dwords per row / column, SA and SB one scale dword per (row | column, k block). C is written
// row-major in the expected tile's words (matrix_tile establishes the lane maps above).
template <int P, int OA, int OB>
__global__ __launch_bounds__(64) void matrix_tile_kernel(const uint32_t* __restrict__ A, const uint32_t* __restrict__ B,
                                                         const uint32_t* __restrict__ SA, const uint32_t* __restrict__ SB,
                                                         uint32_t* __restrict__ C) {
  using M = LaneMap<P>;
  const int l = threadIdx.x, idx = M::idx(l), g = M::group(l);
  uint32_t a[8] = {}, b[8] = {};
#pragma unroll
  for (int j = 0; j < M::kDwords; ++j) {
    a[j] = A[idx * sp::path_row_dwords(P) + M::dword(g, j)];
    b[j] = B[idx * sp::path_row_dwords(P) + M::dword(g, j)];
  }
  uint32_t sa = 0, sb = 0;
  if constexpr (sp::path_scaled(P)) {
    sa = SA[idx * 2 + g];
    sb = SB[idx * 2 + g];
  }
  typename AccOf<P>::type c = {};
  c = path_mfma<P, OA, OB>(a, b, sa, sb, c);
  const int dim = sp::path_dim(P);
#pragma unroll
  for (int reg = 0; reg < M::kRegs; ++reg) {
    const int at = M::row(l, reg) * dim + idx;
    if constexpr (P == sp::kF64) {
      const uint64_t v = static_cast<uint64_t>(__double_as_longlong(c[reg]));
      C[2 * at] = static_cast<uint32_t>(v);
      C[2 * at + 1] = static_cast<uint32_t>(v >> 32);
    } else if constexpr (P == sp::kI8) {
      C[at] = static_cast<uint32_t>(c[reg]);
    } else {
      C[at] = __float_as_uint(c[reg]);
    }
  }
}

template <int P, int S>
__device__ __forceinline__ void path_step(int idx, int g, typename AccOf<P>::type& c) {
  using M = LaneMap<P>;
  uint32_t a[8] = {}, b[8] = {};
#pragma unroll
  for (int j = 0; j < M::kDwords; ++j) {
    a[j] = sp::path_dword(P, 0, S, idx, M::dword(g, j));
    b[j] = sp::path_dword(P, 1, S, idx, M::dword(g, j));
  }
  uint32_t sa = 0, sb = 0;
  if constexpr (sp::path_scaled(P)) {
    sa = sp::path_scale_dword(P, 0, S, idx, g);
    sb = sp::path_scale_dword(P, 1, S, idx, g);
  }
  c = path_mfma<P, sp::path_opsel(0, S), sp::path_opsel(1, S)>(a, b, sa, sb, c);
}

// The chain of kPathSteps accumulating instructions of path P on this wave, compared bit for
// bit with the host's tile (`tiles` + P * kTileWords; the sweep passes its copy in LDS). `flip` is the test hook's bit, XORed
// into the value of register 0 before the comparison.
template <int P>
__device__ __forceinline__ bool path_chain_differs(int lane, const uint32_t* __restrict__ tiles, uint32_t flip) {
  using M = LaneMap<P>;
  static_assert(sp::kPathSteps == 8, "the chain is unrolled by hand: the scale byte selects are immediates");
  const int idx = M::idx(lane), g = M::group(lane);
  typename AccOf<P>::type c = {};
  path_step<P, 0>(idx, g, c);
  path_step<P, 1>(idx, g, c);
  path_step<P, 2>(idx, g, c);
  path_step<P, 3>(idx, g, c);
  path_step<P, 4>(idx, g, c);
  path_step<P, 5>(idx, g, c);
  path_step<P, 6>(idx, g, c);
  path_step<P, 7>(idx, g, c);
  const uint32_t* tile = tiles + P * sp::kTileWords;
  bool bad = false;
#pragma unroll
  for (int reg = 0; reg < M::kRegs; ++reg)
    bad |= acc_differs<P>(c, reg, tile, M::row(lane, reg) * sp::path_dim(P) + idx, reg == 0 ? flip : 0u);
  return bad;
}

template <int P>
__device__ __forceinline__ uint32_t path_checked(uint32_t paths, int lane, const uint32_t* __restrict__ tiles,
                                                 int inject_path) {
  if (!(paths >> P & 1u)) return 0u;   // wave-uniform
  return path_chain_differs<P>(lane, tiles, inject_path == P ? 1u : 0u) ? 1u << P : 0u;
}

using AllPaths = std::make_integer_sequence<int, sp::kNumPaths>;   // the one list of the paths

// Bit P is set when selected path P's chain differed; the chains run in index order.
template <int... P>
__device__ __forceinline__ uint32_t paths_checked(std::integer_sequence<int, P...>, uint32_t paths, int lane,
                                                  const uint32_t* __restrict__ tiles, int inject_path) {
  uint32_t bad = 0;
  ((bad |= path_checked<P>(paths, lane, tiles, inject_path)), ...);
  return bad;
}

// One visit of one CU: every wave runs the exact MFMA chain and compares its accumulators
// bit for bit with the host's integer tile (C layout as in mfma_tile); the workgroup then
// writes mix32(i ^ seed) over `n` LDS dwords, reads it back through other threads than the
// writers, and repeats with the complement. One record per workgroup (selftest_host.h).
// No spin, no inter-workgroup traffic; every loop is bounded by `n` or a constant.
// kPaths: the visit also runs the chain of every path in `paths` on all four waves, against
// `tiles` (kNumPaths x kTileWords words), and writes the 7-word record of selftest_paths_host.h.
// The tiles are first staged in the LDS array, which the pattern test overwrites afterwards:
// one round of global loads per workgroup, in flight during the bf16 chain, instead of one
// round trip per path and wave (n >= kNumPaths * kTileWords is the host's to ensure).
template <bool kPaths>
__device__ __forceinline__ void sweep_body(uint32_t* lds, uint32_t n, const float* __restrict__ expected,
                                           uint32_t* __restrict__ out, uint32_t seed, SweepInject inj,
                                           uint32_t paths, const uint32_t* __restrict__ tiles) {
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;
  uint32_t xcc, hwid;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
  const bool mine = inj.kind != kInjectNone && xcc == static_cast<uint32_t>(inj.xcc) &&
                    st::hw_cu_key(hwid) == static_cast<uint32_t>(inj.cu_key);
  constexpr uint32_t kStaged4 = sp::kNumPaths * sp::kTileWords / 4;
  if constexpr (kPaths) {
    const u32x4v* src = reinterpret_cast<const u32x4v*>(tiles);
    u32x4v* dst = reinterpret_cast<u32x4v*>(lds);
#pragma unroll
    for (uint32_t i = 0; i < kStaged4 / kSweepBlock; ++i) dst[i * kSweepBlock + tid] = src[i * kSweepBlock + tid];
  }

  f32x16 c = {};
#pragma unroll
  for (int s = 0; s < st::kSweepSteps; ++s) {
    bf16x8 a, b;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      a[j] = static_cast<__bf16>(static_cast<float>(st::sweep_a(s, r, 8 * h + j)));
      b[j] = static_cast<__bf16>(static_cast<float>(st::sweep_b(s, 8 * h + j, r)));
    }
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
  bool mfma_bad = false;
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    uint32_t got = __float_as_uint(c[reg]);
    if (mine && inj.kind == kInjectMfma && tid == 0 && reg == 0) got ^= 1u;
    const int row = (reg & 3) + 8 * (reg >> 2) + 4 * h;
    mfma_bad |= got != __float_as_uint(expected[row * 32 + r]);
  }
  uint32_t path_bad = 0;
  if constexpr (kPaths) {
    static_assert(kStaged4 % kSweepBlock == 0, "the staging loop has no tail");
    __syncthreads();   // the tiles are in LDS
    const int inject_path = mine && inj.kind == kInjectPath && tid == 0 ? inj.path : -1;
    path_bad = paths_checked(AllPaths{}, paths, lane, lds, inject_path);
    __syncthreads();   // every wave has compared before the pattern test overwrites the tiles
  }

  volatile uint32_t* v = lds;
  uint32_t bad = st::kNoBadOffset;
  for (uint32_t pass = 0; pass < 2; ++pass) {
    const uint32_t flip = pass ? ~0u : 0u;
    for (uint32_t i = tid; i < n; i += kSweepBlock) v[i] = st::mix32(i ^ seed) ^ flip;
    __syncthreads();
    if (pass == 0 && mine && inj.kind == kInjectLds && tid == 0 && inj.lds_off < n) v[inj.lds_off] ^= 1u;
    __syncthreads();
    for (uint32_t j = tid; j < n; j += kSweepBlock) {
      const uint32_t i = n - 1 - j;
      if (v[i] != (st::mix32(i ^ seed) ^ flip) && i < bad) bad = i;
    }
    __syncthreads();
  }

  // the array has served; its first dwords carry the workgroup's reduction
  if (tid == 0) {
    lds[0] = 0;
    lds[1] = 0;
    lds[2] = st::kNoBadOffset;
    if constexpr (kPaths) {
      lds[3] = 0;
      lds[4] = 0;
    }
  }
  __syncthreads();
  if (mfma_bad) atomicOr(&lds[0], 1u << wave);
  if (path_bad) {
    atomicOr(&lds[3], path_bad);
    atomicOr(&lds[4], 1u << wave);
  }
  if (bad != st::kNoBadOffset) {
    atomicOr(&lds[0], st::kFailLds);
    atomicMin(&lds[2], bad);
  }
  if (lane == 0) atomicOr(&lds[1], 1u << st::hw_simd(hwid));
  __syncthreads();
  if (tid == 0) {
    uint32_t* o = out + static_cast<size_t>(blockIdx.x) * (kPaths ? sp::kPathRecordWords : st::kSweepRecordWords);
    o[0] = xcc;
    o[1] = hwid;
    o[2] = lds[0];
    o[3] = lds[1];
    o[4] = lds[2];
    if constexpr (kPaths) {
      o[5] = lds[3];
      o[6] = lds[4];
    }
  }
}

// kFull: the block holds all 160 KiB, so at most one sweep workgroup is resident per CU and a
// grid of rounds x CUs workgroups is spread over every enabled CU by the dispatcher. Otherwise
// (a runtime that does not let one block hold a whole CU's LDS, or the lds_bytes test hook) `n`
// dwords of dynamic LDS, sized by the host. The plain instantiations ignore `paths` and `tiles`.
// Both arrays are 16-byte aligned for the staging loop.
template <bool kPaths, bool kFull>
__global__ __launch_bounds__(kSweepBlock) void cu_sweep_kernel(const float* __restrict__ expected,
                                                               uint32_t* __restrict__ out, uint32_t seed,
                                                               SweepInject inj, uint32_t n, uint32_t paths,
                                                               const uint32_t* __restrict__ tiles) {
  if constexpr (kFull) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[kLdsDwordsFull];
    sweep_body<kPaths>(lds, kLdsDwordsFull, expected, out, seed, inj, paths, tiles);
  } else {
    extern __shared__ __attribute__((aligned(16))) uint32_t lds_dyn[];
    sweep_body<kPaths>(lds_dyn, n, expected, out, seed, inj, paths, tiles);
  }
}

// ---- vector ALU, transcendentals, register file (selftest_valu_host.h) ----
namespace sv = nanogpu::selftest::valu;

using f16x2 = __attribute__((ext_vector_type(2))) _Float16;
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;
using f32x2 = __attribute__((ext_vector_type(2))) float;

// The chains' operations as gfx950 instructions (the header names them). Nothing here may be
// contracted or reassociated: every function is one rounding.
struct DevOps {
  __device__ __forceinline__ uint32_t fma32(uint32_t a, uint32_t x, uint32_t b) {
    return __float_as_uint(__builtin_fmaf(__uint_as_float(a), __uint_as_float(x), __uint_as_float(b)));
  }
  __device__ __forceinline__ uint64_t fma64(uint64_t a, uint64_t x, uint64_t b) {
    return static_cast<uint64_t>(__double_as_longlong(__builtin_fma(__longlong_as_double(static_cast<long long>(a)),
                                                                    __longlong_as_double(static_cast<long long>(x)),
                                                                    __longlong_as_double(static_cast<long long>(b)))));
  }
  __device__ __forceinline__ uint32_t pkfma16(uint32_t a, uint32_t x, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_fma(__builtin_bit_cast(f16x2, a), __builtin_bit_cast(f16x2, x),
                                                                  __builtin_bit_cast(f16x2, b)));
  }
  __device__ __forceinline__ void pkfma32(uint32_t a0, uint32_t a1, uint32_t& x0, uint32_t& x1, uint32_t b0, uint32_t b1) {
    const f32x2 a = {__uint_as_float(a0), __uint_as_float(a1)}, x = {__uint_as_float(x0), __uint_as_float(x1)},
                b = {__uint_as_float(b0), __uint_as_float(b1)};
    const f32x2 r = __builtin_elementwise_fma(a, x, b);
    x0 = __float_as_uint(r[0]);
    x1 = __float_as_uint(r[1]);
  }
  __device__ __forceinline__ uint32_t mul32(uint32_t a, uint32_t b) {
#pragma clang fp contract(off)
    return __float_as_uint(__uint_as_float(a) * __uint_as_float(b));
  }
  __device__ __forceinline__ uint32_t add32(uint32_t a, uint32_t b) {
#pragma clang fp contract(off)
    return __float_as_uint(__uint_as_float(a) + __uint_as_float(b));
  }
  __device__ __forceinline__ uint32_t mulhi(uint32_t a, uint32_t b) { return __umulhi(a, b); }
  __device__ __forceinline__ uint64_t add64(uint64_t a, uint64_t b) { return a + b; }
  __device__ __forceinline__ uint64_t sub64(uint64_t a, uint64_t b) { return a - b; }
  __device__ __forceinline__ uint64_t asr64(uint64_t x, uint32_t n) {
    return static_cast<uint64_t>(static_cast<long long>(x) >> n);
  }
  __device__ __forceinline__ uint32_t perm(uint32_t s0, uint32_t s1, uint32_t sel) { return __builtin_amdgcn_perm(s0, s1, sel); }
  __device__ __forceinline__ uint32_t bfe_u(uint32_t v, uint32_t off, uint32_t width) { return __builtin_amdgcn_ubfe(v, off, width); }
  __device__ __forceinline__ uint32_t bfe_i(uint32_t v, uint32_t off, uint32_t width) {
    return static_cast<uint32_t>(__builtin_amdgcn_sbfe(static_cast<int>(v), off, width));
  }
  __device__ __forceinline__ uint32_t alignbit(uint32_t hi, uint32_t lo, uint32_t sh) { return __builtin_amdgcn_alignbit(hi, lo, sh); }
  __device__ __forceinline__ uint32_t bcnt(uint32_t v, uint32_t add) { return static_cast<uint32_t>(__builtin_popcount(v)) + add; }
  __device__ __forceinline__ uint32_t ffbl(uint32_t v) { return static_cast<uint32_t>(__builtin_ctz(v)); }
  __device__ __forceinline__ uint32_t ffbh(uint32_t v) { return static_cast<uint32_t>(__builtin_clz(v)); }
  __device__ __forceinline__ uint32_t udot4(uint32_t a, uint32_t b, uint32_t acc) { return __builtin_amdgcn_udot4(a, b, acc, false); }
  __device__ __forceinline__ uint32_t sdot4(uint32_t a, uint32_t b, uint32_t acc) {
    return static_cast<uint32_t>(__builtin_amdgcn_sdot4(static_cast<int>(a), static_cast<int>(b), static_cast<int>(acc), false));
  }
  __device__ __forceinline__ uint32_t pk_bf16(uint32_t a, uint32_t b) {
    const f32x2 v = {__uint_as_float(a), __uint_as_float(b)};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2));
  }
  __device__ __forceinline__ uint32_t f16(uint32_t a) {
    return __builtin_bit_cast(uint16_t, static_cast<_Float16>(__uint_as_float(a)));
  }
  __device__ __forceinline__ uint32_t pk_fp8(uint32_t a, uint32_t b) {
    return static_cast<uint32_t>(__builtin_amdgcn_cvt_pk_fp8_f32(__uint_as_float(a), __uint_as_float(b), 0, false)) & 0xffffu;
  }
  __device__ __forceinline__ uint32_t pk_bf8(uint32_t a, uint32_t b) {
    return static_cast<uint32_t>(__builtin_amdgcn_cvt_pk_bf8_f32(__uint_as_float(a), __uint_as_float(b), 0, false)) & 0xffffu;
  }
  __device__ __forceinline__ uint32_t f2i(uint32_t x) { return static_cast<uint32_t>(static_cast<int>(__uint_as_float(x))); }
  __device__ __forceinline__ uint32_t i2f(uint32_t i) { return __float_as_uint(static_cast<float>(static_cast<int>(i))); }
};

// One step of the cross-lane group: the row rotation and the read lane are immediates. Every
// lane of the wave is active (the callers branch only wave-uniformly).
template <int S>
__device__ __forceinline__ uint32_t xlane_step(uint32_t x, int lane, int c) {
  const uint32_t d = static_cast<uint32_t>(
      __builtin_amdgcn_update_dpp(0, static_cast<int>(x), 0x120 + sv::xlane_ror(S), 0xf, 0xf, false));
  const uint32_t b = static_cast<uint32_t>(__shfl_xor(static_cast<int>(x), 32));
  const uint32_t r = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(x), sv::xlane_readlane(S)));
  return sv::xlane_combine(d, b, r, sv::valu_operand(sv::kXlane, S, lane, 4 * c));
}

__device__ __forceinline__ void chain_xlane(int lane, uint32_t* out) {
  static_assert(sv::kValuSteps == 8, "the chain is unrolled by hand: the DPP control is an immediate");
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    uint32_t x = sv::valu_operand(sv::kXlane, 0, lane, 1 + 4 * c);
    x = xlane_step<0>(x, lane, c);
    x = xlane_step<1>(x, lane, c);
    x = xlane_step<2>(x, lane, c);
    x = xlane_step<3>(x, lane, c);
    x = xlane_step<4>(x, lane, c);
    x = xlane_step<5>(x, lane, c);
    x = xlane_step<6>(x, lane, c);
    x = xlane_step<7>(x, lane, c);
    out[c] = x;
  }
}

template <int G>
__device__ __forceinline__ void valu_chain(int lane, uint32_t* w) {
  DevOps o;
  if constexpr (G == sv::kFma32) sv::chain_fma32(o, lane, w);
  else if constexpr (G == sv::kFma64) sv::chain_fma64(o, lane, w);
  else if constexpr (G == sv::kPkFma16) sv::chain_pkfma16(o, lane, w);
  else if constexpr (G == sv::kPkFma32) sv::chain_pkfma32(o, lane, w);
  else if constexpr (G == sv::kAddMul32) sv::chain_addmul32(o, lane, w);
  else if constexpr (G == sv::kInt32) sv::chain_int32(o, lane, w);
  else if constexpr (G == sv::kInt64) sv::chain_int64(o, lane, w);
  else if constexpr (G == sv::kBits) sv::chain_bits(o, lane, w);
  else if constexpr (G == sv::kDot) sv::chain_dot(o, lane, w);
  else if constexpr (G == sv::kCvt) sv::chain_cvt(o, lane, w);
  else chain_xlane(lane, w);
}

__device__ __forceinline__ void approx_outputs(int lane, uint32_t out[sv::kNumApprox]) {
  out[sv::kExp2] = __float_as_uint(__builtin_amdgcn_exp2f(__uint_as_float(sv::approx_input(sv::kExp2, lane))));
  out[sv::kLog2] = __float_as_uint(__builtin_amdgcn_logf(__uint_as_float(sv::approx_input(sv::kLog2, lane))));
  out[sv::kRcp] = __float_as_uint(__builtin_amdgcn_rcpf(__uint_as_float(sv::approx_input(sv::kRcp, lane))));
  out[sv::kRsq] = __float_as_uint(__builtin_amdgcn_rsqf(__uint_as_float(sv::approx_input(sv::kRsq, lane))));
  out[sv::kSqrt] = __float_as_uint(__builtin_amdgcn_sqrtf(__uint_as_float(sv::approx_input(sv::kSqrt, lane))));
}

using ExactGroups = std::make_integer_sequence<int, sv::kNumExact>;

// Bit G is set when selected group G's two words differed from the table on this lane.
template <int G>
__device__ __forceinline__ uint32_t group_checked(uint32_t groups, int lane, const uint32_t* __restrict__ table, int inject) {
  if (!(groups >> G & 1u)) return 0u;   // wave-uniform
  uint32_t w[sv::kLaneWords];
  valu_chain<G>(lane, w);
  if (inject == G) w[0] ^= 1u;
  const uint32_t* e = table + G * sv::kGroupWords + lane * sv::kLaneWords;
  return (w[0] != e[0] || w[1] != e[1]) ? 1u << G : 0u;
}

template <int... G>
__device__ __forceinline__ uint32_t groups_checked(std::integer_sequence<int, G...>, uint32_t groups, int lane,
                                                   const uint32_t* __restrict__ table, int inject) {
  uint32_t bad = 0;
  ((bad |= group_checked<G>(groups, lane, table, inject)), ...);
  return bad;
}

enum : int { kValuInjectNone = 0, kValuInjectGroup = 1, kValuInjectRegs = 2, kValuInjectApprox = 3 };

// Test hook: on CU (xcc, cu_key), lane 0 of wave 0 flips one bit of data it owns: of group
// `arg`'s result, of one approx output, or, for the register file, of the expected value slot
// `arg` is compared with in pass 0 (not of the held register itself: see regfile_test).
struct ValuInject {
  int xcc = -1, cu_key = -1, kind = kValuInjectNone, arg = -1;
};

// Pattern test of the vector register file: every lane writes sv::kRegSlots values that depend on
// slot, lane and wave, holds them all at once, and compares them in place; the second pass holds
// the complement. What makes "all at once" certain: every slot passes through an empty volatile
// asm statement (so it is in a register and cannot be folded), and the comparison's expected
// values derive from `key`, which passes through a volatile asm statement after the last slot's:
// volatile asm statements keep their order, so no slot can be compared, and die, before every
// slot is held. For the same reason the expected values cannot be the written ones kept alive,
// and the pass loop is a real loop, so pass 1 cannot be computed from pass 0's values. A "v"
// operand is an architectural VGPR: what the 256 of them cannot hold waits in the accumulator
// half of the SIMD's unified file. The host refuses this part when the code object reports
// scratch. `inject_slot` (test hook, wave-uniform; -1: none) flips bit 0 in thread 0's
// comparison of that slot in pass 0: folded into the expected value, because a write to the held
// array costs the registers this test is there to fill.
// Returns flags: bit j of flag f is slot 32 f + j differing in either pass.
__device__ __forceinline__ void regfile_test(uint32_t tid, uint32_t seed, int inject_slot, uint32_t (&flags)[sv::kRegFlags]) {
  uint32_t r[sv::kRegSlots];
#pragma unroll
  for (int f = 0; f < sv::kRegFlags; ++f) flags[f] = 0;
#pragma nounroll
  for (uint32_t pass = 0; pass < 2; ++pass) {
    asm volatile("" : "+s"(seed));
#pragma unroll
    for (int i = 0; i < sv::kRegSlots; ++i) {
      r[i] = sv::reg_word(i, tid, seed, pass);
      asm volatile("" : "+v"(r[i]));
    }
    uint32_t key = tid ^ seed;          // reg_word(i, tid, seed, pass) == mix32(i << 8 ^ key), complemented in pass 1
    int inj = inject_slot;
    uint32_t flipv = (tid == 0 && pass == 0) ? 1u : 0u;
    asm volatile("" : "+v"(key), "+s"(inj), "+v"(flipv));
#pragma unroll
    for (int i = 0; i < sv::kRegSlots; ++i) {
      const uint32_t v = st::mix32((static_cast<uint32_t>(i) << 8) ^ key) ^ (inj == i ? flipv : 0u);
      flags[i / sv::kRegFlagSlots] |= r[i] != (pass ? ~v : v) ? 1u << (i % sv::kRegFlagSlots) : 0u;
    }
  }
}

constexpr int kValuLdsTable = sv::kTableWords + sv::kApproxWords;   // staged: the table, then the approx ranges

// One visit of one CU, on the grid and the stream of cu_sweep_kernel: all four waves (one per
// SIMD: a wave holding sv::kRegSlots registers is alone on its SIMD, so the block is alone on
// its CU) run every selected exact group against the host's table, the transcendentals against
// the host's ranges, and last, with only verdict bits live, the register-file test. One record
// per workgroup. No spin, no inter-workgroup traffic, every loop bounded by a constant.
__global__ __launch_bounds__(kSweepBlock) __attribute__((amdgpu_waves_per_eu(1, 1)))
void cu_valu_kernel(const uint32_t* __restrict__ table, uint32_t* __restrict__ out, uint32_t seed, ValuInject inj,
                    uint32_t groups) {
  __shared__ __attribute__((aligned(16))) uint32_t staged[kValuLdsTable];
  __shared__ uint32_t red[12];   // 0 fail, 1 simds, 2 groups, 3 first bad (slot << 8 | thread), 4..7 approx hash of wave w
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint32_t xcc, hwid;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
  const bool mine = inj.kind != kValuInjectNone && xcc == static_cast<uint32_t>(inj.xcc) &&
                    st::hw_cu_key(hwid) == static_cast<uint32_t>(inj.cu_key) && tid == 0;
  static_assert(kValuLdsTable % kSweepBlock == 0, "the staging loop has no tail");
#pragma unroll
  for (int i = 0; i < kValuLdsTable / kSweepBlock; ++i) staged[i * kSweepBlock + tid] = table[i * kSweepBlock + tid];
  if (tid < 12) red[tid] = tid == 3 ? sv::kNoBad : 0u;
  __syncthreads();

  const uint32_t group_bad =
      groups_checked(ExactGroups{}, groups, static_cast<int>(lane), staged, mine && inj.kind == kValuInjectGroup ? inj.arg : -1);
  bool bound_bad = false;
  if (groups >> sv::kApprox & 1u) {   // wave-uniform
    uint32_t a[sv::kNumApprox];
    approx_outputs(static_cast<int>(lane), a);
    if (mine && inj.kind == kValuInjectApprox) a[sv::kRcp] ^= 1u;
    const uint32_t* range = staged + sv::kTableWords;
#pragma unroll
    for (int op = 0; op < sv::kNumApprox; ++op) {
      const uint32_t key = sv::ordered_key(a[op]);
      bound_bad |= key < range[(op * sv::kLanes + lane) * 2] || key > range[(op * sv::kLanes + lane) * 2 + 1];
    }
    atomicAdd(&red[4 + wave], sv::approx_lane_hash(a, static_cast<int>(lane)));
  }
  if (group_bad) {
    atomicOr(&red[0], 1u << (sv::kFailExactShift + wave));
    atomicOr(&red[2], group_bad);
  }
  if (bound_bad) atomicOr(&red[0], 1u << (sv::kFailBoundShift + wave));
  if (lane == 0) atomicOr(&red[1], 1u << st::hw_simd(hwid));

  if (groups >> sv::kRegs & 1u) {     // wave-uniform; last: nothing but verdicts is live across it
    uint32_t flags[sv::kRegFlags];
    const bool here = inj.kind == kValuInjectRegs && xcc == static_cast<uint32_t>(inj.xcc) &&
                      st::hw_cu_key(hwid) == static_cast<uint32_t>(inj.cu_key) && wave == 0;   // wave-uniform
    regfile_test(tid, seed, __builtin_amdgcn_readfirstlane(here ? inj.arg : -1), flags);
    uint32_t any = 0;
#pragma unroll
    for (int f = 0; f < sv::kRegFlags; ++f) any |= flags[f];
    if (any) {                        // the failing path resolves slot and lane
      uint32_t slot = 0;
#pragma unroll
      for (int f = sv::kRegFlags - 1; f >= 0; --f)
        if (flags[f]) slot = f * sv::kRegFlagSlots + static_cast<uint32_t>(__builtin_ctz(flags[f]));
      atomicOr(&red[0], 1u << (sv::kFailRegsShift + wave));
      atomicMin(&red[3], slot << 8 | tid);
    }
  }
  __syncthreads();
  if (tid == 0) {
    uint32_t fail = red[0];
    for (uint32_t w = 1; w < 4; ++w)
      if (red[4 + w] != red[4]) fail |= 1u << (sv::kFailHashShift + w);
    uint32_t* o = out + static_cast<size_t>(blockIdx.x) * sv::kValuRecordWords;
    o[0] = xcc;
    o[1] = hwid;
    o[2] = fail;
    o[3] = red[1];
    o[4] = red[2];
    o[5] = red[3] == sv::kNoBad ? sv::kNoBad : red[3] >> 8;
    o[6] = red[3] == sv::kNoBad ? sv::kNoBad : red[3] & 0xffu;
    o[7] = red[4];
  }
}

// One wave, one group: the raw per-lane words (exact groups: [lane][2]; approx: [op][lane]). It
// establishes on the device that the kernel's instruction sequence is the twin's arithmetic.
template <int G>
__global__ __launch_bounds__(64) void valu_lanes_kernel(uint32_t* __restrict__ out) {
  const int lane = threadIdx.x;
  if constexpr (G == sv::kApprox) {
    uint32_t a[sv::kNumApprox];
    approx_outputs(lane, a);
#pragma unroll
    for (int op = 0; op < sv::kNumApprox; ++op) out[op * sv::kLanes + lane] = a[op];
  } else {
    uint32_t w[sv::kLaneWords];
    valu_chain<G>(lane, w);
    out[lane * sv::kLaneWords] = w[0];
    out[lane * sv::kLaneWords + 1] = w[1];
  }
}

// ---- scalar ALU, scalar loads, SGPR file (selftest_scalar_host.h) ----
namespace ss = nanogpu::selftest::scalar;

using u32x2v = __attribute__((ext_vector_type(2))) uint32_t;
using u32x8v = __attribute__((ext_vector_type(8))) uint32_t;
using u32x16v = __attribute__((ext_vector_type(16))) uint32_t;

// The chains' operations as gfx950 instructions: one asm statement each, so that the instruction the
// header names is the one that runs. An SCC producer shares its statement with the s_cselect_b32
// that reads SCC (SCC does not survive between statements); every operand is an SGPR.
#define NANOGPU_S2_SCC(name, T, insn)                                                                              \
  __device__ __forceinline__ T name(T a, T b, uint32_t& c) {                                                       \
    T d;                                                                                                           \
    asm volatile(insn " %0, %2, %3\n\ts_cselect_b32 %1, 1, 0" : "=&s"(d), "=&s"(c) : "s"(a), "s"(b) : "scc");      \
    return d;                                                                                                      \
  }
#define NANOGPU_SH_SCC(name, T, insn)                                                                              \
  __device__ __forceinline__ T name(T a, uint32_t n, uint32_t& c) {                                                \
    T d;                                                                                                           \
    n = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(n))); /* a count from a division */   \
    asm volatile(insn " %0, %2, %3\n\ts_cselect_b32 %1, 1, 0" : "=&s"(d), "=&s"(c) : "s"(a), "s"(n) : "scc");      \
    return d;                                                                                                      \
  }
#define NANOGPU_S1_SCC(name, D, T, insn)                                                                           \
  __device__ __forceinline__ D name(T a, uint32_t& c) {                                                            \
    D d;                                                                                                           \
    asm volatile(insn " %0, %2\n\ts_cselect_b32 %1, 1, 0" : "=&s"(d), "=&s"(c) : "s"(a) : "scc");                  \
    return d;                                                                                                      \
  }
#define NANOGPU_S2(name, D, T, insn)                                          \
  __device__ __forceinline__ D name(T a, T b) {                               \
    D d;                                                                      \
    asm volatile(insn " %0, %1, %2" : "=s"(d) : "s"(a), "s"(b) : "scc");      \
    return d;                                                                 \
  }
#define NANOGPU_S1(name, D, T, insn)                                \
  __device__ __forceinline__ D name(T a) {                          \
    D d;                                                            \
    asm volatile(insn " %0, %1" : "=s"(d) : "s"(a) : "scc");        \
    return d;                                                       \
  }
// A compare consumed by a select: SCC ? x : y through s_cselect_b32, through s_cselect_b64 (the pairs
// ~x:x and ~y:y; a wrong high half changes the word) or through s_cmov_b32 onto y.
#define NANOGPU_SEL32(name, insn)                                                                                        \
  template <class T>                                                                                                     \
  __device__ __forceinline__ uint32_t sel_##name(T a, T b, uint32_t x, uint32_t y) {                                     \
    uint32_t d;                                                                                                          \
    asm volatile(insn " %1, %2\n\ts_cselect_b32 %0, %3, %4" : "=&s"(d) : "s"(a), "s"(b), "s"(x), "s"(y) : "scc");        \
    return d;                                                                                                            \
  }
#define NANOGPU_SEL64(name, insn)                                                                                        \
  template <class T>                                                                                                     \
  __device__ __forceinline__ uint32_t sel_##name(T a, T b, uint32_t x, uint32_t y) {                                     \
    uint64_t d;                                                                                                          \
    const uint64_t xx = ss::pair64(~x, x), yy = ss::pair64(~y, y);                                                       \
    asm volatile(insn " %1, %2\n\ts_cselect_b64 %0, %3, %4" : "=&s"(d) : "s"(a), "s"(b), "s"(xx), "s"(yy) : "scc");      \
    return static_cast<uint32_t>(d) + (static_cast<uint32_t>(d >> 32) ^ ~static_cast<uint32_t>(d));                      \
  }
#define NANOGPU_SELMOV(name, insn)                                                                    \
  template <class T>                                                                                  \
  __device__ __forceinline__ uint32_t sel_##name(T a, T b, uint32_t x, uint32_t y) {                  \
    uint32_t d = y;                                                                                   \
    asm volatile(insn " %1, %2\n\ts_cmov_b32 %0, %3" : "+&s"(d) : "s"(a), "s"(b), "s"(x) : "scc");    \
    return d;                                                                                         \
  }
// A compare consumed by a branch that skips forward over one s_mov_b32: SCC ? x : y again.
#define NANOGPU_BR1(name, insn)                                                                                         \
  template <class T>                                                                                                    \
  __device__ __forceinline__ uint32_t br_##name(T a, T b, uint32_t x, uint32_t y) {                                     \
    uint32_t d = x;                                                                                                     \
    asm volatile(insn " %1, %2\n\ts_cbranch_scc1 .Lnanogpu_br%=\n\ts_mov_b32 %0, %3\n.Lnanogpu_br%=:"                   \
                 : "+&s"(d) : "s"(a), "s"(b), "s"(y) : "scc");                                                          \
    return d;                                                                                                           \
  }
#define NANOGPU_BR0(name, insn)                                                                                         \
  template <class T>                                                                                                    \
  __device__ __forceinline__ uint32_t br_##name(T a, T b, uint32_t x, uint32_t y) {                                     \
    uint32_t d = y;                                                                                                     \
    asm volatile(insn " %1, %2\n\ts_cbranch_scc0 .Lnanogpu_br%=\n\ts_mov_b32 %0, %3\n.Lnanogpu_br%=:"                   \
                 : "+&s"(d) : "s"(a), "s"(b), "s"(x) : "scc");                                                          \
    return d;                                                                                                           \
  }

struct DevScalarOps {
  NANOGPU_S2_SCC(add_u32, uint32_t, "s_add_u32")
  NANOGPU_S2_SCC(sub_u32, uint32_t, "s_sub_u32")
  NANOGPU_S2_SCC(add_i32, uint32_t, "s_add_i32")
  NANOGPU_S2_SCC(sub_i32, uint32_t, "s_sub_i32")
  NANOGPU_S2_SCC(min_i32, uint32_t, "s_min_i32")
  NANOGPU_S2_SCC(max_i32, uint32_t, "s_max_i32")
  NANOGPU_S2_SCC(min_u32, uint32_t, "s_min_u32")
  NANOGPU_S2_SCC(max_u32, uint32_t, "s_max_u32")
  NANOGPU_S2_SCC(absdiff_i32, uint32_t, "s_absdiff_i32")
  NANOGPU_S1_SCC(abs_i32, uint32_t, uint32_t, "s_abs_i32")
  __device__ __forceinline__ uint64_t add64(uint64_t a, uint64_t b, uint32_t& c) {
    uint32_t lo, hi;
    asm volatile("s_add_u32 %0, %3, %5\n\ts_addc_u32 %1, %4, %6\n\ts_cselect_b32 %2, 1, 0"
                 : "=&s"(lo), "=&s"(hi), "=&s"(c)
                 : "s"(static_cast<uint32_t>(a)), "s"(static_cast<uint32_t>(a >> 32)), "s"(static_cast<uint32_t>(b)),
                   "s"(static_cast<uint32_t>(b >> 32))
                 : "scc");
    return ss::pair64(hi, lo);
  }
  __device__ __forceinline__ uint64_t sub64(uint64_t a, uint64_t b, uint32_t& c) {
    uint32_t lo, hi;
    asm volatile("s_sub_u32 %0, %3, %5\n\ts_subb_u32 %1, %4, %6\n\ts_cselect_b32 %2, 1, 0"
                 : "=&s"(lo), "=&s"(hi), "=&s"(c)
                 : "s"(static_cast<uint32_t>(a)), "s"(static_cast<uint32_t>(a >> 32)), "s"(static_cast<uint32_t>(b)),
                   "s"(static_cast<uint32_t>(b >> 32))
                 : "scc");
    return ss::pair64(hi, lo);
  }

  NANOGPU_S2(mul_i32, uint32_t, uint32_t, "s_mul_i32")
  NANOGPU_S2(mul_hi_u32, uint32_t, uint32_t, "s_mul_hi_u32")
  NANOGPU_S2(mul_hi_i32, uint32_t, uint32_t, "s_mul_hi_i32")
  NANOGPU_S2_SCC(lshl1_add_u32, uint32_t, "s_lshl1_add_u32")
  NANOGPU_S2_SCC(lshl2_add_u32, uint32_t, "s_lshl2_add_u32")
  NANOGPU_S2_SCC(lshl3_add_u32, uint32_t, "s_lshl3_add_u32")
  NANOGPU_S2_SCC(lshl4_add_u32, uint32_t, "s_lshl4_add_u32")

  NANOGPU_SH_SCC(lshl_b32, uint32_t, "s_lshl_b32")
  NANOGPU_SH_SCC(lshr_b32, uint32_t, "s_lshr_b32")
  NANOGPU_SH_SCC(ashr_i32, uint32_t, "s_ashr_i32")
  NANOGPU_SH_SCC(lshl_b64, uint64_t, "s_lshl_b64")
  NANOGPU_SH_SCC(lshr_b64, uint64_t, "s_lshr_b64")
  NANOGPU_SH_SCC(ashr_i64, uint64_t, "s_ashr_i64")
  NANOGPU_S2(bfm_b32, uint32_t, uint32_t, "s_bfm_b32")
  NANOGPU_S2(bfm_b64, uint64_t, uint32_t, "s_bfm_b64")

  NANOGPU_S2_SCC(and_b32, uint32_t, "s_and_b32")
  NANOGPU_S2_SCC(or_b32, uint32_t, "s_or_b32")
  NANOGPU_S2_SCC(xor_b32, uint32_t, "s_xor_b32")
  NANOGPU_S2_SCC(nand_b32, uint32_t, "s_nand_b32")
  NANOGPU_S2_SCC(nor_b32, uint32_t, "s_nor_b32")
  NANOGPU_S2_SCC(xnor_b32, uint32_t, "s_xnor_b32")
  NANOGPU_S2_SCC(andn2_b32, uint32_t, "s_andn2_b32")
  NANOGPU_S2_SCC(orn2_b32, uint32_t, "s_orn2_b32")
  NANOGPU_S1_SCC(not_b32, uint32_t, uint32_t, "s_not_b32")
  NANOGPU_S2_SCC(and_b64, uint64_t, "s_and_b64")
  NANOGPU_S2_SCC(or_b64, uint64_t, "s_or_b64")
  NANOGPU_S2_SCC(xor_b64, uint64_t, "s_xor_b64")
  NANOGPU_S2_SCC(nand_b64, uint64_t, "s_nand_b64")
  NANOGPU_S2_SCC(nor_b64, uint64_t, "s_nor_b64")
  NANOGPU_S2_SCC(xnor_b64, uint64_t, "s_xnor_b64")
  NANOGPU_S2_SCC(andn2_b64, uint64_t, "s_andn2_b64")
  NANOGPU_S2_SCC(orn2_b64, uint64_t, "s_orn2_b64")
  NANOGPU_S1_SCC(not_b64, uint64_t, uint64_t, "s_not_b64")

  NANOGPU_SH_SCC(bfe_u32, uint32_t, "s_bfe_u32")
  NANOGPU_SH_SCC(bfe_i32, uint32_t, "s_bfe_i32")
  NANOGPU_SH_SCC(bfe_u64, uint64_t, "s_bfe_u64")
  NANOGPU_SH_SCC(bfe_i64, uint64_t, "s_bfe_i64")
  NANOGPU_S1(brev_b32, uint32_t, uint32_t, "s_brev_b32")
  NANOGPU_S1(brev_b64, uint64_t, uint64_t, "s_brev_b64")
  NANOGPU_S1_SCC(bcnt0_i32_b32, uint32_t, uint32_t, "s_bcnt0_i32_b32")
  NANOGPU_S1_SCC(bcnt1_i32_b32, uint32_t, uint32_t, "s_bcnt1_i32_b32")
  NANOGPU_S1_SCC(bcnt0_i32_b64, uint32_t, uint64_t, "s_bcnt0_i32_b64")
  NANOGPU_S1_SCC(bcnt1_i32_b64, uint32_t, uint64_t, "s_bcnt1_i32_b64")
  NANOGPU_S1(ff0_i32_b32, uint32_t, uint32_t, "s_ff0_i32_b32")
  NANOGPU_S1(ff1_i32_b32, uint32_t, uint32_t, "s_ff1_i32_b32")
  NANOGPU_S1(ff0_i32_b64, uint32_t, uint64_t, "s_ff0_i32_b64")
  NANOGPU_S1(ff1_i32_b64, uint32_t, uint64_t, "s_ff1_i32_b64")
  NANOGPU_S1(flbit_i32_b32, uint32_t, uint32_t, "s_flbit_i32_b32")
  NANOGPU_S1(flbit_i32_b64, uint32_t, uint64_t, "s_flbit_i32_b64")
  NANOGPU_S1(flbit_i32, uint32_t, uint32_t, "s_flbit_i32")
  NANOGPU_S1(flbit_i32_i64, uint32_t, uint64_t, "s_flbit_i32_i64")
  __device__ __forceinline__ uint32_t bitset0_b32(uint32_t d, uint32_t n) {
    asm volatile("s_bitset0_b32 %0, %1" : "+s"(d) : "s"(n) : "scc");
    return d;
  }
  __device__ __forceinline__ uint32_t bitset1_b32(uint32_t d, uint32_t n) {
    asm volatile("s_bitset1_b32 %0, %1" : "+s"(d) : "s"(n) : "scc");
    return d;
  }
  NANOGPU_S1(sext_i32_i8, uint32_t, uint32_t, "s_sext_i32_i8")
  NANOGPU_S1(sext_i32_i16, uint32_t, uint32_t, "s_sext_i32_i16")
  NANOGPU_S2(pack_ll_b32_b16, uint32_t, uint32_t, "s_pack_ll_b32_b16")
  NANOGPU_S2(pack_lh_b32_b16, uint32_t, uint32_t, "s_pack_lh_b32_b16")
  NANOGPU_S2(pack_hh_b32_b16, uint32_t, uint32_t, "s_pack_hh_b32_b16")

  // the select form rotates over the compares, the branch form alternates
  NANOGPU_SEL32(eq_i32, "s_cmp_eq_i32") NANOGPU_BR1(eq_i32, "s_cmp_eq_i32")
  NANOGPU_SEL64(lg_i32, "s_cmp_lg_i32") NANOGPU_BR0(lg_i32, "s_cmp_lg_i32")
  NANOGPU_SELMOV(gt_i32, "s_cmp_gt_i32") NANOGPU_BR1(gt_i32, "s_cmp_gt_i32")
  NANOGPU_SEL32(ge_i32, "s_cmp_ge_i32") NANOGPU_BR0(ge_i32, "s_cmp_ge_i32")
  NANOGPU_SEL64(lt_i32, "s_cmp_lt_i32") NANOGPU_BR1(lt_i32, "s_cmp_lt_i32")
  NANOGPU_SELMOV(le_i32, "s_cmp_le_i32") NANOGPU_BR0(le_i32, "s_cmp_le_i32")
  NANOGPU_SEL32(eq_u32, "s_cmp_eq_u32") NANOGPU_BR1(eq_u32, "s_cmp_eq_u32")
  NANOGPU_SEL64(lg_u32, "s_cmp_lg_u32") NANOGPU_BR0(lg_u32, "s_cmp_lg_u32")
  NANOGPU_SELMOV(gt_u32, "s_cmp_gt_u32") NANOGPU_BR1(gt_u32, "s_cmp_gt_u32")
  NANOGPU_SEL32(ge_u32, "s_cmp_ge_u32") NANOGPU_BR0(ge_u32, "s_cmp_ge_u32")
  NANOGPU_SEL64(lt_u32, "s_cmp_lt_u32") NANOGPU_BR1(lt_u32, "s_cmp_lt_u32")
  NANOGPU_SELMOV(le_u32, "s_cmp_le_u32") NANOGPU_BR0(le_u32, "s_cmp_le_u32")
  NANOGPU_SEL32(bitcmp0_b32, "s_bitcmp0_b32") NANOGPU_BR1(bitcmp0_b32, "s_bitcmp0_b32")
  NANOGPU_SEL64(bitcmp1_b32, "s_bitcmp1_b32") NANOGPU_BR0(bitcmp1_b32, "s_bitcmp1_b32")
  NANOGPU_SELMOV(eq_u64, "s_cmp_eq_u64") NANOGPU_BR1(eq_u64, "s_cmp_eq_u64")
  NANOGPU_SEL32(lg_u64, "s_cmp_lg_u64") NANOGPU_BR0(lg_u64, "s_cmp_lg_u64")
};
#undef NANOGPU_S2_SCC
#undef NANOGPU_SH_SCC
#undef NANOGPU_S1_SCC
#undef NANOGPU_S2
#undef NANOGPU_S1
#undef NANOGPU_SEL32
#undef NANOGPU_SEL64
#undef NANOGPU_SELMOV
#undef NANOGPU_BR1
#undef NANOGPU_BR0

// The vcc group (the header states the step): builtins, so the compiler picks the encodings. Every
// lane of the wave is active; h and the operands are wave-uniform.
template <class Out>
__device__ __forceinline__ void chain_vcc(int wave, int lane, Out&& out) {
  uint32_t h = ss::scalar_operand(ss::kVcc, 0, wave, 15);
  for (int s = 0; s < ss::kWaveWords; ++s) {
    const uint32_t u0 = ss::scalar_operand(ss::kVcc, s, wave, 0), thr = ss::scalar_operand(ss::kVcc, s, wave, 1);
    const uint32_t k = ss::scalar_operand(ss::kVcc, s, wave, 4);
    const uint64_t m = ss::pair64(ss::scalar_operand(ss::kVcc, s, wave, 3), ss::scalar_operand(ss::kVcc, s, wave, 2));
    const uint32_t v = ss::vcc_lane_value(u0, lane);
    const uint64_t mask = __ballot(v < thr);
    const uint32_t cnt = static_cast<uint32_t>(__popcll(mask));
    const uint32_t ff = static_cast<uint32_t>(__builtin_ctzll(mask | (uint64_t(1) << 63)));
    const uint32_t r = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(v ^ h)));
    const uint32_t w = __builtin_amdgcn_inverse_ballot_w64(m) ? v + k : v ^ k;
    const uint64_t mask2 = __ballot(w < k);
    h = ss::vcc_fold(h, mask, cnt, ff, r, mask2);
    out(s, h);
  }
}

template <int G, class Out>
__device__ __forceinline__ void scalar_chain(int wave, int lane, Out&& out) {
  DevScalarOps o;
  if constexpr (G == ss::kAdd) ss::chain_add(o, wave, out);
  else if constexpr (G == ss::kMul) ss::chain_mul(o, wave, out);
  else if constexpr (G == ss::kShift) ss::chain_shift(o, wave, out);
  else if constexpr (G == ss::kLogic) ss::chain_logic(o, wave, out);
  else if constexpr (G == ss::kBits) ss::chain_bits(o, wave, out);
  else if constexpr (G == ss::kCmp) ss::chain_cmp(o, wave, out);
  else chain_vcc(wave, lane, out);
}

using ScalarExact = std::make_integer_sequence<int, ss::kNumExact>;

// Bit G is set when one of selected group G's words differed from the table on this wave (uniform).
template <int G>
__device__ __forceinline__ uint32_t scalar_group_checked(uint32_t groups, int wave, int lane, const uint32_t* __restrict__ table,
                                                         int inject) {
  if (!(groups >> G & 1u)) return 0u;   // wave-uniform
  const uint32_t* e = table + G * ss::kGroupWords + wave * ss::kWaveWords;
  bool bad = false;
  scalar_chain<G>(wave, lane, [&](int s, uint32_t h) { bad |= (h ^ (inject == G && s == 0 ? 1u : 0u)) != e[s]; });
  return bad ? 1u << G : 0u;
}

template <int... G>
__device__ __forceinline__ uint32_t scalar_groups_checked(std::integer_sequence<int, G...>, uint32_t groups, int wave, int lane,
                                                          const uint32_t* __restrict__ table, int inject) {
  uint32_t bad = 0;
  ((bad |= scalar_group_checked<G>(groups, wave, lane, table, inject)), ...);
  return bad;
}

enum : int { kScalarInjectNone = 0, kScalarInjectGroup = 1, kScalarInjectSmem = 2, kScalarInjectSregs = 3 };

// Test hook: on CU (xcc, cu_key), bit 0 flips of group `arg`'s first result word on wave 0, of the
// value table word `arg` is compared with (on the wave that reads it), or of the value register slot
// `arg` is compared with in pass 0 on wave 0 (never of the held register).
struct ScalarInject {
  int xcc = -1, cu_key = -1, kind = kScalarInjectNone, arg = -1;
};

// N words the statement before loaded from table words first.., against smem_word of their indices.
// `inject` (-1: none) is the index whose expected value has bit 0 flipped. Returns the lowest bad index.
template <int N, class V>
__device__ __forceinline__ uint32_t smem_compare(const V& got, uint32_t first, uint32_t inject, uint32_t bad) {
#pragma unroll
  for (int j = 0; j < N; ++j) {
    uint32_t g;
    if constexpr (N == 1) g = got;
    else g = got[j];
    const uint32_t idx = first + j;
    if (g != (ss::smem_word(idx) ^ (idx == inject ? 1u : 0u)) && idx < bad) bad = idx;
  }
  return bad;
}

// Wave `wave` reads its quarter of the table through the scalar data cache, each load width its span
// (ss::kSmemSpan*): several loads, then one wait, in one statement. The offsets are immediates
// inside the quarter; every loop is bounded by a span. Returns the lowest bad word index, or kNoBad.
__device__ __forceinline__ uint32_t smem_test(const uint32_t* __restrict__ table, int wave, uint32_t inject) {
  uint32_t bad = ss::kNoBad;
  uint32_t at = static_cast<uint32_t>(wave) * ss::kSmemQuarter;
#pragma nounroll
  for (int i = 0; i < ss::kSmemSpanX16 / 32; ++i, at += 32) {
    u32x16v a, b;
    asm volatile("s_load_dwordx16 %0, %2, 0x0\n\ts_load_dwordx16 %1, %2, 0x40\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(a), "=&s"(b) : "s"(table + at) : "memory");
    bad = smem_compare<16>(a, at, inject, bad);
    bad = smem_compare<16>(b, at + 16, inject, bad);
  }
#pragma nounroll
  for (int i = 0; i < ss::kSmemSpanX8 / 16; ++i, at += 16) {
    u32x8v a, b;
    asm volatile("s_load_dwordx8 %0, %2, 0x0\n\ts_load_dwordx8 %1, %2, 0x20\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(a), "=&s"(b) : "s"(table + at) : "memory");
    bad = smem_compare<8>(a, at, inject, bad);
    bad = smem_compare<8>(b, at + 8, inject, bad);
  }
#pragma nounroll
  for (int i = 0; i < ss::kSmemSpanX4 / 16; ++i, at += 16) {
    u32x4v a, b, c, d;
    asm volatile("s_load_dwordx4 %0, %4, 0x0\n\ts_load_dwordx4 %1, %4, 0x10\n\ts_load_dwordx4 %2, %4, 0x20\n\t"
                 "s_load_dwordx4 %3, %4, 0x30\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(a), "=&s"(b), "=&s"(c), "=&s"(d) : "s"(table + at) : "memory");
    bad = smem_compare<4>(a, at, inject, bad);
    bad = smem_compare<4>(b, at + 4, inject, bad);
    bad = smem_compare<4>(c, at + 8, inject, bad);
    bad = smem_compare<4>(d, at + 12, inject, bad);
  }
#pragma nounroll
  for (int i = 0; i < ss::kSmemSpanX2 / 8; ++i, at += 8) {
    u32x2v a, b, c, d;
    asm volatile("s_load_dwordx2 %0, %4, 0x0\n\ts_load_dwordx2 %1, %4, 0x8\n\ts_load_dwordx2 %2, %4, 0x10\n\t"
                 "s_load_dwordx2 %3, %4, 0x18\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(a), "=&s"(b), "=&s"(c), "=&s"(d) : "s"(table + at) : "memory");
    bad = smem_compare<2>(a, at, inject, bad);
    bad = smem_compare<2>(b, at + 2, inject, bad);
    bad = smem_compare<2>(c, at + 4, inject, bad);
    bad = smem_compare<2>(d, at + 6, inject, bad);
  }
#pragma nounroll
  for (int i = 0; i < ss::kSmemSpanX1 / 4; ++i, at += 4) {
    uint32_t a, b, c, d;
    asm volatile("s_load_dword %0, %4, 0x0\n\ts_load_dword %1, %4, 0x4\n\ts_load_dword %2, %4, 0x8\n\t"
                 "s_load_dword %3, %4, 0xc\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(a), "=&s"(b), "=&s"(c), "=&s"(d) : "s"(table + at) : "memory");
    bad = smem_compare<1>(a, at, inject, bad);
    bad = smem_compare<1>(b, at + 1, inject, bad);
    bad = smem_compare<1>(c, at + 2, inject, bad);
    bad = smem_compare<1>(d, at + 3, inject, bad);
  }
  return bad;
}

// Pattern test of the wave's scalar registers. One asm statement names its registers, s12..s99
// (slot i is s(12 + i)), so the compiler allocates none of them and cannot move a slot to a VGPR
// lane: compiler-allocated slots behind "+s" constraints spill there silently. The statement runs
// twice, the second pass complemented. Per pass it first writes key * odd_i ^ c_i (^ cm: all ones in pass 1) into every slot, then
// recomputes each value in a scratch register from an opaque copy of the key and compares; a slot that differs
// sets bit i % 32 of flag word i / 32. `inj` (-1: none) is the slot whose recomputed value gets
// `flipv` XORed in: the held register is never touched. No backward branch: each slot's skip is a
// forward one over one instruction.
#define NANOGPU_SREG_W(R)                                                  \
  "s_mul_i32 s" #R ", %[key], 0x9e3779b1+2*(" #R "-12)\n\t"                \
  "s_xor_b32 s" #R ", s" #R ", 0x7f4a7c15+0x01000193*(" #R "-12)\n\t"      \
  "s_xor_b32 s" #R ", s" #R ", %[cm]\n\t"
#define NANOGPU_SREG_V(R, F)                                               \
  "s_mul_i32 %[t], %[key2], 0x9e3779b1+2*(" #R "-12)\n\t"                  \
  "s_xor_b32 %[t], %[t], 0x7f4a7c15+0x01000193*(" #R "-12)\n\t"            \
  "s_xor_b32 %[t], %[t], %[cm]\n\t"                                        \
  "s_cmp_lg_u32 %[inj], " #R "-12\n\t"                                     \
  "s_cbranch_scc1 .Lnanogpu_sreg" #R "_%=\n\t"                             \
  "s_xor_b32 %[t], %[t], %[flipv]\n"                                       \
  ".Lnanogpu_sreg" #R "_%=:\n\t"                                           \
  "s_cmp_lg_u32 %[t], s" #R "\n\t"                                         \
  "s_cselect_b32 %[t], 1<<((" #R "-12)&31), 0\n\t"                         \
  "s_or_b32 %[" F "], %[" F "], %[t]\n\t"
#define NANOGPU_SREG_ROW0(M, ...) M(12, ##__VA_ARGS__) M(13, ##__VA_ARGS__) M(14, ##__VA_ARGS__) M(15, ##__VA_ARGS__) \
  M(16, ##__VA_ARGS__) M(17, ##__VA_ARGS__) M(18, ##__VA_ARGS__) M(19, ##__VA_ARGS__) M(20, ##__VA_ARGS__) M(21, ##__VA_ARGS__) \
  M(22, ##__VA_ARGS__) M(23, ##__VA_ARGS__) M(24, ##__VA_ARGS__) M(25, ##__VA_ARGS__) M(26, ##__VA_ARGS__) M(27, ##__VA_ARGS__) \
  M(28, ##__VA_ARGS__) M(29, ##__VA_ARGS__) M(30, ##__VA_ARGS__) M(31, ##__VA_ARGS__) M(32, ##__VA_ARGS__) M(33, ##__VA_ARGS__) \
  M(34, ##__VA_ARGS__) M(35, ##__VA_ARGS__) M(36, ##__VA_ARGS__) M(37, ##__VA_ARGS__) M(38, ##__VA_ARGS__) M(39, ##__VA_ARGS__) \
  M(40, ##__VA_ARGS__) M(41, ##__VA_ARGS__) M(42, ##__VA_ARGS__) M(43, ##__VA_ARGS__)
#define NANOGPU_SREG_ROW1(M, ...) M(44, ##__VA_ARGS__) M(45, ##__VA_ARGS__) M(46, ##__VA_ARGS__) M(47, ##__VA_ARGS__) \
  M(48, ##__VA_ARGS__) M(49, ##__VA_ARGS__) M(50, ##__VA_ARGS__) M(51, ##__VA_ARGS__) M(52, ##__VA_ARGS__) M(53, ##__VA_ARGS__) \
  M(54, ##__VA_ARGS__) M(55, ##__VA_ARGS__) M(56, ##__VA_ARGS__) M(57, ##__VA_ARGS__) M(58, ##__VA_ARGS__) M(59, ##__VA_ARGS__) \
  M(60, ##__VA_ARGS__) M(61, ##__VA_ARGS__) M(62, ##__VA_ARGS__) M(63, ##__VA_ARGS__) M(64, ##__VA_ARGS__) M(65, ##__VA_ARGS__) \
  M(66, ##__VA_ARGS__) M(67, ##__VA_ARGS__) M(68, ##__VA_ARGS__) M(69, ##__VA_ARGS__) M(70, ##__VA_ARGS__) M(71, ##__VA_ARGS__) \
  M(72, ##__VA_ARGS__) M(73, ##__VA_ARGS__) M(74, ##__VA_ARGS__) M(75, ##__VA_ARGS__)
#define NANOGPU_SREG_ROW2(M, ...) M(76, ##__VA_ARGS__) M(77, ##__VA_ARGS__) M(78, ##__VA_ARGS__) M(79, ##__VA_ARGS__) \
  M(80, ##__VA_ARGS__) M(81, ##__VA_ARGS__) M(82, ##__VA_ARGS__) M(83, ##__VA_ARGS__) M(84, ##__VA_ARGS__) M(85, ##__VA_ARGS__) \
  M(86, ##__VA_ARGS__) M(87, ##__VA_ARGS__) M(88, ##__VA_ARGS__) M(89, ##__VA_ARGS__) M(90, ##__VA_ARGS__) M(91, ##__VA_ARGS__) \
  M(92, ##__VA_ARGS__) M(93, ##__VA_ARGS__) M(94, ##__VA_ARGS__) M(95, ##__VA_ARGS__) M(96, ##__VA_ARGS__) M(97, ##__VA_ARGS__) \
  M(98, ##__VA_ARGS__) M(99, ##__VA_ARGS__)
#define NANOGPU_SREG_NAME(R) "s" #R,
static_assert(ss::kSregFirst == 12 && ss::kSregSlots == 88 && ss::kSregFlags == 3, "the statement names s12..s99 and three flag words");

// One pass: `cm` is 0, or all ones for the complement.
__device__ __forceinline__ void sregs_pass(uint32_t key, uint32_t cm, uint32_t inj, uint32_t flipv, uint32_t& f0, uint32_t& f1,
                                           uint32_t& f2) {
  uint32_t key2 = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(key))), t;
  asm volatile("" : "+s"(key2));   // an opaque copy of the key
  asm volatile(NANOGPU_SREG_ROW0(NANOGPU_SREG_W) NANOGPU_SREG_ROW1(NANOGPU_SREG_W) NANOGPU_SREG_ROW2(NANOGPU_SREG_W)
               NANOGPU_SREG_ROW0(NANOGPU_SREG_V, "f0") NANOGPU_SREG_ROW1(NANOGPU_SREG_V, "f1")
               NANOGPU_SREG_ROW2(NANOGPU_SREG_V, "f2")
               : [f0] "+s"(f0), [f1] "+s"(f1), [f2] "+s"(f2), [t] "=&s"(t)
               : [key] "s"(key), [key2] "s"(key2), [cm] "s"(cm), [inj] "s"(inj), [flipv] "s"(flipv)
               : NANOGPU_SREG_ROW0(NANOGPU_SREG_NAME) NANOGPU_SREG_ROW1(NANOGPU_SREG_NAME) NANOGPU_SREG_ROW2(NANOGPU_SREG_NAME)
                 "scc");
}

__device__ __forceinline__ void sregs_test(uint32_t key, uint32_t inj, bool wave0, uint32_t (&flags)[ss::kSregFlags]) {
  uint32_t f0 = 0, f1 = 0, f2 = 0;
  key = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(key)));
  inj = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(inj)));
  const uint32_t flipv = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(wave0 ? 1 : 0));
  sregs_pass(key, 0u, inj, flipv, f0, f1, f2);
  sregs_pass(key, ~0u, inj, 0u, f0, f1, f2);
  flags[0] = f0;
  flags[1] = f1;
  flags[2] = f2;
}
#undef NANOGPU_SREG_W
#undef NANOGPU_SREG_V
#undef NANOGPU_SREG_ROW0
#undef NANOGPU_SREG_ROW1
#undef NANOGPU_SREG_ROW2
#undef NANOGPU_SREG_NAME

// More than half of the CU's 160 KiB: two of these workgroups do not fit one CU, so a grid of
// rounds x CUs workgroups is spread over every enabled CU, as cu_sweep_kernel's is.
constexpr uint32_t kScalarLdsDwords = 21504;   // 84 KiB
static_assert(kScalarLdsDwords * 2 > kLdsDwordsFull && kScalarLdsDwords >= ss::kTableWords + 8, "alone on its CU; the table fits");

// One visit of one CU, on the grid and the stream of cu_sweep_kernel: all four waves (one per SIMD)
// run every selected exact group against the host's table (staged in LDS), the scalar loads and the
// register test. One record per workgroup. It never writes EXEC, M0 or a hardware register; results
// leave the scalar unit only as operands of vector instructions. No spin, no inter-workgroup
// traffic, every loop bounded by a constant.
__global__ __launch_bounds__(kSweepBlock) void cu_scalar_kernel(const uint32_t* __restrict__ table,
                                                                const uint32_t* __restrict__ loads, uint32_t* __restrict__ out,
                                                                uint32_t seed, ScalarInject inj, uint32_t groups) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kScalarLdsDwords];
  uint32_t* red = lds + ss::kTableWords;   // 0 fail, 1 simds, 2 groups, 3 first bad (pack_bad)
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(tid >> 6));
  uint32_t xcc, hwid;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
  const bool mine = __builtin_amdgcn_readfirstlane(inj.kind != kScalarInjectNone && xcc == static_cast<uint32_t>(inj.xcc) &&
                                                   st::hw_cu_key(hwid) == static_cast<uint32_t>(inj.cu_key)) != 0;   // provably uniform: an asm operand below
  if (tid < ss::kTableWords) lds[tid] = table[tid];
  if (tid < 4) red[tid] = tid == 3 ? ss::kNoBad : 0u;
  __syncthreads();

  const uint32_t group_bad = scalar_groups_checked(ScalarExact{}, groups, wave, static_cast<int>(lane), lds,
                                                   mine && inj.kind == kScalarInjectGroup && wave == 0 ? inj.arg : -1);
  uint32_t fail = group_bad ? 1u << (ss::kFailExactShift + wave) : 0u;
  uint32_t first_bad = ss::kNoBad;
  if (groups >> ss::kSmem & 1u) {    // wave-uniform
    const uint32_t word = smem_test(loads, wave, mine && inj.kind == kScalarInjectSmem ? static_cast<uint32_t>(inj.arg) : ss::kNoBad);
    if (word != ss::kNoBad) {
      fail |= 1u << (ss::kFailSmemShift + wave);
      first_bad = ss::pack_bad(ss::kBadSmem, word, static_cast<uint32_t>(wave));
    }
  }
  if (groups >> ss::kSregs & 1u) {   // wave-uniform
    uint32_t flags[ss::kSregFlags];
    const uint32_t slot = mine && inj.kind == kScalarInjectSregs ? static_cast<uint32_t>(inj.arg) : ss::kNoBad;
    sregs_test(seed ^ static_cast<uint32_t>(wave), slot, wave == 0, flags);
    if (flags[0] | flags[1] | flags[2]) {
      const uint32_t bad_slot = flags[0]   ? static_cast<uint32_t>(__builtin_ctz(flags[0]))
                                : flags[1] ? 32u + static_cast<uint32_t>(__builtin_ctz(flags[1]))
                                           : 64u + static_cast<uint32_t>(__builtin_ctz(flags[2]));
      fail |= 1u << (ss::kFailSregsShift + wave);
      first_bad = ss::pack_bad(ss::kBadSregs, bad_slot, static_cast<uint32_t>(wave));   // before a table word
    }
  }
  if (lane == 0) {
    if (fail) atomicOr(&red[0], fail);
    if (group_bad) atomicOr(&red[2], group_bad);
    if (first_bad != ss::kNoBad) atomicMin(&red[3], first_bad);
    atomicOr(&red[1], 1u << st::hw_simd(hwid));
  }
  __syncthreads();
  if (tid == 0) {
    uint32_t* o = out + static_cast<size_t>(blockIdx.x) * ss::kScalarRecordWords;
    const uint32_t b = red[3];
    o[0] = xcc;
    o[1] = hwid;
    o[2] = red[0];
    o[3] = red[1];
    o[4] = red[2];
    o[5] = b == ss::kNoBad ? ss::kNoBad : (b >> 8) & 0xffffu;
    o[6] = b == ss::kNoBad ? ss::kNoBad : b & 0xffu;
    o[7] = b == ss::kNoBad ? ss::kNoBad : b >> 24;
  }
}

// One workgroup of four waves, one group: wave w's kWaveWords raw words at out[w * kWaveWords ..]. It
// establishes on the device that the kernel's instruction sequence is the twin's arithmetic.
template <int G>
__global__ __launch_bounds__(kSweepBlock) void scalar_words_kernel(uint32_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  scalar_chain<G>(wave, lane, [&](int s, uint32_t h) {
    if (lane == 0) out[wave * ss::kWaveWords + s] = h;
  });
}

// ---------------------------------------------------------------------------- memory part
// The CU's memory pipeline (nanogpu/selftest_mem_host.h): global and buffer loads and stores of every
// width, the per-CU L1, LDS instruction forms, the transposed LDS read, LDS-DMA and atomics with
// return. Every instruction form is one asm statement that ends in its own wait, or a builtin the
// compiler counts itself. The statements take per-lane addresses in VGPRs; the only scalar operand
// of an asm statement is the buffer descriptor, and that statement opens with the wait states a
// fresh SGPR needs.
namespace sm = nanogpu::selftest::mem;
using u32x3v = __attribute__((ext_vector_type(3))) uint32_t;

#define NANOGPU_MEM_LOAD(name, text, T)                                                                           \
  __device__ __forceinline__ T name(const void* p) {                                                              \
    T r;                                                                                                          \
    asm volatile(text "\n\ts_waitcnt vmcnt(0)" : "=&v"(r) : "v"(p) : "memory");                                   \
    return r;                                                                                                     \
  }
// A d16 load writes one half of its register; that half is returned.
#define NANOGPU_MEM_LOAD_D16(name, text, hi)                                                                      \
  __device__ __forceinline__ uint32_t name(const void* p) {                                                       \
    uint32_t r = sm::kD16Init;                                                                                    \
    asm volatile(text "\n\ts_waitcnt vmcnt(0)" : "+v"(r) : "v"(p) : "memory");                                    \
    return sm::gload_d16_half(r, hi);                                                                             \
  }
#define NANOGPU_MEM_STORE(name, text, T)                                                                          \
  __device__ __forceinline__ void name(void* p, T v) { asm volatile(text "\n\ts_waitcnt vmcnt(0)" : : "v"(p), "v"(v) : "memory"); }
NANOGPU_MEM_LOAD(gl_ubyte, "global_load_ubyte %0, %1, off", uint32_t)
NANOGPU_MEM_LOAD(gl_sbyte, "global_load_sbyte %0, %1, off", uint32_t)
NANOGPU_MEM_LOAD(gl_ushort, "global_load_ushort %0, %1, off", uint32_t)
NANOGPU_MEM_LOAD(gl_sshort, "global_load_sshort %0, %1, off", uint32_t)
NANOGPU_MEM_LOAD_D16(gl_ubyte_d16, "global_load_ubyte_d16 %0, %1, off", false)
NANOGPU_MEM_LOAD_D16(gl_ubyte_d16_hi, "global_load_ubyte_d16_hi %0, %1, off", true)
NANOGPU_MEM_LOAD_D16(gl_sbyte_d16, "global_load_sbyte_d16 %0, %1, off", false)
NANOGPU_MEM_LOAD_D16(gl_sbyte_d16_hi, "global_load_sbyte_d16_hi %0, %1, off", true)
NANOGPU_MEM_LOAD_D16(gl_short_d16, "global_load_short_d16 %0, %1, off", false)
NANOGPU_MEM_LOAD_D16(gl_short_d16_hi, "global_load_short_d16_hi %0, %1, off", true)
NANOGPU_MEM_LOAD(gl_x1, "global_load_dword %0, %1, off", uint32_t)
NANOGPU_MEM_LOAD(gl_x2, "global_load_dwordx2 %0, %1, off", u32x2v)
NANOGPU_MEM_LOAD(gl_x3, "global_load_dwordx3 %0, %1, off", u32x3v)
NANOGPU_MEM_LOAD(gl_x4, "global_load_dwordx4 %0, %1, off", u32x4v)
NANOGPU_MEM_LOAD(gl_x4_nt, "global_load_dwordx4 %0, %1, off nt", u32x4v)
NANOGPU_MEM_LOAD(gl_x4_sc0, "global_load_dwordx4 %0, %1, off sc0", u32x4v)
NANOGPU_MEM_LOAD(gl_x4_sc1, "global_load_dwordx4 %0, %1, off sc1", u32x4v)
NANOGPU_MEM_LOAD(gl_x4_sc0sc1, "global_load_dwordx4 %0, %1, off sc0 sc1", u32x4v)
NANOGPU_MEM_STORE(gs_byte, "global_store_byte %0, %1, off", uint32_t)
NANOGPU_MEM_STORE(gs_short, "global_store_short %0, %1, off", uint32_t)
NANOGPU_MEM_STORE(gs_short_d16_hi, "global_store_short_d16_hi %0, %1, off", uint32_t)
NANOGPU_MEM_STORE(gs_x1, "global_store_dword %0, %1, off", uint32_t)
NANOGPU_MEM_STORE(gs_x2, "global_store_dwordx2 %0, %1, off", u32x2v)
NANOGPU_MEM_STORE(gs_x3, "global_store_dwordx3 %0, %1, off", u32x3v)
NANOGPU_MEM_STORE(gs_x4, "global_store_dwordx4 %0, %1, off", u32x4v)
#undef NANOGPU_MEM_LOAD
#undef NANOGPU_MEM_LOAD_D16
#undef NANOGPU_MEM_STORE

// LDS statements take the byte address in the LDS aperture.
#define NANOGPU_DS_READ(name, text, T)                                                                            \
  __device__ __forceinline__ T name(uint32_t a) {                                                                 \
    T r;                                                                                                          \
    asm volatile(text "\n\ts_waitcnt lgkmcnt(0)" : "=&v"(r) : "v"(a) : "memory");                                 \
    return r;                                                                                                     \
  }
#define NANOGPU_DS_WRITE(name, text, T)                                                                           \
  __device__ __forceinline__ void name(uint32_t a, T v) { asm volatile(text "\n\ts_waitcnt lgkmcnt(0)" : : "v"(a), "v"(v) : "memory"); }
#define NANOGPU_DS_WRITE2(name, text, T)                                                                          \
  __device__ __forceinline__ void name(uint32_t a, T v, T w) {                                                    \
    asm volatile(text "\n\ts_waitcnt lgkmcnt(0)" : : "v"(a), "v"(v), "v"(w) : "memory");                          \
  }
NANOGPU_DS_READ(ds_r_u8, "ds_read_u8 %0, %1", uint32_t)
NANOGPU_DS_READ(ds_r_i8, "ds_read_i8 %0, %1", uint32_t)
NANOGPU_DS_READ(ds_r_u16, "ds_read_u16 %0, %1", uint32_t)
NANOGPU_DS_READ(ds_r_i16, "ds_read_i16 %0, %1", uint32_t)
NANOGPU_DS_READ(ds_r_b32, "ds_read_b32 %0, %1", uint32_t)
NANOGPU_DS_READ(ds_r_b64, "ds_read_b64 %0, %1", u32x2v)
NANOGPU_DS_READ(ds_r_b96, "ds_read_b96 %0, %1", u32x3v)
NANOGPU_DS_READ(ds_r_b128, "ds_read_b128 %0, %1", u32x4v)
NANOGPU_DS_READ(ds_r2_b32, "ds_read2_b32 %0, %1 offset0:0 offset1:2", u32x2v)
NANOGPU_DS_READ(ds_r2_b64, "ds_read2_b64 %0, %1 offset0:0 offset1:1", u32x4v)
NANOGPU_DS_READ(ds_r2st64_b32, "ds_read2st64_b32 %0, %1 offset0:0 offset1:16", u32x2v)
NANOGPU_DS_READ(ds_r2st64_b64, "ds_read2st64_b64 %0, %1 offset0:0 offset1:8", u32x4v)
NANOGPU_DS_READ(ds_r_tr_b16, "ds_read_b64_tr_b16 %0, %1", u32x2v)
NANOGPU_DS_WRITE(ds_w_b8, "ds_write_b8 %0, %1", uint32_t)
NANOGPU_DS_WRITE(ds_w_b16, "ds_write_b16 %0, %1", uint32_t)
NANOGPU_DS_WRITE(ds_w_b32, "ds_write_b32 %0, %1", uint32_t)
NANOGPU_DS_WRITE(ds_w_b64, "ds_write_b64 %0, %1", u32x2v)
NANOGPU_DS_WRITE(ds_w_b96, "ds_write_b96 %0, %1", u32x3v)
NANOGPU_DS_WRITE(ds_w_b128, "ds_write_b128 %0, %1", u32x4v)
NANOGPU_DS_WRITE2(ds_w2_b32, "ds_write2_b32 %0, %1, %2 offset0:0 offset1:2", uint32_t)
NANOGPU_DS_WRITE2(ds_w2_b64, "ds_write2_b64 %0, %1, %2 offset0:0 offset1:1", u32x2v)
NANOGPU_DS_WRITE2(ds_w2st64_b32, "ds_write2st64_b32 %0, %1, %2 offset0:0 offset1:16", uint32_t)
NANOGPU_DS_WRITE2(ds_w2st64_b64, "ds_write2st64_b64 %0, %1, %2 offset0:0 offset1:8", u32x2v)
#undef NANOGPU_DS_READ
#undef NANOGPU_DS_WRITE
#undef NANOGPU_DS_WRITE2
static_assert(sm::kLdsUpper == 16 * 64 * 4 && sm::kLdsUpper == 8 * 64 * 8, "offset1 of the st64 statements");

// Everything this wave has in flight, whoever issued it.
__device__ __forceinline__ void mem_drain() { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); }

// Raw buffer statements, M: 0 offen, 1 offen with soffset 64, 2 offen with the immediate offset 48. The descriptor is four
// SGPRs fresh from readfirstlane, so every statement opens with the wait states such an operand needs.
#define NANOGPU_BUF_ASM(mnemonic, tail, outs, ...) \
  asm volatile("s_nop 4\n\t" mnemonic " %0, %1, %2, " tail "\n\ts_waitcnt vmcnt(0)" : outs : __VA_ARGS__ : "memory")
#define NANOGPU_BUF_LOAD(name, mnemonic, T)                                                                       \
  template <int M>                                                                                                \
  __device__ __forceinline__ T name(u32x4v rs, uint32_t voffset) {                                                \
    T r;                                                                                                          \
    if constexpr (M == 0) NANOGPU_BUF_ASM(mnemonic, "0 offen", "=&v"(r), "v"(voffset), "s"(rs));                  \
    if constexpr (M == 1) NANOGPU_BUF_ASM(mnemonic, "64 offen", "=&v"(r), "v"(voffset), "s"(rs));                 \
    if constexpr (M == 2) NANOGPU_BUF_ASM(mnemonic, "0 offen offset:48", "=&v"(r), "v"(voffset), "s"(rs));        \
    return r;                                                                                                     \
  }
#define NANOGPU_BUF_STORE(name, mnemonic, T)                                                                      \
  template <int M>                                                                                                \
  __device__ __forceinline__ void name(u32x4v rs, uint32_t voffset, T v) {                                        \
    if constexpr (M == 0) NANOGPU_BUF_ASM(mnemonic, "0 offen", , "v"(v), "v"(voffset), "s"(rs));                  \
    if constexpr (M == 1) NANOGPU_BUF_ASM(mnemonic, "64 offen", , "v"(v), "v"(voffset), "s"(rs));                 \
    if constexpr (M == 2) NANOGPU_BUF_ASM(mnemonic, "0 offen offset:48", , "v"(v), "v"(voffset), "s"(rs));        \
  }
NANOGPU_BUF_LOAD(bl_b8, "buffer_load_ubyte", uint32_t)
NANOGPU_BUF_LOAD(bl_b16, "buffer_load_ushort", uint32_t)
NANOGPU_BUF_LOAD(bl_b32, "buffer_load_dword", uint32_t)
NANOGPU_BUF_LOAD(bl_b64, "buffer_load_dwordx2", u32x2v)
NANOGPU_BUF_LOAD(bl_b96, "buffer_load_dwordx3", u32x3v)
NANOGPU_BUF_LOAD(bl_b128, "buffer_load_dwordx4", u32x4v)
NANOGPU_BUF_STORE(bs_b8, "buffer_store_byte", uint32_t)
NANOGPU_BUF_STORE(bs_b16, "buffer_store_short", uint32_t)
NANOGPU_BUF_STORE(bs_b32, "buffer_store_dword", uint32_t)
NANOGPU_BUF_STORE(bs_b64, "buffer_store_dwordx2", u32x2v)
NANOGPU_BUF_STORE(bs_b96, "buffer_store_dwordx3", u32x3v)
NANOGPU_BUF_STORE(bs_b128, "buffer_store_dwordx4", u32x4v)
#undef NANOGPU_BUF_LOAD
#undef NANOGPU_BUF_STORE
#undef NANOGPU_BUF_ASM
static_assert(sm::kBufSoffset == 64 && sm::kBufImm == 48, "the soffset and the immediate of the statements above");

// What a group works on: the table, the wave's region of the slice and of the LDS array (as a pointer
// and as the byte address the ds_ statements take). `wave` is wave-uniform to the compiler.
struct MemCtx {
  const uint32_t* table;
  char* slice;
  uint32_t* lds;
  uint32_t lds_at;
  int wave, lane;
};

// The sweep's sink: the lowest index whose word is not what the header computes. `inject` (kNoBad:
// none) is the index whose expected value has bit 0 flipped.
struct MemCheck {
  int lane;
  uint32_t inject, bad;
  __device__ __forceinline__ void at(int, uint32_t index, uint32_t got, uint32_t want) {
    if (got != (want ^ (index == inject ? 1u : 0u)) && index < bad) bad = index;
  }
  __device__ __forceinline__ void word(int k, uint32_t got, uint32_t want) { at(k, static_cast<uint32_t>(k * sm::kLanes + lane), got, want); }
};

// mem_lanes' sink: the raw words, [wave][k][lane].
struct MemKeep {
  uint32_t* out;
  int words, wave, lane;
  __device__ __forceinline__ void at(int k, uint32_t, uint32_t got, uint32_t) { out[(wave * words + k) * sm::kLanes + lane] = got; }
  __device__ __forceinline__ void word(int k, uint32_t got, uint32_t want) { at(k, 0u, got, want); }
};

template <int N, class V, class Sink, class Want>
__device__ __forceinline__ void mem_words(Sink& sink, int first, const V& got, Want&& want) {
#pragma unroll
  for (int j = 0; j < N; ++j) {
    uint32_t g;
    if constexpr (std::is_same_v<V, uint32_t>) g = got;
    else g = got[j];
    sink.word(first + j, g, want(j));
  }
}

template <class Sink>
__device__ __forceinline__ void mem_gload(const MemCtx& c, Sink& sink) {
#pragma nounroll
  for (int map = 0; map < sm::kGloadMaps; ++map) {
    auto p = [&](int f) { return reinterpret_cast<const char*>(c.table) + sm::gload_addr(map, c.wave, c.lane, f); };
    auto one = [&](int f, uint32_t got) { sink.word(sm::gload_k(map, f, 0), got, sm::gload_expected(map, c.wave, c.lane, f, 0)); };
    auto want = [&](int f) { return [&c, map, f](int j) { return sm::gload_expected(map, c.wave, c.lane, f, j); }; };
    one(0, gl_ubyte(p(0)));
    one(1, gl_ubyte(p(1)));
    one(2, gl_ubyte(p(2)));
    one(3, gl_ubyte(p(3)));
    one(4, gl_sbyte(p(4)));
    one(5, gl_sbyte(p(5)));
    one(6, gl_sbyte(p(6)));
    one(7, gl_sbyte(p(7)));
    one(8, gl_ushort(p(8)));
    one(9, gl_ushort(p(9)));
    one(10, gl_sshort(p(10)));
    one(11, gl_sshort(p(11)));
    one(12, gl_ubyte_d16(p(12)));
    one(13, gl_ubyte_d16_hi(p(13)));
    one(14, gl_sbyte_d16(p(14)));
    one(15, gl_sbyte_d16_hi(p(15)));
    one(16, gl_short_d16(p(16)));
    one(17, gl_short_d16_hi(p(17)));
    one(18, gl_x1(p(18)));
    mem_words<2>(sink, sm::gload_k(map, 19, 0), gl_x2(p(19)), want(19));
    mem_words<3>(sink, sm::gload_k(map, 20, 0), gl_x3(p(20)), want(20));
    mem_words<4>(sink, sm::gload_k(map, 21, 0), gl_x4(p(21)), want(21));
    mem_words<4>(sink, sm::gload_k(map, 22, 0), gl_x4_nt(p(22)), want(22));
    mem_words<4>(sink, sm::gload_k(map, 23, 0), gl_x4_sc0(p(23)), want(23));
    mem_words<4>(sink, sm::gload_k(map, 24, 0), gl_x4_sc1(p(24)), want(24));
    mem_words<4>(sink, sm::gload_k(map, 25, 0), gl_x4_sc0sc1(p(25)), want(25));
  }
}
static_assert(sm::kGloadForms == 26 && sm::gload_kind(17) == sm::kShortD16Hi && sm::gload_kind(18) == sm::kDwords, "the statements above, in the header's order");

// Four loads, then one wait, a statement: every wave reads every line of the table, twice.
template <class Sink>
__device__ __forceinline__ void mem_l1(const MemCtx& c, Sink& sink) {
#pragma nounroll
  for (int pass = 0; pass < sm::kL1Passes; ++pass) {
#pragma nounroll
    for (int step = 0; step < sm::kL1Steps; step += 4) {
      const u32x4v* t = reinterpret_cast<const u32x4v*>(c.table);
      uint32_t chunk[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) chunk[i] = sm::l1_chunk(pass, step + i, c.lane);
      u32x4v v0, v1, v2, v3;
      asm volatile("global_load_dwordx4 %0, %4, off\n\tglobal_load_dwordx4 %1, %5, off\n\tglobal_load_dwordx4 %2, %6, off\n\t"
                   "global_load_dwordx4 %3, %7, off\n\ts_waitcnt vmcnt(0)"
                   : "=&v"(v0), "=&v"(v1), "=&v"(v2), "=&v"(v3)
                   : "v"(t + chunk[0]), "v"(t + chunk[1]), "v"(t + chunk[2]), "v"(t + chunk[3])
                   : "memory");
      const u32x4v v[4] = {v0, v1, v2, v3};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t word = 4 * chunk[i] + j;
          sink.at(sm::l1_k(pass, step + i, j), word, v[i][j], sm::table_word(word));
        }
    }
  }
}
static_assert(sm::kL1Steps % 4 == 0, "four loads a statement");

template <class Sink>
__device__ __forceinline__ void mem_gstore(const MemCtx& c, Sink& sink) {
  auto form = [&](auto fc) {
    constexpr int f = decltype(fc)::value;
    u32x4v bg;
#pragma unroll
    for (int j = 0; j < 4; ++j) bg[j] = sm::gstore_bg(c.wave, f, 4 * c.lane + j);
    gs_x4(c.slice + 16 * c.lane, bg);
    const uint32_t chunk = sm::gstore_chunk(c.wave, c.lane, f);
    char* p = c.slice + chunk + sm::gstore_sub(c.lane, f);
    auto v = [&](int j) { return sm::gstore_val(c.wave, c.lane, f, j); };
    if constexpr (f == 0) gs_byte(p, v(0));
    if constexpr (f == 1) gs_short(p, v(0));
    if constexpr (f == 2) gs_short_d16_hi(p, v(0));
    if constexpr (f == 3) gs_x1(p, v(0));
    if constexpr (f == 4) gs_x2(p, u32x2v{v(0), v(1)});
    if constexpr (f == 5) gs_x3(p, u32x3v{v(0), v(1), v(2)});
    if constexpr (f == 6) gs_x4(p, u32x4v{v(0), v(1), v(2), v(3)});
    mem_words<4>(sink, sm::gstore_k(f, 0), gl_x4(c.slice + chunk), [&](int j) { return sm::gstore_expected(c.wave, c.lane, f, j); });
  };
  form(std::integral_constant<int, 0>{});
  form(std::integral_constant<int, 1>{});
  form(std::integral_constant<int, 2>{});
  form(std::integral_constant<int, 3>{});
  form(std::integral_constant<int, 4>{});
  form(std::integral_constant<int, 5>{});
  form(std::integral_constant<int, 6>{});
}
static_assert(sm::kGstoreForms == 7, "the forms above");

// W: the header's width index (1, 2, 4, 8, 12, 16 bytes); M: 0 offen, 1 soffset, 2 immediate. The result is padded to four words.
template <int W, int M>
__device__ __forceinline__ u32x4v mem_buf_load(u32x4v rs, uint32_t voffset) {
  u32x4v r = {0u, 0u, 0u, 0u};
  if constexpr (W == 0) r[0] = bl_b8<M>(rs, voffset);
  if constexpr (W == 1) r[0] = bl_b16<M>(rs, voffset);
  if constexpr (W == 2) r[0] = bl_b32<M>(rs, voffset);
  if constexpr (W == 3) { const u32x2v v = bl_b64<M>(rs, voffset); r[0] = v[0], r[1] = v[1]; }
  if constexpr (W == 4) { const u32x3v v = bl_b96<M>(rs, voffset); r[0] = v[0], r[1] = v[1], r[2] = v[2]; }
  if constexpr (W == 5) r = bl_b128<M>(rs, voffset);
  return r;
}

template <int W, int M>
__device__ __forceinline__ void mem_buf_store(u32x4v rs, uint32_t voffset, u32x4v v) {
  if constexpr (W == 0) bs_b8<M>(rs, voffset, v[0]);
  if constexpr (W == 1) bs_b16<M>(rs, voffset, v[0]);
  if constexpr (W == 2) bs_b32<M>(rs, voffset, v[0]);
  if constexpr (W == 3) bs_b64<M>(rs, voffset, u32x2v{v[0], v[1]});
  if constexpr (W == 4) bs_b96<M>(rs, voffset, u32x3v{v[0], v[1], v[2]});
  if constexpr (W == 5) bs_b128<M>(rs, voffset, v);
}

// The wave's whole region, background `phase`.
__device__ __forceinline__ void mem_buf_background(const MemCtx& c, int phase) {
#pragma unroll
  for (uint32_t i = 0; i < sm::kWaveBytes / (16 * sm::kLanes); ++i) {
    const uint32_t chunk = c.lane + 64 * i;
    u32x4v bg;
#pragma unroll
    for (int j = 0; j < 4; ++j) bg[j] = sm::buf_bg(c.wave, phase, 4 * chunk + j);
    gs_x4(c.slice + 16 * chunk, bg);
  }
}

template <class Sink>
__device__ __forceinline__ void mem_buffer(const MemCtx& c, Sink& sink) {
  // the descriptor from wave-uniform values only: the halves of the region's address through readfirstlane
  const uint64_t base = reinterpret_cast<uint64_t>(c.slice);
  const uint32_t lo = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(base)));
  const uint32_t hi = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(base >> 32)));
  const u32x4v rs = {lo, hi & 0xffffu, sm::kBufRecords, 0x00020000u};   // stride 0, raw
  mem_buf_background(c, 0);
  auto load = [&](auto wc, auto mc) {
    constexpr int w = decltype(wc)::value, m = decltype(mc)::value;
    const u32x4v r = mem_buf_load<w, m>(rs, sm::buf_voffset(w, m, c.lane));
    mem_words<sm::buf_words(w)>(sink, sm::buf_load_k(w, m, 0), r, [&](int j) { return sm::buf_load_expected(c.wave, c.lane, w, m, j); });
  };
  auto store = [&](auto wc, auto mc) {
    constexpr int w = decltype(wc)::value, m = decltype(mc)::value;
    mem_buf_background(c, 1 + 3 * w + m);
    u32x4v v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = sm::buf_val(c.wave, c.lane, w, m, j);
    mem_buf_store<w, m>(rs, sm::buf_voffset(w, m, c.lane), v);
    mem_words<4>(sink, sm::buf_store_k(w, m, 0), gl_x4(c.slice + (sm::buf_addr(w, m, c.lane) & ~15u)),
                 [&](int j) { return sm::buf_store_expected(c.wave, c.lane, w, m, j); });
  };
  auto widths = [&](auto&& op, auto mc) {
    op(std::integral_constant<int, 0>{}, mc);
    op(std::integral_constant<int, 1>{}, mc);
    op(std::integral_constant<int, 2>{}, mc);
    op(std::integral_constant<int, 3>{}, mc);
    op(std::integral_constant<int, 4>{}, mc);
    op(std::integral_constant<int, 5>{}, mc);
  };
  widths(load, std::integral_constant<int, 0>{});
  widths(load, std::integral_constant<int, 1>{});
  widths(load, std::integral_constant<int, 2>{});
  widths(store, std::integral_constant<int, 0>{});
  widths(store, std::integral_constant<int, 1>{});
  widths(store, std::integral_constant<int, 2>{});
}
static_assert(sm::kBufWidths == 6 && sm::kBufModes == 3, "the forms above");

__device__ __forceinline__ u32x4v mem_lds_bg4(int wave, int phase, uint32_t at) {   // the chunk at byte `at` of the wave's region
  u32x4v bg;
#pragma unroll
  for (int j = 0; j < 4; ++j) bg[j] = sm::lds_bg(wave, phase, at / 4 + j);
  return bg;
}

template <class Sink>
__device__ __forceinline__ void mem_lds(const MemCtx& c, Sink& sink) {
#pragma nounroll
  for (int map = 0; map < sm::kLdsMaps; ++map) {
    const uint32_t chunk = sm::lds_chunk(map, c.lane), a = c.lds_at + chunk;
    auto background = [&](int phase) {
      ds_w_b128(a, mem_lds_bg4(c.wave, phase, chunk));
      ds_w_b128(a + sm::kLdsUpper, mem_lds_bg4(c.wave, phase, chunk + sm::kLdsUpper));
    };
    background(0);
    auto sub = [&](int f) { return a + sm::lds_read_sub(c.lane, f); };
    auto want = [&](int f) { return [&c, map, f](int j) { return sm::lds_read_expected(c.wave, c.lane, map, f, j); }; };
    auto first = [&](int f) { return sm::lds_read_k(map, f, 0); };
    mem_words<1>(sink, first(0), ds_r_u8(sub(0)), want(0));
    mem_words<1>(sink, first(1), ds_r_i8(sub(1)), want(1));
    mem_words<1>(sink, first(2), ds_r_u16(sub(2)), want(2));
    mem_words<1>(sink, first(3), ds_r_i16(sub(3)), want(3));
    mem_words<1>(sink, first(4), ds_r_b32(sub(4)), want(4));
    mem_words<2>(sink, first(5), ds_r_b64(sub(5)), want(5));
    mem_words<3>(sink, first(6), ds_r_b96(sub(6)), want(6));
    mem_words<4>(sink, first(7), ds_r_b128(sub(7)), want(7));
    mem_words<2>(sink, first(8), ds_r2_b32(a), want(8));
    mem_words<4>(sink, first(9), ds_r2_b64(a), want(9));
    mem_words<2>(sink, first(10), ds_r2st64_b32(a), want(10));
    mem_words<4>(sink, first(11), ds_r2st64_b64(a), want(11));
    auto write = [&](auto fc) {
      constexpr int f = decltype(fc)::value;
      background(1 + 10 * map + f);
      auto v = [&](int j) { return sm::lds_val(c.wave, c.lane, map, f, j); };
      const uint32_t at = a + sm::lds_write_sub(c.lane, f);
      if constexpr (f == 0) ds_w_b8(at, v(0));
      if constexpr (f == 1) ds_w_b16(at, v(0));
      if constexpr (f == 2) ds_w_b32(at, v(0));
      if constexpr (f == 3) ds_w_b64(at, u32x2v{v(0), v(1)});
      if constexpr (f == 4) ds_w_b96(at, u32x3v{v(0), v(1), v(2)});
      if constexpr (f == 5) ds_w_b128(at, u32x4v{v(0), v(1), v(2), v(3)});
      if constexpr (f == 6) ds_w2_b32(at, v(0), v(1));
      if constexpr (f == 7) ds_w2_b64(at, u32x2v{v(0), v(1)}, u32x2v{v(2), v(3)});
      if constexpr (f == 8) ds_w2st64_b32(at, v(0), v(1));
      if constexpr (f == 9) ds_w2st64_b64(at, u32x2v{v(0), v(1)}, u32x2v{v(2), v(3)});
      auto wantw = [&](int up) { return [&c, map, up](int j) { return sm::lds_write_expected(c.wave, c.lane, map, f, 4 * up + j); }; };
      mem_words<4>(sink, sm::lds_write_k(map, f, 0), ds_r_b128(a), wantw(0));
      if constexpr (f >= 8) mem_words<4>(sink, sm::lds_write_k(map, f, 4), ds_r_b128(a + sm::kLdsUpper), wantw(1));
    };
    write(std::integral_constant<int, 0>{});
    write(std::integral_constant<int, 1>{});
    write(std::integral_constant<int, 2>{});
    write(std::integral_constant<int, 3>{});
    write(std::integral_constant<int, 4>{});
    write(std::integral_constant<int, 5>{});
    write(std::integral_constant<int, 6>{});
    write(std::integral_constant<int, 7>{});
    write(std::integral_constant<int, 8>{});
    write(std::integral_constant<int, 9>{});
  }
}
static_assert(sm::kLdsReadForms == 12 && sm::kLdsWriteForms == 10, "the forms above");

// All 64 lanes are active: the caller's branch around the group is wave-uniform and nothing here diverges.
template <class Sink>
__device__ __forceinline__ void mem_ldstr(const MemCtx& c, Sink& sink) {
#pragma unroll
  for (int s = 0; s < sm::kLdstrSteps; ++s) {
    const uint32_t a = c.lds_at + sm::ldstr_addr(s, c.lane);
    ds_w_b64(a, u32x2v{sm::ldstr_written(c.wave, s, c.lane, 0), sm::ldstr_written(c.wave, s, c.lane, 1)});
    mem_words<2>(sink, sm::ldstr_k(s, 0), ds_r_tr_b16(a), [&](int j) { return sm::ldstr_expected(c.wave, s, c.lane, j); });
  }
}

using lds_u32_ptr = __attribute__((address_space(3))) uint32_t*;

template <class Sink>
__device__ __forceinline__ void mem_ldsdma(const MemCtx& c, Sink& sink) {
#pragma unroll
  for (int f = 0; f < sm::kDmaForms; ++f) ds_w_b128(c.lds_at + sm::dma_dst(f) + 16 * c.lane, u32x4v{sm::kDmaBg, sm::kDmaBg, sm::kDmaBg, sm::kDmaBg});
  auto src = [&](int f) { return reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(c.table) + sm::dma_src(c.wave, c.lane, f)); };
  auto dst = [&](int f) { return (lds_u32_ptr)(c.lds + sm::dma_dst(f) / 4); };   // wave-uniform: the hardware adds lane x size
  __builtin_amdgcn_global_load_lds(src(0), dst(0), 4, 0, 0);
  __builtin_amdgcn_global_load_lds(src(1), dst(1), 16, 0, 0);
  const __amdgpu_buffer_rsrc_t table = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(c.table), 0, sm::kTableBytes, 0x00020000);
  __builtin_amdgcn_raw_ptr_buffer_load_lds(table, dst(2), 4, sm::dma_src(c.wave, c.lane, 2), 0, 0, 0);
  mem_drain();   // LDS-DMA is counted by vmcnt; the reads below are this wave's own
#pragma unroll
  for (int f = 0; f < sm::kDmaForms; ++f)
#pragma unroll
    for (int j = 0; j < sm::dma_bytes(f) / 4; ++j)
      sink.word(sm::dma_k(f, j), ds_r_b32(c.lds_at + sm::dma_dst(f) + sm::dma_bytes(f) * c.lane + 4 * j), sm::dma_expected(c.wave, c.lane, f, j));
}

// One atomic with return on *p, which holds a: agent scope on the slice, workgroup scope on LDS.
template <int OP, int SCOPE, class T>
__device__ __forceinline__ T mem_atomic(T* p, T v, T cmp) {
  if constexpr (OP == sm::kAdd || OP == sm::kAdd64) return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, SCOPE);
  if constexpr (OP == sm::kSub) return __hip_atomic_fetch_sub(p, v, __ATOMIC_RELAXED, SCOPE);
  if constexpr (OP == sm::kSmin) return static_cast<T>(__hip_atomic_fetch_min(reinterpret_cast<int32_t*>(p), static_cast<int32_t>(v), __ATOMIC_RELAXED, SCOPE));
  if constexpr (OP == sm::kUmin) return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, SCOPE);
  if constexpr (OP == sm::kSmax) return static_cast<T>(__hip_atomic_fetch_max(reinterpret_cast<int32_t*>(p), static_cast<int32_t>(v), __ATOMIC_RELAXED, SCOPE));
  if constexpr (OP == sm::kUmax || OP == sm::kUmax64) return __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, SCOPE);
  if constexpr (OP == sm::kAnd) return __hip_atomic_fetch_and(p, v, __ATOMIC_RELAXED, SCOPE);
  if constexpr (OP == sm::kOr) return __hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, SCOPE);
  if constexpr (OP == sm::kXor) return __hip_atomic_fetch_xor(p, v, __ATOMIC_RELAXED, SCOPE);
  if constexpr (OP == sm::kInc && SCOPE == __HIP_MEMORY_SCOPE_AGENT) return __builtin_amdgcn_atomic_inc32(p, v, __ATOMIC_RELAXED, "agent");
  if constexpr (OP == sm::kInc && SCOPE != __HIP_MEMORY_SCOPE_AGENT) return __builtin_amdgcn_atomic_inc32(p, v, __ATOMIC_RELAXED, "workgroup");
  if constexpr (OP == sm::kDec && SCOPE == __HIP_MEMORY_SCOPE_AGENT) return __builtin_amdgcn_atomic_dec32(p, v, __ATOMIC_RELAXED, "agent");
  if constexpr (OP == sm::kDec && SCOPE != __HIP_MEMORY_SCOPE_AGENT) return __builtin_amdgcn_atomic_dec32(p, v, __ATOMIC_RELAXED, "workgroup");
  if constexpr (OP == sm::kSwap || OP == sm::kSwap64) return __hip_atomic_exchange(p, v, __ATOMIC_RELAXED, SCOPE);
  if constexpr (OP == sm::kCmpswap || OP == sm::kCmpswap64) {
    __hip_atomic_compare_exchange_strong(p, &cmp, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED, SCOPE);
    return cmp;   // what the location held
  }
  __builtin_unreachable();
}

template <int M, class Sink>
__device__ __forceinline__ void mem_atomic_memory(const MemCtx& c, Sink& sink) {
  constexpr int scope = M == 0 ? __HIP_MEMORY_SCOPE_AGENT : __HIP_MEMORY_SCOPE_WORKGROUP;
  char* region = M == 0 ? c.slice : reinterpret_cast<char*>(c.lds);
  auto op = [&](auto oc) {
    constexpr int o = decltype(oc)::value;
    using T = std::conditional_t<(o < sm::kNumOps32), uint32_t, uint64_t>;
    T* p = reinterpret_cast<T*>(region + 8 * c.lane);
    __hip_atomic_store(p, static_cast<T>(sm::atom_a(M, c.wave, c.lane, o)), __ATOMIC_RELAXED, scope);
    const T got = mem_atomic<o, scope, T>(p, static_cast<T>(sm::atom_v(M, c.wave, c.lane, o)), static_cast<T>(sm::atom_cmp(M, c.wave, c.lane, o)));
    const T after = __hip_atomic_load(p, __ATOMIC_RELAXED, scope);
    constexpr int n = sizeof(T) / 4;
#pragma unroll
    for (int j = 0; j < 2 * n; ++j)
      sink.word(sm::atom_k(M, o, j), static_cast<uint32_t>((j < n ? got : after) >> (32 * (j % n))), sm::atom_expected(M, c.wave, c.lane, o, j));
  };
  op(std::integral_constant<int, sm::kAdd>{});
  op(std::integral_constant<int, sm::kSub>{});
  op(std::integral_constant<int, sm::kSmin>{});
  op(std::integral_constant<int, sm::kUmin>{});
  op(std::integral_constant<int, sm::kSmax>{});
  op(std::integral_constant<int, sm::kUmax>{});
  op(std::integral_constant<int, sm::kAnd>{});
  op(std::integral_constant<int, sm::kOr>{});
  op(std::integral_constant<int, sm::kXor>{});
  op(std::integral_constant<int, sm::kInc>{});
  op(std::integral_constant<int, sm::kDec>{});
  op(std::integral_constant<int, sm::kSwap>{});
  op(std::integral_constant<int, sm::kCmpswap>{});
  op(std::integral_constant<int, sm::kAdd64>{});
  op(std::integral_constant<int, sm::kUmax64>{});
  op(std::integral_constant<int, sm::kSwap64>{});
  op(std::integral_constant<int, sm::kCmpswap64>{});
  // contended: every lane adds c to one word; the flags of the returned values are gathered in LDS
  uint32_t* word = reinterpret_cast<uint32_t*>(region + sm::kAtomContended);
  uint32_t* flags = c.lds + (sm::kAtomContended + 8) / 4;
  __hip_atomic_store(word, sm::atom_cont_b(M, c.wave), __ATOMIC_RELAXED, scope);
  __hip_atomic_store(flags + (c.lane & 1), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  mem_drain();   // another lane's store, before this lane's add
  // one statement, address and operand in VGPRs: 64 lanes' adds reach the atomic unit (the builtin is folded by the
  // compiler into one add of 64 c by one lane when address and operand are wave-uniform)
  uint32_t got;
  const uint32_t add = sm::atom_cont_c(M, c.wave);
  if constexpr (M == 0)
    asm volatile("global_atomic_add %0, %1, %2, off sc0\n\ts_waitcnt vmcnt(0)" : "=&v"(got) : "v"(word), "v"(add) : "memory");
  else
    asm volatile("ds_add_rtn_u32 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=&v"(got) : "v"(c.lds_at + sm::kAtomContended), "v"(add) : "memory");
  const uint32_t q = sm::atom_cont_q(M, c.wave, got);
  __hip_atomic_fetch_or(flags + (q == sm::kNoBad ? 0u : q >> 5), q == sm::kNoBad ? 0u : 1u << (q & 31u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  mem_drain();
  sink.word(sm::atom_cont_k(M, 0), q == sm::kNoBad ? 0u : 1u, sm::atom_cont_expected(M, c.wave, 0));
  sink.word(sm::atom_cont_k(M, 1), __hip_atomic_load(flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP), sm::atom_cont_expected(M, c.wave, 1));
  sink.word(sm::atom_cont_k(M, 2), __hip_atomic_load(flags + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP), sm::atom_cont_expected(M, c.wave, 2));
  sink.word(sm::atom_cont_k(M, 3), __hip_atomic_load(word, __ATOMIC_RELAXED, scope), sm::atom_cont_expected(M, c.wave, 3));
}
static_assert(sm::kNumOps == 17, "the operations above");
static_assert(sm::kDmaForms == 3 && sm::dma_bytes(1) == 16, "mem_ldsdma's three loads");

template <class Sink>
__device__ __forceinline__ void mem_atomic_group(const MemCtx& c, Sink& sink) {
  mem_atomic_memory<0>(c, sink);
  mem_atomic_memory<1>(c, sink);
}

template <int G, class Sink>
__device__ __forceinline__ void mem_group(const MemCtx& c, Sink& sink) {
  if constexpr (G == sm::kGload) mem_gload(c, sink);
  if constexpr (G == sm::kL1) mem_l1(c, sink);
  if constexpr (G == sm::kGstore) mem_gstore(c, sink);
  if constexpr (G == sm::kBuffer) mem_buffer(c, sink);
  if constexpr (G == sm::kLds) mem_lds(c, sink);
  if constexpr (G == sm::kLdstr) mem_ldstr(c, sink);
  if constexpr (G == sm::kLdsdma) mem_ldsdma(c, sink);
  if constexpr (G == sm::kAtomic) mem_atomic_group(c, sink);
}
using MemGroups = std::make_integer_sequence<int, sm::kNumNames>;

// Test hook: on CU (xcc, cu_key), bit 0 flips of the value index `index` of group `group` is compared
// with, on wave index % 4. No held data is touched.
struct MemInject {
  int xcc = -1, cu_key = -1, group = -1, index = -1;
};

// More than half of the CU's 160 KiB, as kScalarLdsDwords: one workgroup a CU.
constexpr uint32_t kMemLdsDwords = sm::kLdsArrayBytes / 4;   // 84 KiB
constexpr uint32_t kMemRed = sm::kWaves * sm::kLdsWaveBytes / 4;
static_assert(kMemLdsDwords * 2 > kLdsDwordsFull && kMemLdsDwords >= kMemRed + 4, "alone on its CU; the waves' regions and the reduction fit");

__device__ __forceinline__ MemCtx mem_ctx(const uint32_t* table, uint8_t* slice, uint32_t* lds, int wave, int lane) {
  return MemCtx{table, reinterpret_cast<char*>(slice) + static_cast<uint32_t>(wave) * sm::kWaveBytes,
                lds + static_cast<uint32_t>(wave) * (sm::kLdsWaveBytes / 4),
                static_cast<uint32_t>(reinterpret_cast<uintptr_t>(lds)) + static_cast<uint32_t>(wave) * sm::kLdsWaveBytes, wave, lane};
}

template <int... G>
__device__ __forceinline__ void mem_groups_checked(std::integer_sequence<int, G...>, const MemCtx& c, uint32_t groups, int inj_group,
                                                   uint32_t inj_index, uint32_t* red) {
  auto one = [&](auto gc) {
    constexpr int g = decltype(gc)::value;
    if (!(groups >> g & 1u)) return;   // wave-uniform: a kernel argument
    MemCheck sink{c.lane, inj_group == g ? inj_index : sm::kNoBad, sm::kNoBad};
    mem_group<g>(c, sink);
    if (sink.bad != sm::kNoBad) {
      atomicOr(&red[0], 1u << c.wave);
      atomicOr(&red[2], 1u << g);
      atomicMin(&red[3], sm::pack_bad(g, sink.bad, static_cast<uint32_t>(c.wave)));
    }
  };
  (one(std::integral_constant<int, G>{}), ...);
}

// One visit of one CU, on the grid and the stream of cu_sweep_kernel: all four waves (one per SIMD)
// run every selected group on the table, on their region of workgroup blockIdx.x's slice of
// `scratch` and on their region of the LDS array. One record per workgroup. It never writes EXEC;
// M0 is written only by the compiler, for LDS-DMA. No spin, no inter-workgroup traffic, every loop
// bounded by a constant; every branch around a group is wave-uniform.
__global__ __launch_bounds__(kSweepBlock) void cu_mem_kernel(const uint32_t* __restrict__ table, uint8_t* __restrict__ scratch,
                                                             uint32_t* __restrict__ out, MemInject inj, uint32_t groups) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kMemLdsDwords];
  uint32_t* red = lds + kMemRed;   // 0 fail, 1 simds, 2 groups, 3 first bad (pack_bad)
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(tid >> 6));
  uint32_t xcc, hwid;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
  const bool mine = inj.group >= 0 && xcc == static_cast<uint32_t>(inj.xcc) && st::hw_cu_key(hwid) == static_cast<uint32_t>(inj.cu_key) &&
                    (inj.index & 3) == wave;
  if (tid < 4) red[tid] = tid == 3 ? sm::kNoBad : 0u;
  __syncthreads();
  const MemCtx c = mem_ctx(table, scratch + static_cast<size_t>(blockIdx.x) * sm::kSliceBytes, lds, wave, static_cast<int>(lane));
  mem_groups_checked(MemGroups{}, c, groups, mine ? inj.group : -1, static_cast<uint32_t>(inj.index), red);
  if (lane == 0) atomicOr(&red[1], 1u << st::hw_simd(hwid));
  __syncthreads();
  if (tid == 0) {
    uint32_t* o = out + static_cast<size_t>(blockIdx.x) * sm::kMemRecordWords;
    const uint32_t b = red[3];
    o[0] = xcc;
    o[1] = hwid;
    o[2] = red[0];
    o[3] = red[1];
    o[4] = red[2];
    o[5] = b == sm::kNoBad ? sm::kNoBad : b >> 20;
    o[6] = b == sm::kNoBad ? sm::kNoBad : (b >> 2) & 0x3ffffu;
    o[7] = b == sm::kNoBad ? sm::kNoBad : b & 3u;
  }
}

// One workgroup of four waves, one group: every lane's raw result words at out[wave][k][lane]. It
// establishes on the device that the kernel's instructions give what the twin computes.
template <int G>
__global__ __launch_bounds__(kSweepBlock) void mem_lanes_kernel(const uint32_t* __restrict__ table, uint8_t* __restrict__ scratch,
                                                                uint32_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kMemLdsDwords];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const MemCtx c = mem_ctx(table, scratch, lds, wave, lane);
  MemKeep sink{out, sm::group_words(G), wave, lane};
  mem_group<G>(c, sink);
}

// HBM pattern test in hbm_copy's shape (256 threads, 4 x 16 B per thread in flight,
// non-temporal, one pass, scalar tail): hbm_fill only writes, hbm_verify only reads. One launch
// covers the n elements at dst / src, which are elements first.. of the buffer (st::launch_spans):
// the pattern and the reported element are the buffer's, first + i.
using u32x4 = __attribute__((ext_vector_type(4))) uint32_t;

__device__ __forceinline__ u32x4 pattern4(uint64_t i, uint32_t seed, uint32_t pass) {
  u32x4 p;
  p[0] = st::pattern_word(i, 0, seed, pass);
  p[1] = st::pattern_word(i, 1, seed, pass);
  p[2] = st::pattern_word(i, 2, seed, pass);
  p[3] = st::pattern_word(i, 3, seed, pass);
  return p;
}

__global__ __launch_bounds__(kCopyBlock) void hbm_fill(u32x4* __restrict__ dst, size_t n, uint64_t first,
                                                       uint32_t seed, uint32_t pass) {
  const size_t base = static_cast<size_t>(blockIdx.x) * (kCopyBlock * kCopyUnroll) + threadIdx.x;
  if (base + (kCopyUnroll - 1) * kCopyBlock < n) {
#pragma unroll
    for (int u = 0; u < kCopyUnroll; ++u)
      __builtin_nontemporal_store(pattern4(first + base + u * kCopyBlock, seed, pass), dst + base + u * kCopyBlock);
  } else {
    for (int u = 0; u < kCopyUnroll; ++u)
      if (base + u * kCopyBlock < n) dst[base + u * kCopyBlock] = pattern4(first + base + u * kCopyBlock, seed, pass);
  }
}

struct VerifyOut {
  unsigned long long errors;                 // mismatching 16-byte elements, all passes
  st::Mismatch slot[st::kMismatchSlots];     // the first ones to report, claimed through `errors`
};

__device__ __forceinline__ void verify_one(uint64_t i, u32x4 got, uint32_t seed, uint32_t pass, VerifyOut* o) {
  const u32x4 exp = pattern4(i, seed, pass);
  if (exp[0] == got[0] && exp[1] == got[1] && exp[2] == got[2] && exp[3] == got[3]) return;
  const unsigned long long e = atomicAdd(&o->errors, 1ull);   // 64 bit: cannot wrap or saturate
  if (e >= static_cast<unsigned long long>(st::kMismatchSlots)) return;
  uint32_t k = 3, ew = exp[3], gw = got[3];
  if (exp[2] != got[2]) k = 2, ew = exp[2], gw = got[2];
  if (exp[1] != got[1]) k = 1, ew = exp[1], gw = got[1];
  if (exp[0] != got[0]) k = 0, ew = exp[0], gw = got[0];
  st::Mismatch* m = &o->slot[e];
  m->element = i;
  m->expected = ew;
  m->got = gw;
  m->word = k;
  m->pad = 0;
}

__global__ __launch_bounds__(kCopyBlock) void hbm_verify(const u32x4* __restrict__ src, size_t n, uint64_t first,
                                                         uint32_t seed, uint32_t pass, VerifyOut* __restrict__ o) {
  const size_t base = static_cast<size_t>(blockIdx.x) * (kCopyBlock * kCopyUnroll) + threadIdx.x;
  if (base + (kCopyUnroll - 1) * kCopyBlock < n) {
    u32x4 v[kCopyUnroll];
#pragma unroll
    for (int u = 0; u < kCopyUnroll; ++u) v[u] = __builtin_nontemporal_load(src + base + u * kCopyBlock);
#pragma unroll
    for (int u = 0; u < kCopyUnroll; ++u) verify_one(first + base + u * kCopyBlock, v[u], seed, pass, o);
  } else {
    for (int u = 0; u < kCopyUnroll; ++u)
      if (base + u * kCopyBlock < n) verify_one(first + base + u * kCopyBlock, src[base + u * kCopyBlock], seed, pass, o);
  }
}

// ---------------------------------------------------------------------------- host helpers

uint16_t f32_to_bf16_bits(float f) {  // round to nearest even
  uint32_t u;
  std::memcpy(&u, &f, 4);
  if ((u & 0x7f800000u) == 0x7f800000u) return static_cast<uint16_t>(u >> 16);
  u += 0x7fffu + ((u >> 16) & 1u);
  return static_cast<uint16_t>(u >> 16);
}

template <class T>
struct DevBuf {
  T* p = nullptr;
  explicit DevBuf(size_t n) { HIP_OK(hipMalloc(&p, n * sizeof(T))); }
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
};

// mfma_burn: 4 chains a wave, 4 waves a block, 32768 FLOP an instruction.
double burn_tflops(int blocks, int iters, double ms) {
  return 4.0 * 32768.0 * iters * (static_cast<double>(blocks) * 4) / (ms * 1e-3) / 1e12;
}

// hbm_copy of n float4, `iters` times: read + write bytes.
double copy_gbs(size_t n, int iters, double ms) {
  return 2.0 * static_cast<double>(n * sizeof(float4)) * iters / (ms * 1e-3) / 1e9;
}

std::vector<float> gemm_tile(const std::vector<float>& a, const std::vector<float>& b) {
  if (a.size() != 32 * 16 || b.size() != 16 * 32) throw std::invalid_argument("gemm_tile: A is 32x16, B is 16x32");
  std::vector<uint16_t> ha(a.size()), hb(b.size());
  for (size_t i = 0; i < a.size(); ++i) ha[i] = f32_to_bf16_bits(a[i]);
  for (size_t i = 0; i < b.size(); ++i) hb[i] = f32_to_bf16_bits(b[i]);
  DevBuf<uint16_t> da(ha.size()), db(hb.size());
  DevBuf<float> dc(32 * 32);
  HIP_OK(hipMemcpy(da.p, ha.data(), ha.size() * 2, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(db.p, hb.data(), hb.size() * 2, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(mfma_tile, dim3(1), dim3(64), 0, 0, reinterpret_cast<const __bf16*>(da.p),
                     reinterpret_cast<const __bf16*>(db.p), dc.p);
  HIP_OK(hipGetLastError());
  std::vector<float> c(32 * 32);
  HIP_OK(hipMemcpy(c.data(), dc.p, c.size() * 4, hipMemcpyDeviceToHost));
  return c;
}

struct Stream {
  hipStream_t s = nullptr;
  explicit Stream(const std::vector<uint32_t>& mask) {
    if (mask.empty())
      HIP_OK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    else
      HIP_OK(hipExtStreamCreateWithCUMask(&s, static_cast<uint32_t>(mask.size()), mask.data()));
  }
  ~Stream() {
    if (s) (void)hipStreamDestroy(s);
  }
};

struct Events {
  hipEvent_t a = nullptr, b = nullptr;
  Events() {
    HIP_OK(hipEventCreate(&a));
    HIP_OK(hipEventCreate(&b));
  }
  ~Events() {
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
  }
  float ms() {
    HIP_OK(hipEventSynchronize(b));
    float t = 0.f;
    HIP_OK(hipEventElapsedTime(&t, a, b));
    return t;
  }
};

int cu_count(int dev) {
  int n = 0;
  HIP_OK(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
  return n;
}

py::dict device_props(int dev) {
  hipDeviceProp_t p;
  HIP_OK(hipGetDeviceProperties(&p, dev));
  py::dict d;
  d["name"] = std::string(p.name);
  d["gcn_arch"] = std::string(p.gcnArchName);
  d["cus"] = p.multiProcessorCount;
  d["total_mem_bytes"] = static_cast<uint64_t>(p.totalGlobalMem);
  d["l2_bytes"] = p.l2CacheSize;
  d["lds_per_block_bytes"] = static_cast<uint64_t>(p.sharedMemPerBlock);
  d["max_shared_per_cu_bytes"] = static_cast<uint64_t>(p.maxSharedMemoryPerMultiProcessor);
  d["warp_size"] = p.warpSize;
  d["clock_khz"] = p.clockRate;
  d["mem_clock_khz"] = p.memoryClockRate;
  d["mem_bus_width"] = p.memoryBusWidth;
  d["pci_bus"] = p.pciBusID;
  d["pci_device"] = p.pciDeviceID;
  d["pci_domain"] = p.pciDomainID;
  d["multi_gpu_board"] = p.isMultiGpuBoard;
  int count = 0;
  HIP_OK(hipGetDeviceCount(&count));
  d["device_count"] = count;
  return d;
}

// Test hook of copy_check and hbm_pattern_check: the buffer a kernel writes sits between two
// guard regions of `guard_bytes` each, filled with kGuardByte before the launch and read back
// after it. A multiple of 16 bytes, so the buffer keeps its 16-byte alignment.
constexpr unsigned char kGuardByte = 0xA5;
constexpr size_t kGuardMax = size_t(1) << 20;

void check_guard_bytes(size_t guard_bytes) {
  if (guard_bytes % 16 != 0 || guard_bytes > kGuardMax)
    throw std::invalid_argument("guard_bytes: a multiple of 16, at most 1 MiB");
}

// Guard bytes that no longer hold kGuardByte, in the regions before and after `bytes` at `base + guard`.
size_t guard_bytes_changed(const unsigned char* base, size_t guard, size_t bytes) {
  if (guard == 0) return 0;
  std::vector<unsigned char> g(2 * guard);
  HIP_OK(hipMemcpy(g.data(), base, guard, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(g.data() + guard, base + guard + bytes, guard, hipMemcpyDeviceToHost));
  return static_cast<size_t>(std::count_if(g.begin(), g.end(), [](unsigned char c) { return c != kGuardByte; }));
}

struct CopyCheck {
  bool ok = false;              // destination == source, bit for bit
  size_t guard_changed = 0;     // guard bytes the kernel overwrote
};

// The source holds integers below 1000003 as floats: the top byte of each is 0x00 or 0x3f..0x49,
// never kGuardByte, so no element of the source written over a guard leaves it unchanged.
CopyCheck copy_check(int dev, size_t n_floats, size_t guard_bytes) {
  HIP_OK(hipSetDevice(dev));
  check_guard_bytes(guard_bytes);
  const size_t n4 = (n_floats + 3) / 4;
  const dim3 grid(copy_grid(n4));
  std::vector<float> h(n4 * 4);
  for (size_t i = 0; i < h.size(); ++i) h[i] = static_cast<float>((i * 2654435761u) % 1000003u);
  DevBuf<float4> a(n4);
  DevBuf<unsigned char> b(n4 * 16 + 2 * guard_bytes);
  float4* dst = reinterpret_cast<float4*>(b.p + guard_bytes);
  HIP_OK(hipMemcpy(a.p, h.data(), n4 * 16, hipMemcpyHostToDevice));
  if (guard_bytes) HIP_OK(hipMemset(b.p, kGuardByte, n4 * 16 + 2 * guard_bytes));
  HIP_OK(hipMemset(dst, 0, n4 * 16));
  hipLaunchKernelGGL(hbm_copy, grid, dim3(kCopyBlock), 0, 0, a.p, dst, n4);
  HIP_OK(hipGetLastError());
  std::vector<float> out(n4 * 4);
  HIP_OK(hipMemcpy(out.data(), dst, n4 * 16, hipMemcpyDeviceToHost));
  CopyCheck res;
  res.ok = std::memcmp(out.data(), h.data(), n4 * 16) == 0;
  res.guard_changed = guard_bytes_changed(b.p, guard_bytes, n4 * 16);
  return res;
}

double hbm_bandwidth(int dev, size_t bytes, int iters) {
  HIP_OK(hipSetDevice(dev));
  const size_t n = bytes / sizeof(float4);
  if (n == 0 || iters <= 0) throw std::invalid_argument("hbm_bandwidth: bytes/iters must be positive");
  const dim3 grid(copy_grid(n));
  DevBuf<float4> a(n), b(n);
  HIP_OK(hipMemset(a.p, 0, n * sizeof(float4)));
  Stream st({});
  Events ev;
  hipLaunchKernelGGL(hbm_copy, grid, dim3(kCopyBlock), 0, st.s, a.p, b.p, n);  // warm-up
  HIP_OK(hipGetLastError());
  HIP_OK(hipEventRecord(ev.a, st.s));
  for (int i = 0; i < iters; ++i)
    hipLaunchKernelGGL(hbm_copy, grid, dim3(kCopyBlock), 0, st.s, a.p, b.p, n);
  HIP_OK(hipGetLastError());
  HIP_OK(hipEventRecord(ev.b, st.s));
  return copy_gbs(n, iters, ev.ms());
}

py::list census(int dev, const std::vector<uint32_t>& mask, int blocks, int sleep_iters) {
  HIP_OK(hipSetDevice(dev));
  if (blocks <= 0 || blocks > (1 << 20)) throw std::invalid_argument("census: bad block count");
  DevBuf<uint32_t> out(static_cast<size_t>(blocks) * 3);
  HIP_OK(hipMemset(out.p, 0xff, static_cast<size_t>(blocks) * 3 * sizeof(uint32_t)));
  Stream st(mask);
  hipLaunchKernelGGL(cu_census, dim3(blocks), dim3(64), 0, st.s, out.p, sleep_iters);
  HIP_OK(hipGetLastError());
  HIP_OK(hipStreamSynchronize(st.s));
  std::vector<uint32_t> h(static_cast<size_t>(blocks) * 3);
  HIP_OK(hipMemcpy(h.data(), out.p, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  py::list res;
  for (int i = 0; i < blocks; ++i) res.append(py::make_tuple(h[3 * i], h[3 * i + 1]));
  return res;
}

double mfma_ms(int dev, const std::vector<uint32_t>& mask, int blocks, int iters) {
  HIP_OK(hipSetDevice(dev));
  if (blocks <= 0 || iters <= 0) throw std::invalid_argument("mfma_throughput: bad shape");
  check_burn_blocks(blocks);
  DevBuf<float> out(static_cast<size_t>(blocks) * 256);
  Stream st(mask);
  Events ev;
  hipLaunchKernelGGL(mfma_burn, dim3(blocks), dim3(256), 0, st.s, out.p, 8);
  HIP_OK(hipGetLastError());
  HIP_OK(hipEventRecord(ev.a, st.s));
  hipLaunchKernelGGL(mfma_burn, dim3(blocks), dim3(256), 0, st.s, out.p, iters);
  HIP_OK(hipGetLastError());
  HIP_OK(hipEventRecord(ev.b, st.s));
  return ev.ms();
}

py::dict mfma_throughput(int dev, const std::vector<uint32_t>& mask, int blocks, int iters) {
  double ms = 0.0;
  {
    py::gil_scoped_release nogil;  // device work without the GIL; py objects built after
    ms = mfma_ms(dev, mask, blocks, iters);
  }
  py::dict d;
  d["ms"] = ms;
  d["tflops"] = burn_tflops(blocks, iters, ms);
  d["blocks"] = blocks;
  d["iters"] = iters;
  return d;
}

// Co-located tenants: one MFMA burn per CU mask, each on its own CU-masked stream, all
// launched back to back so they run concurrently. Returns per-tenant TFLOP/s, timed with
// each stream's own events: with disjoint XCD-symmetric masks every tenant must get
// throughput proportional to its CUs regardless of its neighbours (the agent's spatial
// share, nanogpu/agent/cumask.py).
std::vector<double> mfma_colocated(int dev, const std::vector<std::vector<uint32_t>>& masks,
                                   const std::vector<int>& blocks, int iters) {
  HIP_OK(hipSetDevice(dev));
  if (masks.empty() || masks.size() != blocks.size() || iters <= 0)
    throw std::invalid_argument("mfma_colocated: one block count per mask, iters > 0");
  const size_t n = masks.size();
  std::vector<std::unique_ptr<Stream>> streams;
  std::vector<std::unique_ptr<Events>> evs;
  std::vector<std::unique_ptr<DevBuf<float>>> outs;
  for (int b : blocks) check_burn_blocks(b);
  for (size_t i = 0; i < n; ++i) {
    streams.emplace_back(new Stream(masks[i]));
    evs.emplace_back(new Events());
    outs.emplace_back(new DevBuf<float>(static_cast<size_t>(blocks[i]) * 256));
    hipLaunchKernelGGL(mfma_burn, dim3(blocks[i]), dim3(256), 0, streams[i]->s, outs[i]->p, 8);  // warm-up
  }
  HIP_OK(hipGetLastError());
  HIP_OK(hipDeviceSynchronize());
  for (size_t i = 0; i < n; ++i) {
    HIP_OK(hipEventRecord(evs[i]->a, streams[i]->s));
    hipLaunchKernelGGL(mfma_burn, dim3(blocks[i]), dim3(256), 0, streams[i]->s, outs[i]->p, iters);
    HIP_OK(hipEventRecord(evs[i]->b, streams[i]->s));
  }
  HIP_OK(hipGetLastError());
  std::vector<double> tf(n);
  for (size_t i = 0; i < n; ++i) tf[i] = burn_tflops(blocks[i], iters, evs[i]->ms());
  return tf;
}

// Co-located streaming tenants: one HBM copy per CU mask, each on its own CU-masked stream,
// launched together. Returns per-tenant GB/s (read + write) over each tenant's own events.
// CU masks partition the compute units, not the memory system: this measures how the HBM3E
// bandwidth splits between memory-bound neighbours (profiles/gpu_calibration.md).
// `iters_each` (optional, one per mask) lets a neighbour outlast the tenant being measured.
std::vector<double> hbm_colocated(int dev, const std::vector<std::vector<uint32_t>>& masks, size_t bytes,
                                  int iters, std::vector<int> iters_each) {
  HIP_OK(hipSetDevice(dev));
  const size_t n = bytes / sizeof(float4);
  if (masks.empty() || n == 0 || iters <= 0) throw std::invalid_argument("hbm_colocated: masks, bytes, iters");
  const size_t k = masks.size();
  if (iters_each.empty()) iters_each.assign(k, iters);
  if (iters_each.size() != k) throw std::invalid_argument("hbm_colocated: one iteration count per mask");
  for (int it : iters_each)
    if (it <= 0 || it > 1000) throw std::invalid_argument("hbm_colocated: iterations in 1..1000");
  std::vector<std::unique_ptr<Stream>> streams;
  std::vector<std::unique_ptr<Events>> evs;
  std::vector<std::unique_ptr<DevBuf<float4>>> src, dst;
  const dim3 grid(copy_grid(n));
  for (size_t i = 0; i < k; ++i) {
    streams.emplace_back(new Stream(masks[i]));
    evs.emplace_back(new Events());
    src.emplace_back(new DevBuf<float4>(n));
    dst.emplace_back(new DevBuf<float4>(n));
    HIP_OK(hipMemset(src[i]->p, 0, n * sizeof(float4)));
    hipLaunchKernelGGL(hbm_copy, grid, dim3(kCopyBlock), 0, streams[i]->s, src[i]->p, dst[i]->p, n);  // warm-up
  }
  HIP_OK(hipGetLastError());
  HIP_OK(hipDeviceSynchronize());
  for (size_t i = 0; i < k; ++i) {
    HIP_OK(hipEventRecord(evs[i]->a, streams[i]->s));
    for (int it = 0; it < iters_each[i]; ++it)
      hipLaunchKernelGGL(hbm_copy, grid, dim3(kCopyBlock), 0, streams[i]->s, src[i]->p, dst[i]->p, n);
    HIP_OK(hipEventRecord(evs[i]->b, streams[i]->s));
  }
  HIP_OK(hipGetLastError());
  std::vector<double> gbs(k);
  for (size_t i = 0; i < k; ++i)
    gbs[i] = copy_gbs(n, iters_each[i], evs[i]->ms());
  return gbs;
}

// A streaming tenant next to a compute-bound one: an HBM copy on `hbm_mask` and an MFMA
// burn on `mfma_mask`, launched together on their own CU-masked streams. The burn is sized
// (`mfma_iters`) to outlast the copy, so the copy's rate is measured entirely beside it.
// Returns {copy GB/s, burn TFLOP/s}: what a memory-bound pod gets when the scheduler pairs
// it with a compute-bound neighbour (kFlagMemBound) instead of another streaming one.
std::vector<double> mixed_colocated(int dev, const std::vector<uint32_t>& hbm_mask,
                                    const std::vector<uint32_t>& mfma_mask, size_t bytes, int iters,
                                    int mfma_blocks, int mfma_iters) {
  HIP_OK(hipSetDevice(dev));
  const size_t n = bytes / sizeof(float4);
  if (n == 0 || iters <= 0 || mfma_blocks <= 0 || mfma_iters <= 0)
    throw std::invalid_argument("mixed_colocated: bytes, iters and the burn shape must be positive");
  const dim3 grid(copy_grid(n));
  check_burn_blocks(mfma_blocks);
  Stream sc(hbm_mask), sm(mfma_mask);
  Events ec, em;
  DevBuf<float4> src(n), dst(n);
  DevBuf<float> out(static_cast<size_t>(mfma_blocks) * 256);
  HIP_OK(hipMemset(src.p, 0, n * sizeof(float4)));
  hipLaunchKernelGGL(hbm_copy, grid, dim3(kCopyBlock), 0, sc.s, src.p, dst.p, n);    // warm-up
  hipLaunchKernelGGL(mfma_burn, dim3(mfma_blocks), dim3(256), 0, sm.s, out.p, 8);
  HIP_OK(hipGetLastError());
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipEventRecord(em.a, sm.s));
  hipLaunchKernelGGL(mfma_burn, dim3(mfma_blocks), dim3(256), 0, sm.s, out.p, mfma_iters);
  HIP_OK(hipEventRecord(em.b, sm.s));
  HIP_OK(hipEventRecord(ec.a, sc.s));
  for (int it = 0; it < iters; ++it)
    hipLaunchKernelGGL(hbm_copy, grid, dim3(kCopyBlock), 0, sc.s, src.p, dst.p, n);
  HIP_OK(hipEventRecord(ec.b, sc.s));
  HIP_OK(hipGetLastError());
  const double gbs = copy_gbs(n, iters, ec.ms());
  return {gbs, burn_tflops(mfma_blocks, mfma_iters, em.ms())};
}

struct PeerRate {
  double pull_gbs;   // copy kernel on `dst` reading `src`'s HBM over xGMI (one link, one direction)
  double dma_gbs;    // hipMemcpyPeerAsync (SDMA engines) over the same link
  bool peer_access;
};

// A peer transfer that did not finish by its deadline (a wedged link or peer). Its stream,
// events and buffers are abandoned, never freed: hipFree / hipStreamDestroy would wait on the
// work that never completes.
struct PeerTimeout : std::runtime_error {
  using std::runtime_error::runtime_error;
};

using Clock = std::chrono::steady_clock;

// Polls `e` until it completes (true) or `deadline` passes (false); never blocks in the runtime.
bool wait_event(hipEvent_t e, Clock::time_point deadline) {
  for (;;) {
    const hipError_t q = hipEventQuery(e);
    if (q == hipSuccess) return true;
    if (q != hipErrorNotReady) HIP_OK(q);
    if (Clock::now() > deadline) return false;
    std::this_thread::sleep_for(std::chrono::microseconds(200));
  }
}

// Per-pair link rate for the topology scorer. The copy kernel runs on the destination GPU and
// loads straight from the peer's memory (peer access enabled), so every byte crosses the one
// xGMI link between the pair in one direction; its grid (n / 4096 WGs, >> 256 CUs) keeps
// enough loads in flight to saturate the link rather than one SDMA engine. Every wait polls an
// event against `deadline_s` (from the call): a transfer that never completes throws
// PeerTimeout instead of blocking the rank (and, through the next collective, the whole job).
PeerRate peer_bandwidth(int src, int dst, size_t bytes, int iters, double deadline_s) {
  int n_dev = 0;
  HIP_OK(hipGetDeviceCount(&n_dev));
  if (src < 0 || dst < 0 || src >= n_dev || dst >= n_dev || src == dst)
    throw std::invalid_argument("peer_bandwidth: need two distinct visible devices");
  const size_t n = bytes / sizeof(float4);
  if (n == 0 || iters <= 0) throw std::invalid_argument("peer_bandwidth: bytes/iters must be positive");
  const dim3 grid(copy_grid(n));
  const Clock::time_point deadline =
      Clock::now() + std::chrono::microseconds(static_cast<int64_t>((deadline_s > 0 ? deadline_s : 30.0) * 1e6));
  PeerRate r{0.0, 0.0, false};
  int prev = 0;   // the caller's current device comes back on return (torch tracks it)
  HIP_OK(hipGetDevice(&prev));
  struct Restore {
    int d;
    ~Restore() { (void)hipSetDevice(d); }
  } restore{prev};
  int can = 0;
  HIP_OK(hipDeviceCanAccessPeer(&can, dst, src));
  HIP_OK(hipSetDevice(dst));
  if (can) {
    hipError_t e = hipDeviceEnablePeerAccess(src, 0);
    if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) HIP_OK(e);
    (void)hipGetLastError();
    r.peer_access = true;
  }
  // owned until a timeout abandons them
  hipStream_t ss = nullptr, st = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  float4 *a = nullptr, *b = nullptr;
  bool abandoned = false;
  auto cleanup = [&] {
    if (abandoned) return;
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (ss) (void)hipStreamDestroy(ss);
    if (st) (void)hipStreamDestroy(st);
    if (a) (void)hipFree(a);
    if (b) (void)hipFree(b);
  };
  auto timed = [&](const char* what, auto&& enqueue) -> double {   // seconds of `enqueue`'s work
    HIP_OK(hipEventRecord(e0, st));
    enqueue();
    HIP_OK(hipEventRecord(e1, st));
    if (!wait_event(e1, deadline)) {
      abandoned = true;
      throw PeerTimeout(std::string("peer_bandwidth ") + std::to_string(src) + "->" + std::to_string(dst) + ": " +
                        what + " did not finish within " + std::to_string(deadline_s) + " s");
    }
    float ms = 0.f;
    HIP_OK(hipEventElapsedTime(&ms, e0, e1));
    return ms * 1e-3;
  };
  try {
    HIP_OK(hipSetDevice(src));
    HIP_OK(hipMalloc(&a, n * sizeof(float4)));
    HIP_OK(hipStreamCreateWithFlags(&ss, hipStreamNonBlocking));
    HIP_OK(hipMemsetAsync(a, 0, n * sizeof(float4), ss));
    hipEvent_t fill = nullptr;
    HIP_OK(hipEventCreateWithFlags(&fill, hipEventDisableTiming));
    HIP_OK(hipEventRecord(fill, ss));
    const bool filled = wait_event(fill, deadline);
    (void)hipEventDestroy(fill);
    if (!filled) {
      abandoned = true;
      throw PeerTimeout("peer_bandwidth: the source fill on GPU " + std::to_string(src) + " did not finish");
    }
    HIP_OK(hipSetDevice(dst));
    HIP_OK(hipMalloc(&b, n * sizeof(float4)));
    HIP_OK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    HIP_OK(hipEventCreate(&e0));
    HIP_OK(hipEventCreate(&e1));
    const double nb = static_cast<double>(n * sizeof(float4));
    timed("SDMA warm-up", [&] { HIP_OK(hipMemcpyPeerAsync(b, dst, a, src, n * sizeof(float4), st)); });
    r.dma_gbs = nb * iters / timed("SDMA copies", [&] {
      for (int i = 0; i < iters; ++i) HIP_OK(hipMemcpyPeerAsync(b, dst, a, src, n * sizeof(float4), st));
    }) / 1e9;
    if (r.peer_access) {
      timed("pull warm-up", [&] {
        hipLaunchKernelGGL(hbm_copy, grid, dim3(kCopyBlock), 0, st, a, b, n);
        HIP_OK(hipGetLastError());
      });
      r.pull_gbs = nb * iters / timed("pull copies", [&] {
        for (int i = 0; i < iters; ++i) hipLaunchKernelGGL(hbm_copy, grid, dim3(kCopyBlock), 0, st, a, b, n);
        HIP_OK(hipGetLastError());
      }) / 1e9;
    }
  } catch (...) {
    cleanup();
    throw;
  }
  cleanup();
  return r;
}

// ---------------------------------------------------------------------------- deep self-test (host)

// The names behind the bits of a sweep's selection: the matrix paths, the vector-ALU groups.
struct NameTable {
  int count;
  const char* (*name)(int);
  const char* noun;

  int index(const std::string& n) const {
    for (int i = 0; i < count; ++i)
      if (n == name(i)) return i;
    throw std::invalid_argument(std::string("unknown ") + noun + " '" + n + "'");
  }
  uint32_t bits(const std::vector<std::string>& names) const {
    uint32_t b = 0;
    for (const std::string& n : names) b |= 1u << index(n);
    return b;
  }
  std::pair<py::list, py::list> names_and_checked(uint32_t bits) const {   // every name in bit order; those of `bits`
    py::list all, checked;
    for (int i = 0; i < count; ++i) {
      all.append(name(i));
      if (bits >> i & 1u) checked.append(name(i));
    }
    return {all, checked};
  }
};
constexpr NameTable kPathNames{sp::kNumPaths, sp::path_name, "matrix path"};
constexpr NameTable kValuNames{sv::kNumNames, sv::group_name, "vector-ALU group"};
constexpr NameTable kScalarNames{ss::kNumNames, ss::group_name, "scalar group"};
constexpr NameTable kMemNames{sm::kNumNames, sm::group_name, "memory group"};

// Test hook: a device copy of `count` host words of which one at a time is XORed. flip() first
// puts the word flipped before back as the host has it; the host array is never written. The
// stream is idle between runs (CuSession::run synchronises), so plain copies are ordered with it.
class FlippableUpload {
 public:
  FlippableUpload(const uint32_t* host, size_t count) : host_(host), dev_(count) {
    HIP_OK(hipMemcpy(dev_.p, host, count * sizeof(uint32_t), hipMemcpyHostToDevice));
  }
  const uint32_t* p() const { return dev_.p; }
  void flip(std::optional<size_t> at, uint32_t mask) {
    if (flipped_) write(*flipped_, 0u);
    flipped_ = at;
    if (at) write(*at, mask);
  }

 private:
  void write(size_t at, uint32_t mask) {
    const uint32_t w = host_[at] ^ mask;
    HIP_OK(hipMemcpy(dev_.p + at, &w, 4, hipMemcpyHostToDevice));
  }
  const uint32_t* host_;
  DevBuf<uint32_t> dev_;
  std::optional<size_t> flipped_;
};

// corrupt_expected as a session takes it: word `word` of table `table` XORed with `mask`; -1: none.
// The sweep's tables are 0 (the bf16 chain's tile) and 1 + p (path p's tile); the vector-ALU
// sweep's are its exact groups; the scalar sweep's are its exact groups and, as table ss::kSmem, the load table.
struct WordFlip {
  int table = -1;
  uint32_t word = 0, mask = 0;
};

struct CuRun {
  std::vector<uint32_t> words;   // record_words per workgroup
  int record_words = 0, blocks = 0;
  double ms = 0.0;
};

// What every per-CU check shares: rounds x (enabled CUs) workgroups on a stream masked to `mask`,
// 0xff-filled records of which every workgroup must write its own, and a first launch outside the
// timed span. `who` begins the messages. A session derived from this holds its kernel's inputs,
// which are destroyed before the stream they were used on; `launch(blocks)` is its kernel's launch.
class CuSession {
 protected:
  CuSession(const char* who, int dev, const std::vector<uint32_t>& mask, int rounds, int record_words)
      : who_(who), stream_(mask), blocks_(grid(who_, dev, mask, rounds)), record_words_(record_words),
        out_(static_cast<size_t>(blocks_) * record_words) {}

  template <class Launch>
  void warm_up(Launch&& launch) {   // loads the code object
    launch(1);
    HIP_OK(hipStreamSynchronize(stream_.s));
  }

  template <class Launch>
  CuRun run(Launch&& launch) {
    CuRun res;
    res.blocks = blocks_;
    res.record_words = record_words_;
    const size_t words = static_cast<size_t>(blocks_) * record_words_;
    HIP_OK(hipMemsetAsync(out_.p, 0xff, words * sizeof(uint32_t), stream_.s));
    HIP_OK(hipEventRecord(ev_.a, stream_.s));
    launch(blocks_);
    HIP_OK(hipEventRecord(ev_.b, stream_.s));
    res.ms = ev_.ms();
    HIP_OK(hipStreamSynchronize(stream_.s));
    res.words.resize(words);
    HIP_OK(hipMemcpy(res.words.data(), out_.p, words * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (int b = 0; b < blocks_; ++b)
      if (!st::record_written(res.words.data() + static_cast<size_t>(b) * record_words_))
        throw std::runtime_error(who_ + ": workgroup " + std::to_string(b) + " left no record");
    return res;
  }

  hipStream_t stream() const { return stream_.s; }
  uint32_t* out() const { return out_.p; }
  int blocks() const { return blocks_; }

 private:
  static int grid(const std::string& who, int dev, const std::vector<uint32_t>& mask, int rounds) {
    if (rounds < 1 || rounds > 64) throw std::invalid_argument(who + ": rounds in 1..64");
    int cus = 0;
    if (mask.empty())
      cus = cu_count(dev);
    else
      for (uint32_t w : mask) cus += __builtin_popcount(w);
    if (cus <= 0 || cus > 4096) throw std::invalid_argument(who + ": the mask enables no CU");
    return rounds * cus;
  }

  std::string who_;
  Stream stream_;
  Events ev_;
  int blocks_, record_words_;
  DevBuf<uint32_t> out_;
};

// Test hook behind tests/test_gpu_selftest_sensitivity.py and test_gpu_selftest_valu.py: for every
// flip one run of `session` with `set_flip(flip)` applied. `fields(run, b)` picks N words of record
// b; per flip the AND of each over all records, then the OR of each: 2N words.
struct Sensitivity {
  std::vector<uint32_t> fields;
  int records = 0;                // per sweep
  double seconds = 0.0;           // wall time of the loop
};

template <size_t N, class Session, class Flip, class SetFlip, class Fields>
Sensitivity sensitivity(Session& session, uint32_t seed, const std::vector<Flip>& flips, SetFlip&& set_flip, Fields&& fields) {
  Sensitivity out;
  out.fields.reserve(flips.size() * 2 * N);
  const Clock::time_point t0 = Clock::now();
  for (const Flip& f : flips) {
    set_flip(f);
    const CuRun r = session.run(seed, {});
    out.records = r.blocks;
    std::array<uint32_t, N> a, o;
    a.fill(~0u);
    o.fill(0u);
    for (int b = 0; b < r.blocks; ++b) {
      const std::array<uint32_t, N> v = fields(r, b);
      for (size_t i = 0; i < N; ++i) a[i] &= v[i], o[i] |= v[i];
    }
    out.fields.insert(out.fields.end(), a.begin(), a.end());
    out.fields.insert(out.fields.end(), o.begin(), o.end());
  }
  out.seconds = std::chrono::duration<double>(Clock::now() - t0).count();
  return out;
}

const std::vector<uint32_t>& path_tiles() {   // independent of seed and device: computed once
  static const std::vector<uint32_t> tiles = [] {
    std::vector<uint32_t> t(static_cast<size_t>(sp::kNumPaths) * sp::kTileWords);
    for (int p = 0; p < sp::kNumPaths; ++p) {
      const sp::PathTile tile = sp::path_expected(p);
      if (!tile.exact()) throw std::logic_error(std::string("path ") + sp::path_name(p) + ": the chain is not exact");
      sp::path_expected_words(p, tile, t.data() + static_cast<size_t>(p) * sp::kTileWords);
    }
    return t;
  }();
  return tiles;
}

using SweepKernel = void (*)(const float*, uint32_t*, uint32_t, SweepInject, uint32_t, uint32_t, const uint32_t*);
constexpr SweepKernel kSweepKernels[2][2] = {   // [kPaths][kFull]
    {cu_sweep_kernel<false, false>, cu_sweep_kernel<false, true>},
    {cu_sweep_kernel<true, false>, cu_sweep_kernel<true, true>}};

bool sweep_block_fits(SweepKernel kernel, size_t dynamic_lds) {
  int fit = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&fit, kernel, kSweepBlock, dynamic_lds) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return fit >= 1;
}

// The CuSession of cu_sweep_kernel. Whether one block may hold the whole LDS is asked of the
// occupancy API, never found out by a failing launch. `paths` != 0 launches the kPaths
// instantiations instead (same grid, block and LDS), with every path's expected tile uploaded
// once, and returns their 7-word records. `lds_bytes` (test hook) takes the dynamic-LDS
// instantiation with that much LDS whatever the device allows. cu_sweep is one session and one
// run, sweep_sensitivity a run per word.
class SweepSession : public CuSession {
 public:
  SweepSession(int dev, const std::vector<uint32_t>& mask, int rounds, uint32_t paths,
               std::optional<size_t> lds_bytes = std::nullopt)
      : CuSession("cu_sweep", dev, mask, rounds, paths ? sp::kPathRecordWords : st::kSweepRecordWords), paths_(paths) {
    if (paths & ~sp::kAllPaths) throw std::invalid_argument("cu_sweep_paths: unknown path bit");
    const uint32_t n_min = paths ? static_cast<uint32_t>(sp::kNumPaths * sp::kTileWords) : 4u;   // staging | reduction
    if (lds_bytes && (*lds_bytes % 16 != 0 || *lds_bytes > 65536 || *lds_bytes < n_min * 4u))
      throw std::invalid_argument("cu_sweep: lds_bytes is a multiple of 16, " + std::to_string(n_min * 4u) + "..65536");
    kernel_ = kSweepKernels[paths != 0][1];
    if (lds_bytes || !sweep_block_fits(kernel_, 0)) {
      kernel_ = kSweepKernels[paths != 0][0];
      if (lds_bytes) {
        n_ = static_cast<uint32_t>(*lds_bytes / 4);
      } else {
        hipDeviceProp_t p;
        HIP_OK(hipGetDeviceProperties(&p, dev));
        n_ = static_cast<uint32_t>(std::min<size_t>(p.sharedMemPerBlock, kLdsDwordsFull * 4u) / 4);
      }
      dynamic_lds_ = n_ * 4u;
      if (n_ < n_min || !sweep_block_fits(kernel_, dynamic_lds_))
        throw std::runtime_error("cu_sweep: no sweep workgroup fits a CU of this device");
    }

    std::vector<int32_t> tile(32 * 32);
    st::sweep_expected(tile.data());
    expected_host_.resize(tile.size());
    for (size_t i = 0; i < tile.size(); ++i) {   // the kernel reads floats: their words
      const float f = static_cast<float>(tile[i]);
      std::memcpy(&expected_host_[i], &f, 4);
    }
    expected_.emplace(expected_host_.data(), expected_host_.size());
    if (paths) tiles_.emplace(path_tiles().data(), path_tiles().size());
    warm_up([this](int blocks) { launch(blocks, 0u, SweepInject{}); });
  }

  void set_flip(const WordFlip& f) {
    expected_->flip(std::nullopt, 0u);   // both uploads clean before the checks: a refused flip leaves none behind
    if (tiles_) tiles_->flip(std::nullopt, 0u);
    if (f.table < 0) return;
    if (f.table > sp::kNumPaths) throw std::invalid_argument("corrupt_expected: unknown tile");
    if (f.table > 0 && !(paths_ >> (f.table - 1) & 1u))
      throw std::invalid_argument(std::string("corrupt_expected: path ") + sp::path_name(f.table - 1) + " is not selected");
    const uint32_t words = f.table == 0 ? 32u * 32u : static_cast<uint32_t>(sp::path_tile_words(f.table - 1));
    if (f.word >= words) throw std::invalid_argument("corrupt_expected: word beyond the tile");
    if (f.table == 0)
      expected_->flip(f.word, f.mask);
    else
      tiles_->flip(static_cast<size_t>(f.table - 1) * sp::kTileWords + f.word, f.mask);
  }

  CuRun run(uint32_t seed, SweepInject inj) {
    if (inj.kind == kInjectLds && inj.lds_off >= n_) throw std::invalid_argument("cu_sweep: inject offset beyond the LDS array");
    return CuSession::run([&](int blocks) { launch(blocks, seed, inj); });
  }

  size_t lds_bytes() const { return static_cast<size_t>(n_) * 4; }

 private:
  void launch(int blocks, uint32_t seed, SweepInject j) {
    hipLaunchKernelGGL(kernel_, dim3(blocks), dim3(kSweepBlock), dynamic_lds_, stream(), reinterpret_cast<const float*>(expected_->p()),
                       out(), seed, j, n_, paths_, tiles_ ? tiles_->p() : nullptr);
    HIP_OK(hipGetLastError());
  }

  uint32_t paths_;
  SweepKernel kernel_ = nullptr;
  uint32_t n_ = kLdsDwordsFull, dynamic_lds_ = 0;   // dwords the LDS test covers; bytes of them the launch asks for
  std::vector<uint32_t> expected_host_;
  std::optional<FlippableUpload> expected_, tiles_;   // tiles_: the path sweep only
};

// ---- vector-ALU sweep (host) ----

const std::vector<uint32_t>& valu_table() {   // the expected words, then the approx ranges: computed once
  static const std::vector<uint32_t> table = [] {
    std::vector<uint32_t> t = sv::expected_table();
    const std::vector<uint32_t> r = sv::approx_ranges();
    t.insert(t.end(), r.begin(), r.end());
    return t;
  }();
  return table;
}

// The CuSession of cu_valu_kernel. The kernel's attributes are read once: a register test that
// spills to scratch would test memory, so `regs` is refused then.
class ValuSession : public CuSession {
 public:
  ValuSession(int dev, const std::vector<uint32_t>& mask, int rounds, uint32_t groups)
      : CuSession("cu_sweep_valu", dev, mask, rounds, sv::kValuRecordWords), groups_(groups) {
    if (!groups || (groups & ~sv::kAllGroups)) throw std::invalid_argument("cu_sweep_valu: no group, or an unknown one");
    hipFuncAttributes attr;
    HIP_OK(hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(cu_valu_kernel)));
    scratch_bytes_ = attr.localSizeBytes;
    regs_per_lane_ = attr.numRegs;
    if ((groups >> sv::kRegs & 1u) && scratch_bytes_ != 0)
      throw std::runtime_error("cu_sweep_valu: the register-file test was compiled with " + std::to_string(scratch_bytes_) +
                               " bytes of scratch a lane, so it would test memory, not registers: 'regs' is refused");
    table_.emplace(valu_table().data(), valu_table().size());
    warm_up([this](int blocks) { launch(blocks, 0u, ValuInject{}); });
  }

  void set_flip(const WordFlip& f) {
    table_->flip(std::nullopt, 0u);
    if (f.table < 0) return;
    if (f.table >= sv::kNumExact) throw std::invalid_argument("corrupt_expected: an exact group's name");
    if (!(groups_ >> f.table & 1u)) throw std::invalid_argument(std::string("corrupt_expected: group ") + sv::group_name(f.table) + " is not selected");
    if (f.word >= static_cast<uint32_t>(sv::kGroupWords)) throw std::invalid_argument("corrupt_expected: word beyond the group's table");
    table_->flip(static_cast<size_t>(f.table) * sv::kGroupWords + f.word, f.mask);
  }

  CuRun run(uint32_t seed, ValuInject inj) {
    return CuSession::run([&](int blocks) { launch(blocks, seed, inj); });
  }

  size_t scratch_bytes() const { return scratch_bytes_; }
  int regs_per_lane() const { return regs_per_lane_; }

 private:
  void launch(int blocks, uint32_t seed, ValuInject j) {
    hipLaunchKernelGGL(cu_valu_kernel, dim3(blocks), dim3(kSweepBlock), 0, stream(), table_->p(), out(), seed, j, groups_);
    HIP_OK(hipGetLastError());
  }

  uint32_t groups_;
  int regs_per_lane_ = 0;
  size_t scratch_bytes_ = 0;
  std::optional<FlippableUpload> table_;
};

using LanesKernel = void (*)(uint32_t*);
template <int... G>
LanesKernel lanes_kernel(std::integer_sequence<int, G...>, int g) {
  static constexpr LanesKernel table[] = {valu_lanes_kernel<G>...};
  return table[g];
}

// Group g (an exact group or approx) on one wave: its raw words.
std::vector<uint32_t> valu_lanes(int g) {
  if (g < 0 || g > sv::kApprox) throw std::invalid_argument("valu_lanes: an exact group or 'approx'");
  const size_t n = g == sv::kApprox ? sv::kNumApprox * sv::kLanes : sv::kGroupWords;
  DevBuf<uint32_t> d(n);
  HIP_OK(hipMemset(d.p, 0, n * 4));
  hipLaunchKernelGGL(lanes_kernel(std::make_integer_sequence<int, sv::kApprox + 1>{}, g), dim3(1), dim3(64), 0, 0, d.p);
  HIP_OK(hipGetLastError());
  std::vector<uint32_t> h(n);
  HIP_OK(hipMemcpy(h.data(), d.p, n * 4, hipMemcpyDeviceToHost));
  return h;
}

// inject of cu_sweep_valu: (xcc, cu_key, 'valu', group) | (xcc, cu_key, 'regs', slot) | (xcc, cu_key, 'approx').
ValuInject parse_valu_inject(const py::object& inject) {
  ValuInject inj;
  if (inject.is_none()) return inj;
  const py::tuple t = inject.cast<py::tuple>();
  if (t.size() < 3 || t.size() > 4) throw std::invalid_argument("cu_sweep_valu: inject = (xcc, cu_key, kind[, arg])");
  inj.xcc = t[0].cast<int>();
  inj.cu_key = t[1].cast<int>();
  const std::string kind = t[2].cast<std::string>();
  if (kind == "valu" && t.size() == 4) {
    inj.kind = kValuInjectGroup;
    inj.arg = kValuNames.index(t[3].cast<std::string>());
    if (inj.arg >= sv::kNumExact) throw std::invalid_argument("cu_sweep_valu: inject 'valu' names an exact group");
  } else if (kind == "regs" && t.size() == 4) {
    inj.kind = kValuInjectRegs;
    inj.arg = t[3].cast<int>();
    if (inj.arg < 0 || inj.arg >= sv::kRegSlots) throw std::invalid_argument("cu_sweep_valu: inject slot beyond reg_slots");
  } else if (kind == "approx" && t.size() == 3) {
    inj.kind = kValuInjectApprox;
  } else {
    throw std::invalid_argument("cu_sweep_valu: inject kind is ('valu', group), ('regs', slot) or 'approx'");
  }
  return inj;
}

// ---- scalar sweep (host) ----

const std::vector<uint32_t>& scalar_table() {   // computed once
  static const std::vector<uint32_t> table = ss::expected_table();
  return table;
}
const std::vector<uint32_t>& scalar_loads() {
  static const std::vector<uint32_t> table = ss::smem_table();
  return table;
}

// The CuSession of cu_scalar_kernel. The kernel's attributes are read once: `sregs` names its
// registers, so no slot can have been spilled, but a kernel that reports scratch is refused that
// part all the same, as ValuSession refuses `regs`.
class ScalarSession : public CuSession {
 public:
  ScalarSession(int dev, const std::vector<uint32_t>& mask, int rounds, uint32_t groups)
      : CuSession("cu_sweep_scalar", dev, mask, rounds, ss::kScalarRecordWords), groups_(groups) {
    if (!groups || (groups & ~ss::kAllGroups)) throw std::invalid_argument("cu_sweep_scalar: no group, or an unknown one");
    hipFuncAttributes attr;
    HIP_OK(hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(cu_scalar_kernel)));
    scratch_bytes_ = attr.localSizeBytes;
    num_regs_ = attr.numRegs;
    if ((groups >> ss::kSregs & 1u) && scratch_bytes_ != 0)
      throw std::runtime_error("cu_sweep_scalar: the kernel was compiled with " + std::to_string(scratch_bytes_) +
                               " bytes of scratch a lane: 'sregs' is refused");
    int fit = 0;
    HIP_OK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&fit, cu_scalar_kernel, kSweepBlock, 0));
    if (fit < 1) throw std::runtime_error("cu_sweep_scalar: no scalar workgroup fits a CU of this device");
    table_.emplace(scalar_table().data(), scalar_table().size());
    loads_.emplace(scalar_loads().data(), scalar_loads().size());
    warm_up([this](int blocks) { launch(blocks, 0u, ScalarInject{}); });
  }

  void set_flip(const WordFlip& f) {
    table_->flip(std::nullopt, 0u);
    loads_->flip(std::nullopt, 0u);
    if (f.table < 0) return;
    if (f.table > ss::kSmem) throw std::invalid_argument("corrupt_expected: an exact group's name, or 'smem'");
    if (!(groups_ >> f.table & 1u)) throw std::invalid_argument(std::string("corrupt_expected: group ") + ss::group_name(f.table) + " is not selected");
    if (f.word >= static_cast<uint32_t>(f.table == ss::kSmem ? ss::kSmemWords : ss::kGroupWords))
      throw std::invalid_argument("corrupt_expected: word beyond the table");
    if (f.table == ss::kSmem)
      loads_->flip(f.word, f.mask);
    else
      table_->flip(static_cast<size_t>(f.table) * ss::kGroupWords + f.word, f.mask);
  }

  CuRun run(uint32_t seed, ScalarInject inj) {
    return CuSession::run([&](int blocks) { launch(blocks, seed, inj); });
  }

  size_t scratch_bytes() const { return scratch_bytes_; }
  int num_regs() const { return num_regs_; }

 private:
  void launch(int blocks, uint32_t seed, ScalarInject j) {
    hipLaunchKernelGGL(cu_scalar_kernel, dim3(blocks), dim3(kSweepBlock), 0, stream(), table_->p(), loads_->p(), out(), seed, j, groups_);
    HIP_OK(hipGetLastError());
  }

  uint32_t groups_;
  int num_regs_ = 0;
  size_t scratch_bytes_ = 0;
  std::optional<FlippableUpload> table_, loads_;
};

template <int... G>
LanesKernel scalar_words_kernel_of(std::integer_sequence<int, G...>, int g) {
  static constexpr LanesKernel table[] = {scalar_words_kernel<G>...};
  return table[g];
}

// Exact group g on one workgroup of four waves: its raw words [wave][word].
std::vector<uint32_t> scalar_words(int g) {
  if (g < 0 || g >= ss::kNumExact) throw std::invalid_argument("scalar_words: an exact group");
  DevBuf<uint32_t> d(ss::kGroupWords);
  HIP_OK(hipMemset(d.p, 0, ss::kGroupWords * 4));
  hipLaunchKernelGGL(scalar_words_kernel_of(ScalarExact{}, g), dim3(1), dim3(kSweepBlock), 0, 0, d.p);
  HIP_OK(hipGetLastError());
  std::vector<uint32_t> h(ss::kGroupWords);
  HIP_OK(hipMemcpy(h.data(), d.p, ss::kGroupWords * 4, hipMemcpyDeviceToHost));
  return h;
}

// inject of cu_sweep_scalar: (xcc, cu_key, 'scalar', group) | (xcc, cu_key, 'smem', word) | (xcc, cu_key, 'sregs', slot).
ScalarInject parse_scalar_inject(const py::object& inject) {
  ScalarInject inj;
  if (inject.is_none()) return inj;
  const py::tuple t = inject.cast<py::tuple>();
  if (t.size() != 4) throw std::invalid_argument("cu_sweep_scalar: inject = (xcc, cu_key, kind, arg)");
  inj.xcc = t[0].cast<int>();
  inj.cu_key = t[1].cast<int>();
  const std::string kind = t[2].cast<std::string>();
  if (kind == "scalar") {
    inj.kind = kScalarInjectGroup;
    inj.arg = kScalarNames.index(t[3].cast<std::string>());
    if (inj.arg >= ss::kNumExact) throw std::invalid_argument("cu_sweep_scalar: inject 'scalar' names an exact group");
  } else if (kind == "smem" || kind == "sregs") {
    inj.kind = kind == "smem" ? kScalarInjectSmem : kScalarInjectSregs;
    inj.arg = t[3].cast<int>();
    if (inj.arg < 0 || inj.arg >= (kind == "smem" ? ss::kSmemWords : ss::kSregSlots))
      throw std::invalid_argument("cu_sweep_scalar: inject word beyond the table, or slot beyond sreg_slots");
  } else {
    throw std::invalid_argument("cu_sweep_scalar: inject kind is ('scalar', group), ('smem', word) or ('sregs', slot)");
  }
  return inj;
}

const std::vector<uint32_t>& mem_table_words() {
  static const std::vector<uint32_t> table = sm::mem_table();
  return table;
}

// The CuSession of cu_mem_kernel: the table, and one slice of scratch memory per workgroup of the grid.
class MemSession : public CuSession {
 public:
  MemSession(int dev, const std::vector<uint32_t>& mask, int rounds, uint32_t groups)
      : CuSession("cu_sweep_mem", dev, mask, rounds, sm::kMemRecordWords), groups_(groups),
        scratch_(static_cast<size_t>(blocks()) * sm::kSliceBytes) {
    if (!groups || (groups & ~sm::kAllGroups)) throw std::invalid_argument("cu_sweep_mem: no group, or an unknown one");
    hipFuncAttributes attr;
    HIP_OK(hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(cu_mem_kernel)));
    scratch_bytes_ = attr.localSizeBytes;
    num_regs_ = attr.numRegs;
    int fit = 0;
    HIP_OK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&fit, cu_mem_kernel, kSweepBlock, 0));
    if (fit < 1) throw std::runtime_error("cu_sweep_mem: no memory workgroup fits a CU of this device");
    table_.emplace(mem_table_words().data(), mem_table_words().size());
    warm_up([this](int blocks) { launch(blocks, MemInject{}); });
  }

  void set_flip(const WordFlip& f) {
    table_->flip(std::nullopt, 0u);
    if (f.table < 0) return;
    if (!(sm::kTableGroups >> f.table & 1u)) throw std::invalid_argument("corrupt_expected: a group that reads the table: gload, l1 or ldsdma");
    if (!(groups_ >> f.table & 1u)) throw std::invalid_argument(std::string("corrupt_expected: group ") + sm::group_name(f.table) + " is not selected");
    if (f.word >= static_cast<uint32_t>(sm::kTableWords)) throw std::invalid_argument("corrupt_expected: word beyond the table");
    table_->flip(f.word, f.mask);
  }

  CuRun run(uint32_t /*seed: the part's data are fixed*/, MemInject inj) {
    return CuSession::run([&](int blocks) { launch(blocks, inj); });
  }

  size_t scratch_bytes() const { return scratch_bytes_; }
  int num_regs() const { return num_regs_; }

 private:
  void launch(int blocks, MemInject j) {
    hipLaunchKernelGGL(cu_mem_kernel, dim3(blocks), dim3(kSweepBlock), 0, stream(), table_->p(), scratch_.p, out(), j, groups_);
    HIP_OK(hipGetLastError());
  }

  uint32_t groups_;
  int num_regs_ = 0;
  size_t scratch_bytes_ = 0;
  DevBuf<uint8_t> scratch_;
  std::optional<FlippableUpload> table_;
};

using MemLanesKernel = void (*)(const uint32_t*, uint8_t*, uint32_t*);
template <int... G>
MemLanesKernel mem_lanes_kernel_of(std::integer_sequence<int, G...>, int g) {
  static constexpr MemLanesKernel table[] = {mem_lanes_kernel<G>...};
  return table[g];
}

// Group g on one workgroup of four waves: every lane's raw result words [wave][k][lane].
std::vector<uint32_t> mem_lanes(int g) {
  const size_t n = static_cast<size_t>(sm::kWaves) * sm::group_words(g) * sm::kLanes;
  DevBuf<uint32_t> table(sm::kTableWords), out(n);
  DevBuf<uint8_t> slice(sm::kSliceBytes);
  HIP_OK(hipMemcpy(table.p, mem_table_words().data(), sm::kTableBytes, hipMemcpyHostToDevice));
  HIP_OK(hipMemset(out.p, 0, n * 4));
  HIP_OK(hipMemset(slice.p, 0, sm::kSliceBytes));
  hipLaunchKernelGGL(mem_lanes_kernel_of(MemGroups{}, g), dim3(1), dim3(kSweepBlock), 0, 0, table.p, slice.p, out.p);
  HIP_OK(hipGetLastError());
  std::vector<uint32_t> h(n);
  HIP_OK(hipMemcpy(h.data(), out.p, n * 4, hipMemcpyDeviceToHost));
  return h;
}

// inject of cu_sweep_mem: (xcc, cu_key, group, index).
MemInject parse_mem_inject(const py::object& inject) {
  MemInject inj;
  if (inject.is_none()) return inj;
  const py::tuple t = inject.cast<py::tuple>();
  if (t.size() != 4) throw std::invalid_argument("cu_sweep_mem: inject = (xcc, cu_key, group, index)");
  inj.xcc = t[0].cast<int>();
  inj.cu_key = t[1].cast<int>();
  inj.group = kMemNames.index(t[2].cast<std::string>());
  inj.index = t[3].cast<int>();
  if (inj.index < 0 || inj.index >= sm::group_indices(inj.group)) throw std::invalid_argument("cu_sweep_mem: inject index beyond the group's");
  return inj;
}

struct PatternResult {
  size_t bytes = 0;
  unsigned long long errors = 0;
  std::vector<st::Mismatch> first;
  double fill_gbs = 0.0, verify_gbs = 0.0;
  size_t guard_changed = 0;   // guard bytes overwritten (guard_bytes > 0 only)
  size_t fill_launches = 0, verify_launches = 0;   // per pass
};

// Blocks a launch of hbm_fill / hbm_verify: 0 is the production bound, 1..kMaxLaunchBlocks a test's own.
uint64_t launch_blocks_arg(long long v) {
  if (v < 0 || static_cast<uint64_t>(v) > st::kMaxLaunchBlocks)
    throw std::invalid_argument("hbm_pattern_check: launch blocks in 0.." + std::to_string(st::kMaxLaunchBlocks) +
                                " (0: that many)");
  return v == 0 ? st::kMaxLaunchBlocks : static_cast<uint64_t>(v);
}

// Fill `bytes` of fresh device memory with the address-derived pattern and verify it, `passes`
// times (odd passes: the complement). `corrupt` = (byte offset, xor byte) pairs the host applies
// between a pass's fill and its verify; `verify_seed` < 0 verifies with `seed`. `guard_bytes`
// (tests) puts the buffer between two guard regions, see kGuardByte. A pass is one launch after
// another on one stream (st::launch_spans), each below 2^32 work-items, under one pair of events;
// `fill_launch_blocks` / `verify_launch_blocks` (tests) move the seams between them, separately.
// `cu_mask` (empty: every CU) is the CU mask of that stream, as in the sweep: the agent's mask of
// a device with fenced units, so that no fenced CU writes or judges the pattern.
PatternResult hbm_pattern_check(int dev, size_t bytes, uint32_t seed, int passes,
                                const std::vector<std::pair<uint64_t, uint32_t>>& corrupt, int64_t verify_seed,
                                size_t guard_bytes, long long fill_launch_blocks, long long verify_launch_blocks,
                                const std::vector<uint32_t>& cu_mask) {
  HIP_OK(hipSetDevice(dev));
  check_guard_bytes(guard_bytes);
  if (bytes == 0 || bytes % 16 != 0) throw std::invalid_argument("hbm_pattern_check: bytes must be a positive multiple of 16");
  if (passes < 1 || passes > 16) throw std::invalid_argument("hbm_pattern_check: passes in 1..16");
  for (const auto& c : corrupt)
    if (c.first >= bytes + guard_bytes || c.second > 0xff)   // with a guard, the guard behind the buffer too
      throw std::invalid_argument("hbm_pattern_check: corrupt = (offset < bytes, xor byte)");
  const size_t n = bytes / 16;
  const auto fill_spans = st::launch_spans(n, launch_blocks_arg(fill_launch_blocks));
  const auto verify_spans = st::launch_spans(n, launch_blocks_arg(verify_launch_blocks));
  const uint32_t vseed = verify_seed < 0 ? seed : static_cast<uint32_t>(verify_seed);

  struct Buf {   // an allocation that does not fit is the caller's to shrink, not a device fault
    unsigned char* p = nullptr;
    explicit Buf(size_t b) {
      const hipError_t e = hipMalloc(&p, b);
      if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        throw std::bad_alloc();
      }
      HIP_OK(e);
    }
    ~Buf() {
      if (p) (void)hipFree(p);
    }
  } whole(bytes + 2 * guard_bytes);
  u32x4* const data = reinterpret_cast<u32x4*>(whole.p + guard_bytes);
  if (guard_bytes) {
    HIP_OK(hipMemset(whole.p, kGuardByte, guard_bytes));
    HIP_OK(hipMemset(whole.p + guard_bytes + bytes, kGuardByte, guard_bytes));
    HIP_OK(hipDeviceSynchronize());   // the kernels run on a stream that does not wait for the null stream
  }
  DevBuf<VerifyOut> vo(1);
  Stream stream(cu_mask);
  Events ev;
  HIP_OK(hipMemsetAsync(vo.p, 0, sizeof(VerifyOut), stream.s));
  // n = 0 touches no memory: loads both kernels outside the timed spans
  hipLaunchKernelGGL(hbm_fill, dim3(1), dim3(kCopyBlock), 0, stream.s, data, size_t(0), uint64_t(0), seed, 0u);
  hipLaunchKernelGGL(hbm_verify, dim3(1), dim3(kCopyBlock), 0, stream.s, data, size_t(0), uint64_t(0), seed, 0u, vo.p);
  HIP_OK(hipGetLastError());
  HIP_OK(hipStreamSynchronize(stream.s));
  auto grid_of = [](uint64_t elements) { return dim3(static_cast<unsigned>(st::span_blocks(elements))); };
  double fill_ms = 0.0, verify_ms = 0.0;
  for (int pass = 0; pass < passes; ++pass) {
    HIP_OK(hipEventRecord(ev.a, stream.s));
    for (const auto& span : fill_spans)
      hipLaunchKernelGGL(hbm_fill, grid_of(span.second), dim3(kCopyBlock), 0, stream.s, data + span.first,
                         static_cast<size_t>(span.second), span.first, seed, static_cast<uint32_t>(pass));
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(ev.b, stream.s));
    fill_ms += ev.ms();
    for (const auto& c : corrupt) {
      unsigned char* at = reinterpret_cast<unsigned char*>(data) + c.first;
      unsigned char byte = 0;
      HIP_OK(hipMemcpy(&byte, at, 1, hipMemcpyDeviceToHost));
      byte ^= static_cast<unsigned char>(c.second);
      HIP_OK(hipMemcpy(at, &byte, 1, hipMemcpyHostToDevice));
    }
    HIP_OK(hipEventRecord(ev.a, stream.s));
    for (const auto& span : verify_spans)
      hipLaunchKernelGGL(hbm_verify, grid_of(span.second), dim3(kCopyBlock), 0, stream.s, data + span.first,
                         static_cast<size_t>(span.second), span.first, vseed, static_cast<uint32_t>(pass), vo.p);
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(ev.b, stream.s));
    verify_ms += ev.ms();
  }
  HIP_OK(hipStreamSynchronize(stream.s));
  VerifyOut h;
  HIP_OK(hipMemcpy(&h, vo.p, sizeof(VerifyOut), hipMemcpyDeviceToHost));
  PatternResult res;
  res.bytes = bytes;
  res.errors = h.errors;
  const size_t k = static_cast<size_t>(std::min<unsigned long long>(h.errors, st::kMismatchSlots));
  res.first.assign(h.slot, h.slot + k);
  std::stable_sort(res.first.begin(), res.first.end(),
                   [](const st::Mismatch& a, const st::Mismatch& b) { return a.element < b.element; });
  const double moved = static_cast<double>(bytes) * passes;
  res.fill_gbs = moved / (fill_ms * 1e-3) / 1e9;
  res.verify_gbs = moved / (verify_ms * 1e-3) / 1e9;
  res.guard_changed = guard_bytes_changed(whole.p, guard_bytes, bytes);
  res.fill_launches = fill_spans.size();
  res.verify_launches = verify_spans.size();
  return res;
}

using TileKernel = void (*)(const uint32_t*, const uint32_t*, const uint32_t*, const uint32_t*, uint32_t*);

// matrix_tile_kernel<P, opsel / 4, opsel % 4> for every opsel of the sequence: the byte selects
// are immediates of the instruction. The unscaled paths have the one instantiation <P, 0, 0>.
template <int P, int... I>
TileKernel opsel_kernel(std::integer_sequence<int, I...>, int opsel) {
  static constexpr TileKernel table[] = {matrix_tile_kernel<P, I / 4, I % 4>...};
  return table[sizeof...(I) == 1 ? 0 : opsel];
}

template <int P>
TileKernel path_kernel(int opsel) {
  return opsel_kernel<P>(std::make_integer_sequence<int, sp::path_scaled(P) ? 16 : 1>{}, opsel);
}

template <int... P>
TileKernel tile_kernel(std::integer_sequence<int, P...>, int p, int opsel) {
  static constexpr TileKernel (*table[])(int) = {path_kernel<P>...};
  return table[p](opsel);
}

// One instruction of path `p` on the caller's codes: a_codes is A[row][k] (dim x K, row-major),
// b_codes is B[k][col] (K x dim), scale_a is [row][k block] and scale_b [k block][col] (E8M0,
// scaled paths only), opsel_a / opsel_b the scale register's byte that carries them (the
// other bytes get another scale). Returns the tile's words, row-major (path_expected_words).
std::vector<uint32_t> matrix_tile(int p, const std::vector<uint64_t>& a_codes, const std::vector<uint64_t>& b_codes,
                                  const std::vector<uint32_t>& scale_a, const std::vector<uint32_t>& scale_b,
                                  int opsel_a, int opsel_b) {
  if (p < 0 || p >= sp::kNumPaths) throw std::invalid_argument("matrix_tile: unknown path");
  const int dim = sp::path_dim(p), K = sp::path_k(p), cb = sp::path_code_bits(p), rowdw = sp::path_row_dwords(p);
  const size_t n = static_cast<size_t>(dim) * K;
  if (a_codes.size() != n || b_codes.size() != n)
    throw std::invalid_argument("matrix_tile: A is dim x K codes and B is K x dim codes");
  const size_t n_scale = sp::path_scaled(p) ? static_cast<size_t>(dim) * 2 : 0;
  if (scale_a.size() != n_scale || scale_b.size() != n_scale)
    throw std::invalid_argument("matrix_tile: scales are dim x 2 and 2 x dim on the scaled paths, absent elsewhere");
  if (opsel_a < 0 || opsel_a > 3 || opsel_b < 0 || opsel_b > 3) throw std::invalid_argument("matrix_tile: opsel in 0..3");
  std::vector<uint32_t> A(static_cast<size_t>(dim) * rowdw, 0u), B(A.size(), 0u), SA(dim * 2, 0u), SB(dim * 2, 0u);
  auto put = [&](std::vector<uint32_t>& v, int idx, int k, uint64_t code) {
    if (cb < 64 && (code >> cb)) throw std::invalid_argument("matrix_tile: a code wider than the format");
    size_t bit = static_cast<size_t>(idx) * rowdw * 32 + static_cast<size_t>(k) * cb;
    for (int i = 0; i < cb;) {
      const int sh = static_cast<int>(bit % 32), take = std::min(cb - i, 32 - sh);
      v[bit / 32] |= static_cast<uint32_t>((code >> i) & ((1ull << take) - 1)) << sh;
      i += take;
      bit += take;
    }
  };
  for (int i = 0; i < dim; ++i)
    for (int k = 0; k < K; ++k) {
      put(A, i, k, a_codes[static_cast<size_t>(i) * K + k]);
      put(B, i, k, b_codes[static_cast<size_t>(k) * dim + i]);
    }
  auto scale_dword = [](uint32_t scale, int byte) {
    if (scale > 0xfe) throw std::invalid_argument("matrix_tile: an E8M0 scale is 0..254");
    return ((scale ^ 1u) * 0x01010101u & ~(0xffu << (8 * byte))) | (scale << (8 * byte));
  };
  for (size_t i = 0; i < n_scale / 2; ++i)
    for (int blk = 0; blk < 2; ++blk) {
      SA[i * 2 + blk] = scale_dword(scale_a[i * 2 + blk], opsel_a);
      SB[i * 2 + blk] = scale_dword(scale_b[static_cast<size_t>(blk) * dim + i], opsel_b);
    }
  DevBuf<uint32_t> da(A.size()), db(B.size()), dsa(SA.size()), dsb(SB.size()), dc(sp::kTileWords);
  HIP_OK(hipMemcpy(da.p, A.data(), A.size() * 4, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(db.p, B.data(), B.size() * 4, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(dsa.p, SA.data(), SA.size() * 4, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(dsb.p, SB.data(), SB.size() * 4, hipMemcpyHostToDevice));
  HIP_OK(hipMemset(dc.p, 0, sp::kTileWords * 4));
  hipLaunchKernelGGL(tile_kernel(AllPaths{}, p, opsel_a * 4 + opsel_b), dim3(1), dim3(64), 0, 0, da.p, db.p, dsa.p, dsb.p,
                     dc.p);
  HIP_OK(hipGetLastError());
  std::vector<uint32_t> c(sp::path_tile_words(p));
  HIP_OK(hipMemcpy(c.data(), dc.p, c.size() * 4, hipMemcpyDeviceToHost));
  return c;
}

// inject of cu_sweep: (xcc, cu_key, 'mfma' | 'lds'[, lds dword]); of cu_sweep_paths: (xcc, cu_key, path name).
SweepInject parse_inject(const py::object& inject, bool paths) {
  SweepInject inj;
  if (inject.is_none()) return inj;
  const py::tuple t = inject.cast<py::tuple>();
  if (paths ? t.size() != 3 : t.size() < 3 || t.size() > 4)
    throw std::invalid_argument(paths ? "cu_sweep_paths: inject = (xcc, cu_key, path name)"
                                      : "cu_sweep: inject = (xcc, cu_key, kind[, lds_dword])");
  inj.xcc = t[0].cast<int>();
  inj.cu_key = t[1].cast<int>();
  const std::string kind = t[2].cast<std::string>();
  if (paths) {
    inj.kind = kInjectPath;
    inj.path = kPathNames.index(kind);
  } else if (kind == "mfma") {
    inj.kind = kInjectMfma;
  } else if (kind == "lds") {
    inj.kind = kInjectLds;
  } else {
    throw std::invalid_argument("cu_sweep: inject kind is 'mfma' or 'lds'");
  }
  if (t.size() == 4) inj.lds_off = t[3].cast<uint32_t>();
  return inj;
}

// "bf16" is table 0, path p's tile 1 + p (WordFlip).
int tile_index(const std::string& name) { return name == "bf16" ? 0 : 1 + kPathNames.index(name); }
int group_index(const std::string& name) { return kValuNames.index(name); }
int scalar_index(const std::string& name) { return kScalarNames.index(name); }

// corrupt_expected = (table name, word, xor), or (word, xor) of table 0 where `table` is null. `usage` is the message.
WordFlip parse_flip(const py::object& corrupt, int (*table)(const std::string&), const char* usage) {
  WordFlip f;
  if (corrupt.is_none()) return f;
  const py::tuple t = corrupt.cast<py::tuple>();
  const size_t named = table ? 1 : 0;
  if (t.size() != 2 + named) throw std::invalid_argument(usage);
  f.table = table ? table(t[0].cast<std::string>()) : 0;
  f.word = t[named].cast<uint32_t>();
  f.mask = t[named + 1].cast<uint32_t>();
  return f;
}

static_assert(st::kNoBadOffset == sv::kNoBad, "one 'none' word in every record");
int64_t or_minus1(uint32_t v) { return v == sv::kNoBad ? int64_t(-1) : int64_t(v); }

// {words: [(AND tuple, OR tuple)] per flip, records, seconds}; `tuple` packs one half's n words.
template <class Tuple>
py::dict sensitivity_dict(const Sensitivity& r, size_t flips, size_t n, Tuple&& tuple) {
  py::list words;
  for (size_t i = 0; i < flips; ++i) {
    const uint32_t* f = r.fields.data() + 2 * n * i;
    words.append(py::make_tuple(tuple(f), tuple(f + n)));
  }
  py::dict d;
  d["words"] = words;
  d["records"] = r.records;
  d["seconds"] = r.seconds;
  return d;
}

// cu_sweep (`paths` null: 5-field records) and cu_sweep_paths (7 fields, and the keys `paths` / `checked`).
py::dict sweep_binding(int dev, const std::vector<uint32_t>& mask, int rounds, uint32_t seed,
                       const std::vector<std::string>* paths, const py::object& inject, const py::object& corrupt_expected,
                       std::optional<size_t> lds_bytes) {
  const uint32_t bits = paths ? kPathNames.bits(*paths) : 0u;
  if (paths && !bits) throw std::invalid_argument("cu_sweep_paths: no path selected");
  const SweepInject inj = parse_inject(inject, paths != nullptr);
  const WordFlip flip = paths ? parse_flip(corrupt_expected, tile_index, "cu_sweep_paths: corrupt_expected = ('bf16' | path name, word, xor)")
                              : parse_flip(corrupt_expected, nullptr, "cu_sweep: corrupt_expected = (word, xor)");
  CuRun r;
  size_t lds = 0;
  {
    py::gil_scoped_release nogil;
    HIP_OK(hipSetDevice(dev));
    SweepSession session(dev, mask, rounds, bits, lds_bytes);
    session.set_flip(flip);
    r = session.run(seed, inj);
    lds = session.lds_bytes();
  }
  py::list recs;
  for (int b = 0; b < r.blocks; ++b) {
    const st::SweepRecord rec = st::decode_record(r.words.data(), b, r.record_words);
    const py::tuple base = py::make_tuple(rec.xcc, rec.hw_id, rec.fail, rec.simds, or_minus1(rec.lds_bad));
    recs.append(paths ? py::tuple(base + py::make_tuple(rec.path_fail, rec.path_waves)) : base);
  }
  py::dict d;
  d["records"] = recs;
  if (paths) {
    const auto [names, checked] = kPathNames.names_and_checked(bits);
    d["paths"] = names;
    d["checked"] = checked;
  }
  d["lds_bytes"] = lds;
  d["ms"] = r.ms;
  return d;
}

py::dict valu_binding(int dev, const std::vector<uint32_t>& mask, int rounds, uint32_t seed, const std::vector<std::string>& groups,
                      const py::object& inject, const py::object& corrupt_expected) {
  const uint32_t bits = kValuNames.bits(groups);
  const ValuInject inj = parse_valu_inject(inject);
  const WordFlip flip = parse_flip(corrupt_expected, group_index, "cu_sweep_valu: corrupt_expected = (group, word, xor)");
  CuRun r;
  size_t scratch = 0;
  int regs = 0;
  {
    py::gil_scoped_release nogil;
    HIP_OK(hipSetDevice(dev));
    ValuSession session(dev, mask, rounds, bits);
    session.set_flip(flip);
    r = session.run(seed, inj);
    scratch = session.scratch_bytes();
    regs = session.regs_per_lane();
  }
  py::list recs;
  for (int b = 0; b < r.blocks; ++b) {
    const sv::ValuRecord rec = sv::decode_valu_record(r.words.data(), b);
    recs.append(py::make_tuple(rec.xcc, rec.hw_id, rec.fail, rec.simds, rec.groups, or_minus1(rec.bad_slot), or_minus1(rec.bad_thread),
                               rec.approx_hash));
  }
  py::dict d;
  d["records"] = recs;
  const auto [names, checked] = kValuNames.names_and_checked(bits);
  d["groups"] = names;
  d["checked"] = checked;
  d["reg_slots"] = sv::kRegSlots;
  d["regs_per_lane"] = regs;
  d["scratch_bytes"] = scratch;
  d["ms"] = r.ms;
  return d;
}

// Per word the fields fail, lds_bad, path_fail and path_waves (the last two 0 when `paths` is empty).
py::dict sweep_sensitivity(int dev, const std::string& tile, const std::vector<std::pair<uint32_t, uint32_t>>& flips,
                           const std::vector<std::string>& paths, const std::vector<uint32_t>& mask, int rounds, uint32_t seed) {
  const uint32_t bits = kPathNames.bits(paths);
  const int t = tile_index(tile);
  Sensitivity r;
  {
    py::gil_scoped_release nogil;
    HIP_OK(hipSetDevice(dev));
    if (flips.size() > 4096) throw std::invalid_argument("sweep_sensitivity: at most 4096 words a call");
    SweepSession session(dev, mask, rounds, bits);
    r = sensitivity<4>(
        session, seed, flips,
        [&](const std::pair<uint32_t, uint32_t>& f) { session.set_flip(WordFlip{t, f.first, f.second}); },
        [](const CuRun& run, int b) {
          const st::SweepRecord rec = st::decode_record(run.words.data(), b, run.record_words);
          return std::array<uint32_t, 4>{rec.fail, rec.lds_bad, rec.path_fail, rec.path_waves};
        });
  }
  return sensitivity_dict(r, flips.size(), 4, [](const uint32_t* f) { return py::make_tuple(f[0], or_minus1(f[1]), f[2], f[3]); });
}

py::dict valu_sensitivity(int dev, const std::string& group, const std::vector<std::pair<uint32_t, uint32_t>>& flips,
                          const std::vector<uint32_t>& mask, int rounds, uint32_t seed) {
  const int g = kValuNames.index(group);
  if (flips.size() > 4096) throw std::invalid_argument("valu_sensitivity: at most 4096 words a call");
  Sensitivity r;
  {
    py::gil_scoped_release nogil;
    HIP_OK(hipSetDevice(dev));
    ValuSession session(dev, mask, rounds, sv::kAllExact);
    r = sensitivity<2>(
        session, seed, flips,
        [&](const std::pair<uint32_t, uint32_t>& f) { session.set_flip(WordFlip{g, f.first, f.second}); },
        [](const CuRun& run, int b) {
          const sv::ValuRecord rec = sv::decode_valu_record(run.words.data(), b);
          return std::array<uint32_t, 2>{rec.fail, rec.groups};
        });
  }
  return sensitivity_dict(r, flips.size(), 2, [](const uint32_t* f) { return py::make_tuple(f[0], f[1]); });
}

py::dict scalar_binding(int dev, const std::vector<uint32_t>& mask, int rounds, uint32_t seed, const std::vector<std::string>& groups,
                        const py::object& inject, const py::object& corrupt_expected) {
  const uint32_t bits = kScalarNames.bits(groups);
  const ScalarInject inj = parse_scalar_inject(inject);
  const WordFlip flip = parse_flip(corrupt_expected, scalar_index, "cu_sweep_scalar: corrupt_expected = (group | 'smem', word, xor)");
  CuRun r;
  size_t scratch = 0;
  int num_regs = 0;
  {
    py::gil_scoped_release nogil;
    HIP_OK(hipSetDevice(dev));
    ScalarSession session(dev, mask, rounds, bits);
    session.set_flip(flip);
    r = session.run(seed, inj);
    scratch = session.scratch_bytes();
    num_regs = session.num_regs();
  }
  py::list recs;
  for (int b = 0; b < r.blocks; ++b) {
    const ss::ScalarRecord rec = ss::decode_scalar_record(r.words.data(), b);
    recs.append(py::make_tuple(rec.xcc, rec.hw_id, rec.fail, rec.simds, rec.groups, or_minus1(rec.bad_index), or_minus1(rec.bad_wave),
                               or_minus1(rec.bad_which)));
  }
  py::dict d;
  d["records"] = recs;
  const auto [names, checked] = kScalarNames.names_and_checked(bits);
  d["groups"] = names;
  d["checked"] = checked;
  d["sreg_slots"] = ss::kSregSlots;
  d["num_regs"] = num_regs;   // hipFuncAttributes has no count of scalar registers
  d["scratch_bytes"] = scratch;
  d["ms"] = r.ms;
  return d;
}

// Per word the fields fail, failed-group bits and first bad index (a table word of 'smem').
py::dict scalar_sensitivity(int dev, const std::string& group, const std::vector<std::pair<uint32_t, uint32_t>>& flips,
                            const std::vector<uint32_t>& mask, int rounds, uint32_t seed) {
  const int g = kScalarNames.index(group);
  if (flips.size() > 4096) throw std::invalid_argument("scalar_sensitivity: at most 4096 words a call");
  Sensitivity r;
  {
    py::gil_scoped_release nogil;
    HIP_OK(hipSetDevice(dev));
    ScalarSession session(dev, mask, rounds, ss::kAllExact | 1u << ss::kSmem);
    r = sensitivity<3>(
        session, seed, flips,
        [&](const std::pair<uint32_t, uint32_t>& f) { session.set_flip(WordFlip{g, f.first, f.second}); },
        [](const CuRun& run, int b) {
          const ss::ScalarRecord rec = ss::decode_scalar_record(run.words.data(), b);
          return std::array<uint32_t, 3>{rec.fail, rec.groups, rec.bad_index};
        });
  }
  return sensitivity_dict(r, flips.size(), 3, [](const uint32_t* f) { return py::make_tuple(f[0], f[1], or_minus1(f[2])); });
}

int mem_index(const std::string& name) { return kMemNames.index(name); }

py::dict mem_binding(int dev, const std::vector<uint32_t>& mask, int rounds, uint32_t seed, const std::vector<std::string>& groups,
                     const py::object& inject, const py::object& corrupt_expected) {
  const uint32_t bits = kMemNames.bits(groups);
  const MemInject inj = parse_mem_inject(inject);
  const WordFlip flip = parse_flip(corrupt_expected, mem_index, "cu_sweep_mem: corrupt_expected = ('gload' | 'l1' | 'ldsdma', word, xor)");
  CuRun r;
  size_t scratch = 0;
  int num_regs = 0;
  {
    py::gil_scoped_release nogil;
    HIP_OK(hipSetDevice(dev));
    MemSession session(dev, mask, rounds, bits);
    session.set_flip(flip);
    r = session.run(seed, inj);
    scratch = session.scratch_bytes();
    num_regs = session.num_regs();
  }
  py::list recs;
  for (int b = 0; b < r.blocks; ++b) {
    const sm::MemRecord rec = sm::decode_mem_record(r.words.data(), b);
    recs.append(py::make_tuple(rec.xcc, rec.hw_id, rec.fail, rec.simds, rec.groups, or_minus1(rec.bad_group), or_minus1(rec.bad_index),
                               or_minus1(rec.bad_wave)));
  }
  py::dict d;
  d["records"] = recs;
  const auto [names, checked] = kMemNames.names_and_checked(bits);
  d["groups"] = names;
  d["checked"] = checked;
  d["table_words"] = sm::kTableWords;
  d["slice_bytes"] = sm::kSliceBytes;
  d["num_regs"] = num_regs;
  d["scratch_bytes"] = scratch;
  d["ms"] = r.ms;
  return d;
}

// Per word the fields fail, failed-group bits, first bad group and its lowest bad index.
py::dict mem_sensitivity(int dev, const std::string& group, const std::vector<std::pair<uint32_t, uint32_t>>& flips,
                         const std::vector<uint32_t>& mask, int rounds, uint32_t seed) {
  const int g = kMemNames.index(group);
  if (flips.size() > 4096) throw std::invalid_argument("mem_sensitivity: at most 4096 words a call");
  Sensitivity r;
  {
    py::gil_scoped_release nogil;
    HIP_OK(hipSetDevice(dev));
    MemSession session(dev, mask, rounds, 1u << g);
    r = sensitivity<4>(
        session, seed, flips,
        [&](const std::pair<uint32_t, uint32_t>& f) { session.set_flip(WordFlip{g, f.first, f.second}); },
        [](const CuRun& run, int b) {
          const sm::MemRecord rec = sm::decode_mem_record(run.words.data(), b);
          return std::array<uint32_t, 4>{rec.fail, rec.groups, rec.bad_group, rec.bad_index};
        });
  }
  return sensitivity_dict(r, flips.size(), 4, [](const uint32_t* f) { return py::make_tuple(f[0], f[1], or_minus1(f[2]), or_minus1(f[3])); });
}

}  // namespace

PYBIND11_MODULE(_probe, m) {
  m.doc() = "MI355X calibration kernels (gfx950): CU census, MFMA burn, HBM and xGMI bandwidth";
  m.def("device_count", []() {
    int n = 0;
    HIP_OK(hipGetDeviceCount(&n));
    return n;
  });
  m.def("device_props", &device_props, py::arg("device") = 0);
  m.def("hbm_bandwidth", &hbm_bandwidth, py::arg("device") = 0, py::arg("bytes") = size_t(1) << 30,
        py::arg("iters") = 10, py::call_guard<py::gil_scoped_release>(),
        "Streaming copy bandwidth in GB/s (read + write bytes).");
  m.def("cu_census", &census, py::arg("device") = 0, py::arg("cu_mask") = std::vector<uint32_t>{},
        py::arg("blocks") = 2048, py::arg("sleep_iters") = 64,
        "Per-workgroup (xcc_id, hw_id) for a launch on a CU-masked stream.");
  m.def("mfma_throughput", &mfma_throughput, py::arg("device") = 0,
        py::arg("cu_mask") = std::vector<uint32_t>{}, py::arg("blocks") = 2048, py::arg("iters") = 2048,
        "bf16 MFMA TFLOP/s on a CU-masked stream.");
  m.def("gemm_tile", &gemm_tile, py::arg("a"), py::arg("b"),
        "C[32x32] = bf16(A[32x16]) @ bf16(B[16x32]) with one v_mfma_f32_32x32x16_bf16 (fp32 accumulate).");
  m.def(
      "copy_check",
      [](int dev, size_t n_floats, size_t guard_bytes) -> py::object {
        CopyCheck r;
        {
          py::gil_scoped_release nogil;
          r = copy_check(dev, n_floats, guard_bytes);
        }
        if (guard_bytes == 0) return py::bool_(r.ok);
        py::dict d;
        d["ok"] = r.ok;
        d["guards_ok"] = r.guard_changed == 0;
        d["guard_bytes_changed"] = r.guard_changed;
        return d;
      },
      py::arg("device") = 0, py::arg("n_floats") = size_t(1) << 24, py::arg("guard_bytes") = size_t(0),
      "hbm_copy kernel result == source, bit for bit. Test hook: guard_bytes > 0 (a multiple of 16) puts the "
      "destination between two guard regions of that size and returns {ok, guards_ok, guard_bytes_changed} "
      "instead of the bool: guards_ok is false when the kernel wrote outside the destination.");
  m.def("mixed_colocated", &mixed_colocated, py::arg("device"), py::arg("hbm_mask"), py::arg("mfma_mask"),
        py::arg("bytes") = size_t(1) << 30, py::arg("iters") = 10, py::arg("mfma_blocks") = 1536,
        py::arg("mfma_iters") = 4096, py::call_guard<py::gil_scoped_release>(),
        "{copy GB/s, MFMA TFLOP/s} for a streaming tenant beside a compute-bound one.");
  m.def("hbm_colocated", &hbm_colocated, py::arg("device"), py::arg("cu_masks"), py::arg("bytes") = size_t(1) << 30,
        py::arg("iters") = 10, py::arg("iters_each") = std::vector<int>{}, py::call_guard<py::gil_scoped_release>(),
        "Per-tenant HBM copy GB/s for concurrent tenants on CU-masked streams.");
  m.def("mfma_colocated", &mfma_colocated, py::arg("device"), py::arg("cu_masks"), py::arg("blocks"),
        py::arg("iters") = 2048, py::call_guard<py::gil_scoped_release>(),
        "Concurrent MFMA burns on CU-masked streams; per-stream TFLOP/s.");
  m.def(
      "peer_bandwidth",
      [](int src, int dst, size_t bytes, int iters, double deadline_s) {
        PeerRate r;
        {
          py::gil_scoped_release nogil;
          r = peer_bandwidth(src, dst, bytes, iters, deadline_s);
        }
        py::dict d;
        d["pull_gbs"] = r.pull_gbs;
        d["dma_gbs"] = r.dma_gbs;
        d["peer_access"] = r.peer_access;
        d["gbs"] = std::max(r.pull_gbs, r.dma_gbs);
        return d;
      },
      py::arg("src"), py::arg("dst"), py::arg("bytes") = size_t(256) << 20, py::arg("iters") = 10,
      py::arg("deadline_s") = 30.0,
      "One-direction xGMI rate src -> dst in GB/s: copy kernel pulling over peer access, and SDMA. "
      "Raises TimeoutError when the transfers do not finish within deadline_s (the work is abandoned).");
  py::register_exception<PeerTimeout>(m, "PeerTimeout", PyExc_TimeoutError);
  m.def(
      "cu_sweep",
      [](int dev, const std::vector<uint32_t>& mask, int rounds, uint32_t seed, const py::object& inject,
         const py::object& corrupt_expected, std::optional<size_t> lds_bytes) {
        return sweep_binding(dev, mask, rounds, seed, nullptr, inject, corrupt_expected, lds_bytes);
      },
      py::arg("device") = 0, py::arg("cu_mask") = std::vector<uint32_t>{}, py::arg("rounds") = 4,
      py::arg("seed") = 0x5eed5eedu, py::arg("inject") = py::none(), py::arg("corrupt_expected") = py::none(),
      py::arg("lds_bytes") = py::none(),
      "Deep CU check on a CU-masked stream: rounds x CUs workgroups, each holding a CU's whole LDS, run an "
      "exact bf16 MFMA chain on all 4 waves and a pattern test of the LDS. Records are (xcc, hw_id, fail bits, "
      "SIMD ids seen, first bad LDS dword or -1). inject = (xcc, cu_key, 'mfma' | 'lds'[, lds dword]) flips one "
      "bit of that CU's own data (tests). Test hook: corrupt_expected = (word, xor) XORs word 0..1023 of the host's "
      "expected bf16 tile in the upload, so every wave of every visit must report the MFMA check failed. Test hook: "
      "lds_bytes (a multiple of 16, 16..65536) runs the dynamic-LDS kernel with that much LDS instead of the one a "
      "device without room for a whole-LDS block would get; several such workgroups share a CU, so a visit of "
      "every CU is not promised in this mode.");
  m.def(
      "matrix_tile",
      [](const std::string& path, const std::vector<uint64_t>& a, const std::vector<uint64_t>& b,
         const std::vector<uint32_t>& scale_a, const std::vector<uint32_t>& scale_b, std::pair<int, int> opsel) {
        const int p = kPathNames.index(path);
        const std::vector<uint32_t> w = matrix_tile(p, a, b, scale_a, scale_b, opsel.first, opsel.second);
        py::list c;
        const size_t n = static_cast<size_t>(sp::path_dim(p)) * sp::path_dim(p);
        for (size_t i = 0; i < n; ++i) {
          if (p == sp::kI8) {
            c.append(static_cast<int32_t>(w[i]));
          } else if (p == sp::kF64) {
            const uint64_t bits = (static_cast<uint64_t>(w[2 * i + 1]) << 32) | w[2 * i];
            double v;
            std::memcpy(&v, &bits, 8);
            c.append(v);
          } else {
            float v;
            std::memcpy(&v, &w[i], 4);
            c.append(v);
          }
        }
        return c;
      },
      py::arg("path"), py::arg("a_codes"), py::arg("b_codes"), py::arg("scale_a") = std::vector<uint32_t>{},
      py::arg("scale_b") = std::vector<uint32_t>{}, py::arg("opsel") = std::pair<int, int>{0, 0},
      "One MFMA instruction of `path` (f16, fp8, bf8, i8, mxfp8, mxfp6, mxfp4, f32, f64) on operand codes: "
      "a_codes = A[row][k] and b_codes = B[k][col] bit patterns, row-major; on the scaled paths scale_a = "
      "[row][k block] and scale_b = [k block][col] E8M0 codes, carried in byte opsel = (a, b) of the scale "
      "register. Returns C row-major: floats, ints for i8, doubles (16x16) for f64.");
  m.def(
      "cu_sweep_paths",
      [](int dev, const std::vector<uint32_t>& mask, int rounds, uint32_t seed, const std::vector<std::string>& paths,
         const py::object& inject, const py::object& corrupt_expected, std::optional<size_t> lds_bytes) {
        return sweep_binding(dev, mask, rounds, seed, &paths, inject, corrupt_expected, lds_bytes);
      },
      py::arg("device") = 0, py::arg("cu_mask") = std::vector<uint32_t>{}, py::arg("rounds") = 4,
      py::arg("seed") = 0x5eed5eedu, py::arg("paths") = std::vector<std::string>{}, py::arg("inject") = py::none(),
      py::arg("corrupt_expected") = py::none(), py::arg("lds_bytes") = py::none(),
      "cu_sweep whose visits also run, on all 4 waves, an exact chain of 8 MFMA instructions of every path in "
      "`paths` and compare every accumulator bit with the host's tile. Records are cu_sweep's 5 fields plus "
      "(failed-path bits, waves that saw a path fail); `paths` in the result names the bits in order, `checked` "
      "the paths that ran. inject = (xcc, cu_key, path name) flips one accumulator bit of that path on that CU (tests). "
      "Test hook: corrupt_expected = ('bf16' | path name, word, xor) XORs one word of that expected tile (1024 "
      "words, f64 512) in this call's upload, never in the host's cached tiles; the path must be selected. Test hook: "
      "lds_bytes as in cu_sweep, 36864 (the nine staged tiles)..65536; a visit of every CU is not promised then.");
  m.def(
      "sweep_sensitivity",
      &sweep_sensitivity,
      py::arg("device"), py::arg("tile"), py::arg("flips"), py::arg("paths") = std::vector<std::string>{},
      py::arg("cu_mask") = std::vector<uint32_t>{}, py::arg("rounds") = 1, py::arg("seed") = 0x5eed5eedu,
      "Test hook: for every (word, xor) of `flips` one sweep (cu_sweep_paths over `paths`, or cu_sweep when "
      "`paths` is empty) with that word of expected tile `tile` ('bf16' or a path name) corrupted as by "
      "corrupt_expected, all on one set of buffers. words[i] = (AND, OR) over that sweep's records of (fail bits, "
      "lds_bad or -1, failed-path bits, path waves); records = workgroups per sweep, seconds = the loop's wall time.");
  m.def(
      "hbm_pattern_check",
      [](int dev, size_t bytes, uint32_t seed, int passes, const std::vector<std::pair<uint64_t, uint32_t>>& corrupt,
         const py::object& verify_seed, size_t guard_bytes, long long fill_launch_blocks,
         long long verify_launch_blocks, const std::vector<uint32_t>& cu_mask) {
        const int64_t vseed = verify_seed.is_none() ? int64_t(-1) : int64_t(verify_seed.cast<uint32_t>());
        PatternResult r;
        {
          py::gil_scoped_release nogil;
          r = hbm_pattern_check(dev, bytes, seed, passes, corrupt, vseed, guard_bytes, fill_launch_blocks,
                                verify_launch_blocks, cu_mask);
        }
        py::list first;
        for (const st::Mismatch& mm : r.first)
          first.append(py::make_tuple(st::mismatch_byte_offset(mm), mm.expected, mm.got));
        py::dict d;
        d["bytes"] = r.bytes;
        d["errors"] = r.errors;
        d["first"] = first;
        d["fill_gbs"] = r.fill_gbs;
        d["verify_gbs"] = r.verify_gbs;
        d["fill_launches"] = r.fill_launches;
        d["verify_launches"] = r.verify_launches;
        if (guard_bytes) d["guard_ok"] = r.guard_changed == 0;
        return d;
      },
      py::arg("device") = 0, py::arg("bytes") = size_t(256) << 20, py::arg("seed") = 0x5eed5eedu,
      py::arg("passes") = 2, py::arg("corrupt") = std::vector<std::pair<uint64_t, uint32_t>>{},
      py::arg("verify_seed") = py::none(), py::arg("guard_bytes") = size_t(0), py::arg("fill_launch_blocks") = 0LL,
      py::arg("verify_launch_blocks") = 0LL, py::arg("cu_mask") = std::vector<uint32_t>{},
      "Fills `bytes` of device memory with an address-derived pattern and verifies it (odd passes: the "
      "complement). errors counts mismatching 16-byte elements over all passes; first = up to 16 of "
      "(byte offset of the first differing byte, expected word, got word). corrupt = [(byte offset, xor byte)] "
      "is applied by the host between fill and verify. Test hook: guard_bytes > 0 (a multiple of 16) puts the "
      "buffer between two guard regions of that size and adds guard_ok, false when a guard byte changed: a kernel "
      "wrote outside the buffer, or `corrupt` named an offset in the guard behind it (bytes <= offset < bytes + guard_bytes). A pass is one launch after another of at most 2^22 blocks (64 GiB), "
      "each below the 2^32 work-items HIP supports; fill_launches / verify_launches count them per pass. Test hook: "
      "fill_launch_blocks / verify_launch_blocks = blocks of 1,024 elements a launch of the fill / of the verify "
      "(0: 2^22; 1..2^22; anything else raises ValueError). cu_mask = 32-bit words of a CU mask (as cu_sweep's): the fill, "
      "the verify and the clearing of their result run on a stream masked to those CUs; empty: an unmasked stream, "
      "every CU. Raises MemoryError when the buffer cannot be allocated.");
  m.def(
      "cu_sweep_valu",
      &valu_binding,
      py::arg("device") = 0, py::arg("cu_mask") = std::vector<uint32_t>{}, py::arg("rounds") = 4,
      py::arg("seed") = 0x5eed5eedu, py::arg("groups") = std::vector<std::string>{}, py::arg("inject") = py::none(),
      py::arg("corrupt_expected") = py::none(),
      "Vector-ALU part of the deep CU check, on cu_sweep's grid and stream: all 4 waves of every visit run the exact "
      "chains of the selected groups (fma32, fma64, pkfma16, pkfma32, addmul32, int32, int64, bits, dot, cvt, xlane) "
      "against the host's table, 'approx' (exp2, log2, rcp, rsq, sqrt within 8 ulp of libm, and one hash per wave) and "
      "'regs' (a pattern test of reg_slots vector registers a lane, twice). Records are (xcc, hw_id, fail bits: 0..3 exact "
      "groups, 4..7 registers, 8..11 approx bound, 12..15 approx hash unlike wave 0's, by wave; SIMD ids seen; failed-group "
      "bits; first bad slot or -1; its thread (wave << 6 | lane) or -1; wave 0's approx hash). `groups` in the result names "
      "the bits, `checked` what ran; regs_per_lane and scratch_bytes are the kernel's attributes as the runtime reports "
      "them ('regs' raises when scratch_bytes is not 0). inject = (xcc, cu_key, 'valu', group) | (xcc, cu_key, 'regs', slot) "
      "| (xcc, cu_key, 'approx') flips one bit of that CU's wave 0, lane 0 (tests): of the group's result, of one approx "
      "output, or of the value held slot `slot` is compared with (the held register is not written: that would cost "
      "the registers under test; the reported slot, wave and lane are the same). Test hook: corrupt_expected = (group, "
      "word 0..127, xor) XORs one word of that group's expected words in this call's upload only.");
  m.def(
      "valu_lanes",
      [](const std::string& group) -> py::object {
        const int g = kValuNames.index(group);
        const std::vector<uint32_t> w = valu_lanes(g);
        py::list out;
        for (uint32_t v : w) {
          if (g == sv::kApprox) out.append(sv::bits_float(v));
          else out.append(v);
        }
        return out;
      },
      py::arg("group"),
      "One wave runs group `group`: the 128 words [lane][2] of an exact group, or for 'approx' the 320 floats [op][lane] "
      "of exp2, log2, rcp, rsq, sqrt.");
  m.def(
      "valu_sensitivity",
      &valu_sensitivity,
      py::arg("device"), py::arg("group"), py::arg("flips"), py::arg("cu_mask") = std::vector<uint32_t>{},
      py::arg("rounds") = 1, py::arg("seed") = 0x5eed5eedu,
      "Test hook: for every (word, xor) of `flips` one cu_sweep_valu over every exact group with that word of `group`'s "
      "expected words corrupted, all on one session. words[i] = (AND, OR) over that sweep's records of (fail bits, "
      "failed-group bits); records = workgroups per sweep, seconds = the loop's wall time.");
  m.def(
      "cu_sweep_scalar",
      &scalar_binding,
      py::arg("device") = 0, py::arg("cu_mask") = std::vector<uint32_t>{}, py::arg("rounds") = 4,
      py::arg("seed") = 0x5eed5eedu, py::arg("groups") = std::vector<std::string>{}, py::arg("inject") = py::none(),
      py::arg("corrupt_expected") = py::none(),
      "Scalar part of the deep CU check, on cu_sweep's grid and stream: all 4 waves of every visit run the exact chains "
      "of the selected groups (add, mul, shift, logic, bits, cmp: one asm statement per scalar-ALU instruction; vcc: the "
      "vector / scalar boundary) against the host's table of 224 words, 'smem' (scalar loads of every width from a "
      "read-only table of 4096 words, wave w its quarter) and 'sregs' (a pattern test of sreg_slots named scalar "
      "registers a wave, twice). Records are (xcc, hw_id, fail bits: 0..3 exact groups, 4..7 smem, 8..11 sregs, by wave; "
      "SIMD ids seen; failed-group bits; first bad register slot, else first bad table word, or -1; its wave or -1; 0 for "
      "a slot, 1 for a word, or -1). `groups` in the result names the bits, `checked` what ran; num_regs and scratch_bytes "
      "are the kernel's attributes as the runtime reports them (it has no count of scalar registers; 'sregs' raises when scratch_bytes is not 0). inject = "
      "(xcc, cu_key, 'scalar', group) | (xcc, cu_key, 'smem', word) | (xcc, cu_key, 'sregs', slot) flips bit 0 on that CU "
      "(tests): of the group's first result word on wave 0, of the value table word `word` is compared with (on the wave "
      "that reads it: word // 1024), or of the value slot `slot` is compared with in pass 0 on wave 0 (the held "
      "register is not written). Test hook: corrupt_expected = (group, word 0..31, xor) | ('smem', word 0..4095, xor) "
      "XORs one word of that table in this call's upload only.");
  m.def(
      "scalar_words",
      [](const std::string& group) { return scalar_words(kScalarNames.index(group)); },
      py::arg("group"), "One workgroup of four waves runs exact scalar group `group`: its 32 words [wave][8].");
  m.def(
      "scalar_sensitivity",
      &scalar_sensitivity,
      py::arg("device"), py::arg("group"), py::arg("flips"), py::arg("cu_mask") = std::vector<uint32_t>{},
      py::arg("rounds") = 1, py::arg("seed") = 0x5eed5eedu,
      "Test hook: for every (word, xor) of `flips` one cu_sweep_scalar over every exact group and 'smem' with that word "
      "of `group`'s expected words (or, for 'smem', of the load table) corrupted, all on one session. words[i] = (AND, "
      "OR) over that sweep's records of (fail bits, failed-group bits, first bad index or -1); records = workgroups per "
      "sweep, seconds = the loop's wall time.");
  m.def(
      "cu_sweep_mem",
      &mem_binding,
      py::arg("device") = 0, py::arg("cu_mask") = std::vector<uint32_t>{}, py::arg("rounds") = 4,
      py::arg("seed") = 0x5eed5eedu, py::arg("groups") = std::vector<std::string>{}, py::arg("inject") = py::none(),
      py::arg("corrupt_expected") = py::none(),
      "Memory part of the deep CU check, on cu_sweep's grid and stream: all 4 waves of every visit run the selected groups "
      "(gload, l1, gstore, buffer, lds, ldstr, ldsdma, atomic: nanogpu/selftest_mem_host.h lists each one's instructions) on a "
      "read-only table of table_words words, on their quarter of the workgroup's slice_bytes of scratch memory and on LDS, and "
      "compare every result word with the value computed from its index. `seed` is accepted and not used: the part's data are "
      "fixed. Records are (xcc, hw_id, fail bits: bit w is wave w; SIMD ids seen; failed-group bits; first bad group, its lowest "
      "bad index and that index's wave, or -1). The index of a result word is k * 64 + lane, in l1 the table word. `groups` in "
      "the result names the bits, `checked` what ran; num_regs and scratch_bytes are the kernel's attributes as the runtime "
      "reports them. inject = (xcc, cu_key, group, index) flips bit 0 of the value that index is compared with on that CU, on "
      "wave index % 4 (tests; no held data is touched). Test hook: corrupt_expected = ('gload' | 'l1' | 'ldsdma', word 0..8191, "
      "xor) XORs one word of the table in this call's upload only.");
  m.def(
      "mem_lanes",
      [](const std::string& group) { return mem_lanes(kMemNames.index(group)); },
      py::arg("group"), py::call_guard<py::gil_scoped_release>(),
      "One workgroup of four waves runs memory group `group`: every lane's raw result words [wave][k][lane].");
  m.def(
      "mem_sensitivity",
      &mem_sensitivity,
      py::arg("device"), py::arg("group"), py::arg("flips"), py::arg("cu_mask") = std::vector<uint32_t>{},
      py::arg("rounds") = 1, py::arg("seed") = 0x5eed5eedu,
      "Test hook: for every (word, xor) of `flips` one cu_sweep_mem of `group` (gload, l1 or ldsdma) alone with that word of the "
      "table corrupted, all on one session. words[i] = (AND, OR) over that sweep's records of (fail bits, failed-group bits, "
      "first bad group or -1, its lowest bad index or -1); records = workgroups per sweep, seconds = the loop's wall time.");
  m.def(
      "mem_info",
      [](int dev) {
        size_t free_b = 0, total_b = 0;
        HIP_OK(hipSetDevice(dev));
        HIP_OK(hipMemGetInfo(&free_b, &total_b));
        return py::make_tuple(free_b, total_b);
      },
      py::arg("device") = 0, "(free bytes, total bytes) of the device's memory.");
}
