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

// ---- sweep and matrix paths (host) ----

constexpr NameTable kPathNames{sp::kNumPaths, sp::path_name, "matrix path"};

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

// cu_sweep (`paths` null: 5-field records) and cu_sweep_paths (7 fields, and the keys `paths` / `checked`).
py::dict sweep_binding(int dev, const std::vector<uint32_t>& mask, int rounds, uint32_t seed,
                       const std::vector<std::string>* paths, const py::object& inject, const py::object& corrupt_expected,
                       std::optional<size_t> lds_bytes) {
  const uint32_t bits = paths ? kPathNames.bits(*paths) : 0u;
  if (paths && !bits) throw std::invalid_argument("cu_sweep_paths: no path selected");
  const SweepInject inj = parse_inject(inject, paths != nullptr);
  const WordFlip flip = paths ? parse_flip(corrupt_expected, &kPathNames, "bf16", "cu_sweep_paths: corrupt_expected = ('bf16' | path name, word, xor)")
                              : parse_flip(corrupt_expected, nullptr, nullptr, "cu_sweep: corrupt_expected = (word, xor)");
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

// Per word the fields fail, lds_bad, path_fail and path_waves (the last two 0 when `paths` is empty).
py::dict sweep_sensitivity(int dev, const std::string& tile, const std::vector<std::pair<uint32_t, uint32_t>>& flips,
                           const std::vector<std::string>& paths, const std::vector<uint32_t>& mask, int rounds, uint32_t seed) {
  const uint32_t bits = kPathNames.bits(paths);
  const int t = table_index(kPathNames, "bf16", tile);
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
