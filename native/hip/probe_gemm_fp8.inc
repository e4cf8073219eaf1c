// The FP8 matrix tenant of the interference calibration: C[M][N] (fp32) = A[M][K] . B^T, A e4m3 [M][K] and B e4m3
// [N][K] as a server stores a weight matrix, through HBM, the XCD's L2 and LDS onto v_mfma_scale_f32_32x32x64_f8f6f4
// with unit scales. It differs from the bf16 tenant (probe_gemm.inc) in its operand type and in nothing else: the
// same tile of C, the same walk over the tiles, fp32 C. nanogpu/gemm_fp8_host.h holds the tile sizes, the shape
// rules and every index formed here; native/tests/gemm_fp8_host_main.cpp checks them on the CPU.

namespace g8 = nanogpu::gemm_fp8;

// ---------------------------------------------------------------------------- kernels

using u32x4 = __attribute__((ext_vector_type(4))) uint32_t;
using i32x8v = __attribute__((ext_vector_type(8))) int;

// E8M0 code of 2^0, in the byte of the scale register that opsel 0 selects, for A and for B.
constexpr int kUnitScale = 127;

// One workgroup of 256 threads owns a 128 x 128 tile of C, each wave a 64 x 64 quadrant in four f32x16
// accumulators. K goes through two LDS stages of 128: the 16-byte global loads of tile t + 1 (four of A, four of B
// a thread) are issued before the 8 MFMAs of tile t and written to the other stage after them, with one barrier a
// tile. Both operands are K-contiguous, so both lie in LDS as 128-byte rows with their 16-byte chunks XOR-swizzled
// and are read with ds_read_b128, two reads an operand: a lane's 32 consecutive k (g8::read_index says why that
// order is sound with unit scales, and only with them). No tail code: the host admits only shapes the tiles divide
// (g8::shape_ok), so every access lies inside A, B or C. No loop but the one over K / 128.
__global__ __launch_bounds__(g8::kThreads, 2) void gemm_fp8_kernel(const uint8_t* __restrict__ A, const uint8_t* __restrict__ B,
                                                                   float* __restrict__ C, int m, int n, int k) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[g8::kLdsBytes];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t tile = gm::tile_of_block(blockIdx.x, gridDim.x);
  const gm::TileAt at = gm::tile_at(tile, m, n);
  const int tm = at.m, tn = at.n;
  const int k_tiles = k / g8::kBK;

  u32x4 ra[g8::kLoadPasses], rb[g8::kLoadPasses];
  auto load_global = [&](int kt) {
#pragma unroll
    for (int i = 0; i < g8::kLoadPasses; ++i) {
      ra[i] = *reinterpret_cast<const u32x4*>(A + g8::global_index(tm, kt, k, tid, i));
      rb[i] = *reinterpret_cast<const u32x4*>(B + g8::global_index(tn, kt, k, tid, i));
    }
  };
  auto store_lds = [&](int stage) {
#pragma unroll
    for (int i = 0; i < g8::kLoadPasses; ++i) {
      *reinterpret_cast<u32x4*>(&lds[g8::lds_index(0, stage, g8::load_row(tid, i), g8::load_chunk(tid))]) = ra[i];
      *reinterpret_cast<u32x4*>(&lds[g8::lds_index(1, stage, g8::load_row(tid, i), g8::load_chunk(tid))]) = rb[i];
    }
  };
  // one operand of one MFMA: the lane's 32 bytes, as the instruction's eight dwords
  auto read_operand = [&](int operand, int stage, int s, int ij) {
    const u32x4 lo = *reinterpret_cast<const u32x4*>(&lds[g8::read_index(operand, stage, wave, lane, s, ij, 0)]);
    const u32x4 hi = *reinterpret_cast<const u32x4*>(&lds[g8::read_index(operand, stage, wave, lane, s, ij, 1)]);
    return i32x8v{int(lo[0]), int(lo[1]), int(lo[2]), int(lo[3]), int(hi[0]), int(hi[1]), int(hi[2]), int(hi[3])};
  };

  f32x16 acc[2][2] = {};
  load_global(0);
  store_lds(0);
  __syncthreads();
  for (int kt = 0; kt < k_tiles; ++kt) {
    const int stage = kt & 1;
    const bool more = kt + 1 < k_tiles;
    if (more) load_global(kt + 1);
#pragma unroll
    for (int s = 0; s < g8::kKSteps; ++s) {
      i32x8v a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) a[i] = read_operand(0, stage, s, i);
#pragma unroll
      for (int j = 0; j < 2; ++j) b[j] = read_operand(1, stage, s, j);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a[i], b[j], acc[i][j], 0, 0, 0, kUnitScale, 0, kUnitScale);
    }
    // the other stage was last read before the barrier that ended tile kt - 1
    if (more) store_lds(stage ^ 1);
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) C[g8::c_index(tm, tn, n, wave, lane, i, j, reg)] = acc[i][j][reg];
}

// Operands of a tenant, four codes a thread and step: e4m3 of +-1/8 .. +-1 in eighths from a hash of the word's
// index, looked up in a table of eight codes (byte v of kEighths is (v + 1) / 8), so no float is converted on the
// device. None is zero, subnormal or NaN. `words` is the operand's size in bytes over four: K is a multiple of 128.
constexpr uint64_t kEighths = 0x38363432302c2820ull;
__global__ __launch_bounds__(256) void gemm_fp8_fill_kernel(uint32_t* __restrict__ p, size_t words, uint32_t seed) {
  for (size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; i < words; i += static_cast<size_t>(kFillBlocks) * 256) {
    const uint32_t h = st::mix32(static_cast<uint32_t>(i) ^ static_cast<uint32_t>(i >> 32) ^ seed);
    uint32_t word = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const uint32_t nibble = h >> (4 * b);
      const uint32_t code = static_cast<uint32_t>(kEighths >> (8 * (nibble & 7u))) & 0xffu;
      word |= (code | ((nibble & 8u) << 4)) << (8 * b);
    }
    p[i] = word;
  }
}

// ---------------------------------------------------------------------------- host

// Refused before any allocation or launch, as check_gemm refuses.
void check_gemm_fp8(const char* who, long long m, long long n, long long k, long long iters) {
  if (!g8::shape_ok(m, n, k))
    throw std::invalid_argument(std::string(who) + ": for fp8, M, N and K are positive multiples of 128, and M N / 128^2 stays below 2^24 workgroups");
  if (iters <= 0 || static_cast<uint64_t>(iters) * g8::kThreads >= gm::kWorkItemLimit)
    throw std::invalid_argument(std::string(who) + ": iterations in 1..2^24 - 1");
}

void gemm_fp8_launch(hipStream_t s, const uint8_t* a, const uint8_t* b, float* c, int m, int n, int k) {
  hipLaunchKernelGGL(gemm_fp8_kernel, dim3(static_cast<unsigned>(gm::tiles(m, n))), dim3(g8::kThreads), 0, s, a, b, c, m, n, k);
}

Tenant Tenant::gemm_fp8(const std::vector<uint32_t>& mask, int m, int n, int k, int iters) {
  Tenant t{Stream(mask), Events(), iters};
  t.kind = Kind::kGemmFp8;
  t.gemm_m = m, t.gemm_n = n, t.gemm_k = k;
  const size_t na = static_cast<size_t>(m) * k, nb = static_cast<size_t>(n) * k;
  t.fa = DevBuf<uint8_t>(na, OomIsBadAlloc{});
  t.fb = DevBuf<uint8_t>(nb, OomIsBadAlloc{});
  t.gc = DevBuf<float>(static_cast<size_t>(m) * n, OomIsBadAlloc{});
  hipLaunchKernelGGL(gemm_fp8_fill_kernel, dim3(kFillBlocks), dim3(256), 0, t.st.s, reinterpret_cast<uint32_t*>(t.fa.p), na / 4, 0xa11ce5edu);
  hipLaunchKernelGGL(gemm_fp8_fill_kernel, dim3(kFillBlocks), dim3(256), 0, t.st.s, reinterpret_cast<uint32_t*>(t.fb.p), nb / 4, 0xb0b5eedu);
  return t;
}

// e4m3 codes as the caller holds them: a one-dimensional contiguous uint8 buffer, read as it lies, or a list of ints.
std::vector<uint8_t> fp8_codes(const py::object& x) {
  if (!py::isinstance<py::buffer>(x)) return x.cast<std::vector<uint8_t>>();
  const py::buffer_info info = x.cast<py::buffer>().request();
  if (info.itemsize != 1 || info.format != py::format_descriptor<uint8_t>::format() || info.ndim != 1 || info.strides[0] != 1)
    throw std::invalid_argument("gemm_fp8: a buffer must be one contiguous dimension of uint8");
  const uint8_t* p = static_cast<const uint8_t*>(info.ptr);
  return std::vector<uint8_t>(p, p + info.shape[0]);
}

// The numerics entry: small shapes only, so that it cannot serve as a burn. The codes reach the device as they are.
std::vector<float> gemm_fp8(const py::object& a_codes, const py::object& b_codes, int m, int n, int k, int dev) {
  check_gemm_fp8("gemm_fp8", m, n, k, 1);
  if (m > 1024 || n > 1024 || k > 1024) throw std::invalid_argument("gemm_fp8: M, N and K at most 1024");
  const std::vector<uint8_t> a = fp8_codes(a_codes), b = fp8_codes(b_codes);
  if (a.size() != static_cast<size_t>(m) * k || b.size() != static_cast<size_t>(n) * k)
    throw std::invalid_argument("gemm_fp8: a_codes holds M x K and b_codes N x K codes");
  std::vector<float> c(static_cast<size_t>(m) * n);
  py::gil_scoped_release nogil;
  HIP_OK(hipSetDevice(dev));
  DevBuf<uint8_t> da(a.size()), db(b.size());
  DevBuf<float> dc(c.size());
  HIP_OK(hipMemcpy(da.p, a.data(), a.size(), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(db.p, b.data(), b.size(), hipMemcpyHostToDevice));
  HIP_OK(hipMemset(dc.p, 0xff, c.size() * 4));   // NaN wherever the kernel does not write
  gemm_fp8_launch(nullptr, da.p, db.p, dc.p, m, n, k);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpy(c.data(), dc.p, c.size() * 4, hipMemcpyDeviceToHost));
  return c;
}
