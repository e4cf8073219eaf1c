// A matrix tenant with real memory traffic, for the interference calibration: C[M][N] (fp32) = A[M][K] . B[K][N],
// A and B bf16 and row-major, through HBM, the XCD's L2 and LDS. Its K sets its arithmetic intensity: at K = 64 it
// streams C, at K = 4096 it is bound by the matrix unit. nanogpu/gemm_host.h holds the tile sizes, the shape rules,
// the workgroup-to-tile map and every index formed here; native/tests/gemm_host_main.cpp checks them on the CPU.

namespace gm = nanogpu::gemm;

// ---------------------------------------------------------------------------- kernels

using u16x8 = __attribute__((ext_vector_type(8))) unsigned short;
using bf16x4 = __attribute__((ext_vector_type(4))) __bf16;

// One workgroup of 256 threads owns a 128 x 128 tile of C, each wave a 64 x 64 quadrant in four f32x16
// accumulators. K goes through two LDS stages of 64: the 16-byte global loads of tile t + 1 are issued before the
// 16 MFMAs of tile t and written to the other stage after them, with one barrier a tile. A lies in LDS row-major
// with its 16-byte chunks XOR-swizzled, read with ds_read_b128. B lies row-major as in memory, rows padded to
// 320 bytes, and the eight consecutive k of one column that a lane needs come from two ds_read_b64_tr_b16: a
// transposed write would cost 32 two-byte LDS stores a thread and tile. No tail code: the host admits only shapes
// the tiles divide (gm::shape_ok), so every access lies inside A, B or C. No loop but the one over K / 64.
__global__ __launch_bounds__(gm::kThreads, 2) void gemm_bf16_kernel(const uint16_t* __restrict__ A,
                                                                    const uint16_t* __restrict__ B,
                                                                    float* __restrict__ C, int m, int n, int k) {
  __shared__ __attribute__((aligned(16))) uint16_t lds[gm::kLdsElems];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t tile = gm::tile_of_block(blockIdx.x, gridDim.x);
  const gm::TileAt at = gm::tile_at(tile, m, n);
  const int tm = at.m, tn = at.n;
  const int k_tiles = k / gm::kBK;

  u16x8 ra[gm::kLoadPasses], rb[gm::kLoadPasses];
  auto load_global = [&](int kt) {
#pragma unroll
    for (int i = 0; i < gm::kLoadPasses; ++i) {
      ra[i] = *reinterpret_cast<const u16x8*>(A + gm::a_global_index(tm, kt, k, tid, i));
      rb[i] = *reinterpret_cast<const u16x8*>(B + gm::b_global_index(tn, kt, n, tid, i));
    }
  };
  auto store_lds = [&](int stage) {
#pragma unroll
    for (int i = 0; i < gm::kLoadPasses; ++i) {
      *reinterpret_cast<u16x8*>(&lds[gm::a_lds_index(stage, gm::a_load_row(tid, i), gm::a_load_chunk(tid))]) = ra[i];
      *reinterpret_cast<u16x8*>(&lds[gm::b_lds_index(stage, gm::b_load_row(tid, i), gm::kChunk * gm::b_load_chunk(tid))]) = rb[i];
    }
  };
  auto read_tr = [&](int index) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
        (__attribute__((address_space(3))) bf16x4*)reinterpret_cast<bf16x4*>(&lds[index]));
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
    for (int s = 0; s < gm::kBK / 16; ++s) {
      bf16x8 a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) a[i] = *reinterpret_cast<const bf16x8*>(&lds[gm::a_read_index(stage, wave, lane, s, i)]);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const bf16x4 lo = read_tr(gm::b_read_index(stage, wave, lane, s, j, 0));
        const bf16x4 hi = read_tr(gm::b_read_index(stage, wave, lane, s, j, 1));
        b[j] = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
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
      for (int reg = 0; reg < 16; ++reg) C[gm::c_index(tm, tn, n, wave, lane, i, j, reg)] = acc[i][j][reg];
}

// Operands of a tenant: +-1/8 .. +-1 in eighths from a hash of the index. bf16 holds them exactly; none is zero,
// subnormal, infinite or NaN. A grid-stride loop over a bounded grid.
constexpr unsigned kFillBlocks = 1024;
__global__ __launch_bounds__(256) void gemm_fill_kernel(uint16_t* __restrict__ p, size_t count, uint32_t seed) {
  for (size_t i = static_cast<size_t>(blockIdx.x) * 256 + threadIdx.x; i < count; i += static_cast<size_t>(kFillBlocks) * 256) {
    const uint32_t h = st::mix32(static_cast<uint32_t>(i) ^ static_cast<uint32_t>(i >> 32) ^ seed);
    const float v = 0.125f * static_cast<float>((h & 7u) + 1u);
    const __bf16 b = static_cast<__bf16>((h & 8u) ? -v : v);
    p[i] = __builtin_bit_cast(uint16_t, b);
  }
}

// ---------------------------------------------------------------------------- host

// Refused before any allocation or launch: a shape the tiles do not divide, and a launch or an iteration count
// that reaches HIP's 2^32 work-items.
void check_gemm(const char* who, long long m, long long n, long long k, long long iters) {
  if (!gm::shape_ok(m, n, k))
    throw std::invalid_argument(std::string(who) + ": M and N are positive multiples of 128 and K of 64, and M N / 128^2 stays below 2^24 workgroups");
  if (iters <= 0 || static_cast<uint64_t>(iters) * gm::kThreads >= gm::kWorkItemLimit)
    throw std::invalid_argument(std::string(who) + ": iterations in 1..2^24 - 1");
}

void gemm_launch(hipStream_t s, const uint16_t* a, const uint16_t* b, float* c, int m, int n, int k) {
  hipLaunchKernelGGL(gemm_bf16_kernel, dim3(static_cast<unsigned>(gm::tiles(m, n))), dim3(gm::kThreads), 0, s, a, b, c, m, n, k);
}

void gemm_fill(hipStream_t s, uint16_t* p, size_t count, uint32_t seed) {
  hipLaunchKernelGGL(gemm_fill_kernel, dim3(kFillBlocks), dim3(256), 0, s, p, count, seed);
}

double gemm_tflops(int m, int n, int k, int iters, double ms) {
  return 2.0 * m * n * k * iters / (ms * 1e-3) / 1e12;
}

// The numerics entry: small shapes only, so that it cannot serve as a burn.
std::vector<float> gemm_bf16(const std::vector<float>& a, const std::vector<float>& b, int m, int n, int k, int dev) {
  check_gemm("gemm_bf16", m, n, k, 1);
  if (m > 1024 || n > 1024 || k > 1024) throw std::invalid_argument("gemm_bf16: M, N and K at most 1024");
  if (a.size() != static_cast<size_t>(m) * k || b.size() != static_cast<size_t>(k) * n)
    throw std::invalid_argument("gemm_bf16: a holds M x K and b holds K x N values");
  HIP_OK(hipSetDevice(dev));
  std::vector<uint16_t> ha(a.size()), hb(b.size());
  for (size_t i = 0; i < a.size(); ++i) ha[i] = st::f32_to_bf16_bits(a[i]);
  for (size_t i = 0; i < b.size(); ++i) hb[i] = st::f32_to_bf16_bits(b[i]);
  DevBuf<uint16_t> da(ha.size()), db(hb.size());
  std::vector<float> c(static_cast<size_t>(m) * n);
  DevBuf<float> dc(c.size());
  HIP_OK(hipMemcpy(da.p, ha.data(), ha.size() * 2, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(db.p, hb.data(), hb.size() * 2, hipMemcpyHostToDevice));
  HIP_OK(hipMemset(dc.p, 0xff, c.size() * 4));   // NaN wherever the kernel does not write
  gemm_launch(nullptr, da.p, db.p, dc.p, m, n, k);
  HIP_OK(hipGetLastError());
  HIP_OK(hipMemcpy(c.data(), dc.p, c.size() * 4, hipMemcpyDeviceToHost));
  return c;
}

// The operand type of a GEMM tenant, "bf16" or "fp8" (gemm_fp8_kernel, probe_gemm_fp8.inc); anything else is refused.
bool gemm_is_fp8(const char* who, const std::string& dtype) {
  if (dtype != "bf16" && dtype != "fp8") throw std::invalid_argument(std::string(who) + ": dtype is 'bf16' or 'fp8'");
  return dtype == "fp8";
}

// The checked tenant of either type: every refusal comes before any allocation or launch.
Tenant gemm_tenant(const char* who, int dev, const std::vector<uint32_t>& mask, int m, int n, int k, int iters, bool fp8) {
  (fp8 ? check_gemm_fp8 : check_gemm)(who, m, n, k, iters);
  HIP_OK(hipSetDevice(dev));
  return fp8 ? Tenant::gemm_fp8(mask, m, n, k, iters) : Tenant::gemm(mask, m, n, k, iters);
}

py::dict gemm_throughput(int dev, const std::vector<uint32_t>& mask, int m, int n, int k, int iters, const std::string& dtype) {
  double ms = 0.0, tflops = 0.0;
  const bool fp8 = gemm_is_fp8("gemm_throughput", dtype);
  {
    py::gil_scoped_release nogil;
    std::vector<Tenant> tenants;
    tenants.push_back(gemm_tenant("gemm_throughput", dev, mask, m, n, k, iters, fp8));
    tflops = run_tenants(tenants)[0];
    ms = tenants[0].ev.ms();
  }
  py::dict d;
  d["ms"] = ms;
  d["tflops"] = tflops;
  d["gbs"] = (fp8 ? nanogpu::gemm_fp8::compulsory_bytes(m, n, k) : gm::compulsory_bytes(m, n, k)) * iters / (ms * 1e-3) / 1e9;
  d["m"] = m;
  d["n"] = n;
  d["k"] = k;
  d["iters"] = iters;
  d["dtype"] = dtype;
  return d;
}

// A matrix tenant next to a streaming one: the GEMM on `gemm_mask` and an HBM copy on `hbm_mask`, enqueued
// together on their own CU-masked streams, each timed by its own events. The caller sizes which outlasts the
// other: the shorter one is the one measured entirely beside its neighbour. Returns {GEMM TFLOP/s, copy GB/s}.
std::vector<double> gemm_colocated(int dev, const std::vector<uint32_t>& gemm_mask, const std::vector<uint32_t>& hbm_mask,
                                   int m, int n, int k, int gemm_iters, size_t bytes, int hbm_iters, const std::string& dtype) {
  const bool fp8 = gemm_is_fp8("gemm_colocated", dtype);
  const size_t count = bytes / sizeof(float4);
  if (count == 0 || hbm_iters <= 0) throw std::invalid_argument("gemm_colocated: bytes and hbm_iters must be positive");
  const unsigned grid = copy_grid(count);
  std::vector<Tenant> tenants;
  tenants.push_back(gemm_tenant("gemm_colocated", dev, gemm_mask, m, n, k, gemm_iters, fp8));
  tenants.push_back(Tenant::copy(hbm_mask, count, grid, hbm_iters));
  return run_tenants(tenants);
}
