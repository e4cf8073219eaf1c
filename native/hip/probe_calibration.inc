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
// dependent-accumulator latency; each MFMA is 2*32*32*16 = 32768 FLOP. kStoreSums = false is the
// timed kernel, which never stores on a healthy device; true stores every thread's sum, so that a
// test can check the arithmetic burn_tflops charges for (mfma_burn_sums).
template <bool kStoreSums>
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
  if (kStoreSums || s == 12345.678f) out[blockIdx.x * blockDim.x + threadIdx.x] = s;  // keeps the chains live
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

// ---------------------------------------------------------------------------- host helpers

// DevBuf, Stream and Events own HIP handles: they move and never copy, and abandon() gives a handle
// up without freeing it (peer_bandwidth after a timeout).
struct OomIsBadAlloc {};

template <class T>
struct DevBuf {
  T* p = nullptr;
  DevBuf() = default;
  explicit DevBuf(size_t n) { HIP_OK(hipMalloc(&p, n * sizeof(T))); }
  // An allocation that does not fit is the caller's to shrink, not a device fault.
  DevBuf(size_t n, OomIsBadAlloc) {
    const hipError_t e = hipMalloc(&p, n * sizeof(T));
    if (e == hipErrorOutOfMemory) {
      (void)hipGetLastError();
      throw std::bad_alloc();
    }
    HIP_OK(e);
  }
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)) {}
  DevBuf& operator=(DevBuf&& o) noexcept {
    std::swap(p, o.p);
    return *this;
  }
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
  void abandon() { p = nullptr; }
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
  for (size_t i = 0; i < a.size(); ++i) ha[i] = st::f32_to_bf16_bits(a[i]);
  for (size_t i = 0; i < b.size(); ++i) hb[i] = st::f32_to_bf16_bits(b[i]);
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
  Stream(const Stream&) = delete;
  Stream& operator=(const Stream&) = delete;
  Stream(Stream&& o) noexcept : s(std::exchange(o.s, nullptr)) {}
  Stream& operator=(Stream&& o) noexcept {
    std::swap(s, o.s);
    return *this;
  }
  ~Stream() {
    if (s) (void)hipStreamDestroy(s);
  }
  void abandon() { s = nullptr; }
};

struct Events {
  hipEvent_t a = nullptr, b = nullptr;
  Events() {
    HIP_OK(hipEventCreate(&a));
    HIP_OK(hipEventCreate(&b));
  }
  Events(const Events&) = delete;
  Events& operator=(const Events&) = delete;
  Events(Events&& o) noexcept : a(std::exchange(o.a, nullptr)), b(std::exchange(o.b, nullptr)) {}
  Events& operator=(Events&& o) noexcept {
    std::swap(a, o.a);
    std::swap(b, o.b);
    return *this;
  }
  ~Events() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
  void abandon() { a = b = nullptr; }
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

// One tenant of a device in a rate probe: a stream under its CU mask (empty: every CU) with its own
// events, and the work it repeats there: `iters` launches of an HBM copy of n float4, or one launch of an
// MFMA burn of `blocks` blocks that loops `iters` times. The callers have checked the shapes.
struct Tenant {
  Stream st;
  Events ev;
  int iters;
  size_t n = 0;   // a copy: n > 0
  unsigned grid = 0;
  DevBuf<float4> src, dst;
  int blocks = 0;   // a burn
  DevBuf<float> out;

  static Tenant copy(const std::vector<uint32_t>& mask, size_t n, unsigned grid, int iters) {
    Tenant t{Stream(mask), Events(), iters};
    t.n = n;
    t.grid = grid;
    t.src = DevBuf<float4>(n);
    t.dst = DevBuf<float4>(n);
    // on the tenant's own stream, which does not wait for the null stream: ordered before the warm-up
    HIP_OK(hipMemsetAsync(t.src.p, 0, n * sizeof(float4), t.st.s));
    return t;
  }
  static Tenant burn(const std::vector<uint32_t>& mask, int blocks, int iters) {
    Tenant t{Stream(mask), Events(), iters};
    t.blocks = blocks;
    t.out = DevBuf<float>(static_cast<size_t>(blocks) * 256);
    return t;
  }
  void copy_once() const { hipLaunchKernelGGL(hbm_copy, dim3(grid), dim3(kCopyBlock), 0, st.s, src.p, dst.p, n); }
  void burn_once(int loops) const {
    hipLaunchKernelGGL(mfma_burn<false>, dim3(blocks), dim3(256), 0, st.s, out.p, loops);
  }
  void warm_up() const { n ? copy_once() : burn_once(8); }
  void enqueue_timed() const {
    HIP_OK(hipEventRecord(ev.a, st.s));
    if (n)
      for (int i = 0; i < iters; ++i) copy_once();
    else
      burn_once(iters);
    HIP_OK(hipEventRecord(ev.b, st.s));
  }
  double rate() { return n ? copy_gbs(n, iters, ev.ms()) : burn_tflops(blocks, iters, ev.ms()); }
};

// The one procedure behind the rate probes. Every tenant warms up and the device drains; then the timed
// work of all of them is enqueued back to back, so that they run together, each between its own events.
// Launch errors are read after the loops: nothing stands between two timed launches.
std::vector<double> run_tenants(std::vector<Tenant>& tenants) {
  for (const Tenant& t : tenants) t.warm_up();
  HIP_OK(hipGetLastError());
  HIP_OK(hipDeviceSynchronize());
  for (const Tenant& t : tenants) t.enqueue_timed();
  HIP_OK(hipGetLastError());
  std::vector<double> rates;
  for (Tenant& t : tenants) rates.push_back(t.rate());
  return rates;
}

double hbm_bandwidth(int dev, size_t bytes, int iters) {
  HIP_OK(hipSetDevice(dev));
  const size_t n = bytes / sizeof(float4);
  if (n == 0 || iters <= 0) throw std::invalid_argument("hbm_bandwidth: bytes/iters must be positive");
  const unsigned grid = copy_grid(n);
  std::vector<Tenant> tenants;
  tenants.push_back(Tenant::copy({}, n, grid, iters));
  return run_tenants(tenants)[0];
}

py::list census(int dev, const std::vector<uint32_t>& mask, int blocks, int sleep_iters) {
  HIP_OK(hipSetDevice(dev));
  if (blocks <= 0 || blocks > (1 << 20)) throw std::invalid_argument("census: bad block count");
  DevBuf<uint32_t> out(static_cast<size_t>(blocks) * 3);
  Stream st(mask);
  HIP_OK(hipMemsetAsync(out.p, 0xff, static_cast<size_t>(blocks) * 3 * sizeof(uint32_t), st.s));
  hipLaunchKernelGGL(cu_census, dim3(blocks), dim3(64), 0, st.s, out.p, sleep_iters);
  HIP_OK(hipGetLastError());
  HIP_OK(hipStreamSynchronize(st.s));
  std::vector<uint32_t> h(static_cast<size_t>(blocks) * 3);
  HIP_OK(hipMemcpy(h.data(), out.p, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  py::list res;
  for (int i = 0; i < blocks; ++i) res.append(py::make_tuple(h[3 * i], h[3 * i + 1]));
  return res;
}

py::dict mfma_throughput(int dev, const std::vector<uint32_t>& mask, int blocks, int iters) {
  double ms = 0.0, tflops = 0.0;
  {
    py::gil_scoped_release nogil;  // device work without the GIL; py objects built after
    HIP_OK(hipSetDevice(dev));
    if (blocks <= 0 || iters <= 0) throw std::invalid_argument("mfma_throughput: bad shape");
    check_burn_blocks(blocks);
    std::vector<Tenant> tenants;
    tenants.push_back(Tenant::burn(mask, blocks, iters));
    tflops = run_tenants(tenants)[0];
    ms = tenants[0].ev.ms();
  }
  py::dict d;
  d["ms"] = ms;
  d["tflops"] = tflops;
  d["blocks"] = blocks;
  d["iters"] = iters;
  return d;
}

// One launch of the checking instantiation of mfma_burn: every thread's sum, [block][thread].
// Small shapes only, so that it cannot serve as a burn.
std::vector<float> mfma_burn_sums(int dev, int blocks, int iters) {
  if (blocks < 1 || blocks > 8 || iters < 1 || iters > 1024)
    throw std::invalid_argument("mfma_burn_sums: blocks in 1..8, iters in 1..1024");
  HIP_OK(hipSetDevice(dev));
  const size_t n = static_cast<size_t>(blocks) * 256;
  DevBuf<float> out(n);
  HIP_OK(hipMemset(out.p, 0xff, n * sizeof(float)));
  hipLaunchKernelGGL(mfma_burn<true>, dim3(blocks), dim3(256), 0, 0, out.p, iters);
  HIP_OK(hipGetLastError());
  std::vector<float> h(n);
  HIP_OK(hipMemcpy(h.data(), out.p, n * sizeof(float), hipMemcpyDeviceToHost));
  return h;
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
  for (int b : blocks) check_burn_blocks(b);
  std::vector<Tenant> tenants;
  for (size_t i = 0; i < masks.size(); ++i) tenants.push_back(Tenant::burn(masks[i], blocks[i], iters));
  return run_tenants(tenants);
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
  const unsigned grid = copy_grid(n);
  std::vector<Tenant> tenants;
  for (size_t i = 0; i < k; ++i) tenants.push_back(Tenant::copy(masks[i], n, grid, iters_each[i]));
  return run_tenants(tenants);
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
  const unsigned grid = copy_grid(n);
  check_burn_blocks(mfma_blocks);
  std::vector<Tenant> tenants;   // the burn first: it is under way when the first timed copy starts
  tenants.push_back(Tenant::burn(mfma_mask, mfma_blocks, mfma_iters));
  tenants.push_back(Tenant::copy(hbm_mask, n, grid, iters));
  const std::vector<double> rates = run_tenants(tenants);
  return {rates[1], rates[0]};
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
  // A transfer that missed the deadline abandons what it holds and never frees it (see PeerTimeout).
  HIP_OK(hipSetDevice(src));
  DevBuf<float4> a(n);
  Stream ss({});
  HIP_OK(hipMemsetAsync(a.p, 0, n * sizeof(float4), ss.s));
  hipEvent_t fill = nullptr;
  HIP_OK(hipEventCreateWithFlags(&fill, hipEventDisableTiming));
  HIP_OK(hipEventRecord(fill, ss.s));
  const bool filled = wait_event(fill, deadline);
  (void)hipEventDestroy(fill);
  if (!filled) {
    a.abandon(), ss.abandon();
    throw PeerTimeout("peer_bandwidth: the source fill on GPU " + std::to_string(src) + " did not finish");
  }
  HIP_OK(hipSetDevice(dst));
  DevBuf<float4> b(n);
  Stream st({});
  Events ev;
  auto timed = [&](const char* what, auto&& enqueue) -> double {   // seconds of `enqueue`'s work
    HIP_OK(hipEventRecord(ev.a, st.s));
    enqueue();
    HIP_OK(hipEventRecord(ev.b, st.s));
    if (!wait_event(ev.b, deadline)) {
      a.abandon(), b.abandon(), ss.abandon(), st.abandon(), ev.abandon();
      throw PeerTimeout(std::string("peer_bandwidth ") + std::to_string(src) + "->" + std::to_string(dst) + ": " +
                        what + " did not finish within " + std::to_string(deadline_s) + " s");
    }
    float ms = 0.f;
    HIP_OK(hipEventElapsedTime(&ms, ev.a, ev.b));
    return ms * 1e-3;
  };
  const double nb = static_cast<double>(n * sizeof(float4));
  timed("SDMA warm-up", [&] { HIP_OK(hipMemcpyPeerAsync(b.p, dst, a.p, src, n * sizeof(float4), st.s)); });
  r.dma_gbs = nb * iters / timed("SDMA copies", [&] {
    for (int i = 0; i < iters; ++i) HIP_OK(hipMemcpyPeerAsync(b.p, dst, a.p, src, n * sizeof(float4), st.s));
  }) / 1e9;
  if (r.peer_access) {
    timed("pull warm-up", [&] {
      hipLaunchKernelGGL(hbm_copy, grid, dim3(kCopyBlock), 0, st.s, a.p, b.p, n);
      HIP_OK(hipGetLastError());
    });
    r.pull_gbs = nb * iters / timed("pull copies", [&] {
      for (int i = 0; i < iters; ++i) hipLaunchKernelGGL(hbm_copy, grid, dim3(kCopyBlock), 0, st.s, a.p, b.p, n);
      HIP_OK(hipGetLastError());
    }) / 1e9;
  }
  return r;
}
