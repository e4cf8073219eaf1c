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

  DevBuf<unsigned char> whole(bytes + 2 * guard_bytes, OomIsBadAlloc{});
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
