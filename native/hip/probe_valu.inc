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

using LanesKernel = void (*)(uint32_t*);
static_assert(sv::kNoBad == st::kNoBadOffset, "or_minus1's 'none' word");

// The vector-ALU part (PartSession). A register test that spills to scratch would test memory, so `regs` is
// refused when the kernel reports scratch.
struct ValuPart {
  static constexpr const char* who = "cu_sweep_valu";
  static constexpr const char* sensitivity_who = "valu_sensitivity";
  static constexpr NameTable names{sv::kNumNames, sv::group_name, "vector-ALU group"};
  static constexpr uint32_t kAllGroups = sv::kAllGroups;
  static constexpr int kRecordWords = sv::kValuRecordWords;
  static constexpr auto kernel = cu_valu_kernel;
  static constexpr size_t kSliceBytes = 0;
  template <int G>
  static constexpr LanesKernel group_kernel = valu_lanes_kernel<G>;

  // inject of cu_sweep_valu: (xcc, cu_key, 'valu', group) | (xcc, cu_key, 'regs', slot) | (xcc, cu_key, 'approx').
  using Inject = ValuInject;
  static Inject parse_inject(const py::object& inject) {
    Inject inj;
    const py::tuple t = inject_head(inject, 3, 4, "cu_sweep_valu: inject = (xcc, cu_key, kind[, arg])", inj);
    if (t.empty()) return inj;
    const std::string kind = t[2].cast<std::string>();
    if (kind == "valu" && t.size() == 4) {
      inj.kind = kValuInjectGroup;
      inj.arg = names.index(t[3].cast<std::string>());
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

  static std::vector<const std::vector<uint32_t>*> tables() { return {&valu_table()}; }
  static constexpr const char* flip_usage = "cu_sweep_valu: corrupt_expected = (group, word, xor)";
  static FlipTarget flip_target(int table) {
    if (table >= sv::kNumExact) throw std::invalid_argument("corrupt_expected: an exact group's name");
    return {0, static_cast<size_t>(table) * sv::kGroupWords, sv::kGroupWords};
  }
  static void check(uint32_t groups, const hipFuncAttributes& attr) { refuse_scratch(who, names, sv::kRegs, groups, attr); }

  static void launch(hipStream_t stream, int blocks, const Uploads& up, uint8_t*, uint32_t* out, uint32_t seed, const Inject& j,
                     uint32_t groups) {
    hipLaunchKernelGGL(cu_valu_kernel, dim3(blocks), dim3(kSweepBlock), 0, stream, up[0]->p(), out, seed, j, groups);
  }

  static py::tuple record_tuple(const uint32_t* words, int b) {
    const sv::ValuRecord rec = sv::decode_valu_record(words, b);
    return py::make_tuple(rec.xcc, rec.hw_id, rec.fail, rec.simds, rec.groups, or_minus1(rec.bad_slot), or_minus1(rec.bad_thread),
                          rec.approx_hash);
  }
  static void extras(py::dict& d, const hipFuncAttributes& attr) {
    d["reg_slots"] = sv::kRegSlots;
    d["regs_per_lane"] = attr.numRegs;
  }

  // Per word the fields fail and failed-group bits, of a sweep over every exact group.
  static uint32_t sensitivity_groups(int) { return sv::kAllExact; }
  static constexpr uint32_t kSensitivityMinus1 = 0;
  static std::array<uint32_t, 2> sensitivity_fields(const uint32_t* words, int b) {
    const sv::ValuRecord rec = sv::decode_valu_record(words, b);
    return {rec.fail, rec.groups};
  }
};

// Group g (an exact group or approx) on one wave: its raw words.
std::vector<uint32_t> valu_lanes(int g) {
  if (g < 0 || g > sv::kApprox) throw std::invalid_argument("valu_lanes: an exact group or 'approx'");
  const size_t n = g == sv::kApprox ? sv::kNumApprox * sv::kLanes : sv::kGroupWords;
  return one_workgroup_words(n, [&](uint32_t* out) {
    hipLaunchKernelGGL(kernel_of<ValuPart>(std::make_integer_sequence<int, sv::kApprox + 1>{}, g), dim3(1), dim3(64), 0, 0, out);
  });
}

