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

// ---- scalar sweep (host) ----

const std::vector<uint32_t>& scalar_table() {   // computed once
  static const std::vector<uint32_t> table = ss::expected_table();
  return table;
}
const std::vector<uint32_t>& scalar_loads() {
  static const std::vector<uint32_t> table = ss::smem_table();
  return table;
}

static_assert(ss::kNoBad == st::kNoBadOffset, "or_minus1's 'none' word");

// The scalar part (PartSession). `sregs` names its registers, so no slot can have been spilled, but a
// kernel that reports scratch is refused that part all the same, as ValuPart refuses `regs`.
struct ScalarPart {
  static constexpr const char* who = "cu_sweep_scalar";
  static constexpr const char* sensitivity_who = "scalar_sensitivity";
  static constexpr NameTable names{ss::kNumNames, ss::group_name, "scalar group"};
  static constexpr uint32_t kAllGroups = ss::kAllGroups;
  static constexpr int kRecordWords = ss::kScalarRecordWords;
  static constexpr auto kernel = cu_scalar_kernel;
  static constexpr size_t kSliceBytes = 0;
  template <int G>
  static constexpr LanesKernel group_kernel = scalar_words_kernel<G>;

  // inject of cu_sweep_scalar: (xcc, cu_key, 'scalar', group) | (xcc, cu_key, 'smem', word) | (xcc, cu_key, 'sregs', slot).
  using Inject = ScalarInject;
  static Inject parse_inject(const py::object& inject) {
    Inject inj;
    const py::tuple t = inject_head(inject, 4, 4, "cu_sweep_scalar: inject = (xcc, cu_key, kind, arg)", inj);
    if (t.empty()) return inj;
    const std::string kind = t[2].cast<std::string>();
    if (kind == "scalar") {
      inj.kind = kScalarInjectGroup;
      inj.arg = names.index(t[3].cast<std::string>());
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

  static std::vector<const std::vector<uint32_t>*> tables() { return {&scalar_table(), &scalar_loads()}; }
  static constexpr const char* flip_usage = "cu_sweep_scalar: corrupt_expected = (group | 'smem', word, xor)";
  static FlipTarget flip_target(int table) {
    if (table > ss::kSmem) throw std::invalid_argument("corrupt_expected: an exact group's name, or 'smem'");
    if (table == ss::kSmem) return {1, 0, ss::kSmemWords};
    return {0, static_cast<size_t>(table) * ss::kGroupWords, ss::kGroupWords};
  }
  static void check(uint32_t groups, const hipFuncAttributes& attr) {
    refuse_scratch(who, names, ss::kSregs, groups, attr);
    require_block_fits(who, kernel);
  }

  static void launch(hipStream_t stream, int blocks, const Uploads& up, uint8_t*, uint32_t* out, uint32_t seed, const Inject& j,
                     uint32_t groups) {
    hipLaunchKernelGGL(cu_scalar_kernel, dim3(blocks), dim3(kSweepBlock), 0, stream, up[0]->p(), up[1]->p(), out, seed, j, groups);
  }

  static py::tuple record_tuple(const uint32_t* words, int b) {
    const ss::ScalarRecord rec = ss::decode_scalar_record(words, b);
    return py::make_tuple(rec.xcc, rec.hw_id, rec.fail, rec.simds, rec.groups, or_minus1(rec.bad_index), or_minus1(rec.bad_wave),
                          or_minus1(rec.bad_which));
  }
  static void extras(py::dict& d, const hipFuncAttributes& attr) {
    d["sreg_slots"] = ss::kSregSlots;
    d["num_regs"] = attr.numRegs;   // hipFuncAttributes has no count of scalar registers
  }

  // Per word the fields fail, failed-group bits and first bad index (a table word of 'smem'), of a sweep over
  // every exact group and 'smem'.
  static uint32_t sensitivity_groups(int) { return ss::kAllExact | 1u << ss::kSmem; }
  static constexpr uint32_t kSensitivityMinus1 = 1u << 2;
  static std::array<uint32_t, 3> sensitivity_fields(const uint32_t* words, int b) {
    const ss::ScalarRecord rec = ss::decode_scalar_record(words, b);
    return {rec.fail, rec.groups, rec.bad_index};
  }
};

// Exact group g on one workgroup of four waves: its raw words [wave][word].
std::vector<uint32_t> scalar_words(int g) {
  if (g < 0 || g >= ss::kNumExact) throw std::invalid_argument("scalar_words: an exact group");
  return one_workgroup_words(ss::kGroupWords, [&](uint32_t* out) {
    hipLaunchKernelGGL(kernel_of<ScalarPart>(ScalarExact{}, g), dim3(1), dim3(kSweepBlock), 0, 0, out);
  });
}

