// Host/device-shared arithmetic of the deep self-test's scalar part (native/hip/probe_scalar.inc:
// cu_scalar_kernel, scalar_words_kernel). Plain C++ with no HIP dependency: the stand-alone program
// native/tests/selftest_scalar_host_main.cpp builds it on its own, also under ASan + UBSan. The
// Python twin, in plain integers, is nanogpu/probe/selftest_scalar.py.
//
// Every exact group is one chain of kWaveWords steps per wave. A step runs every instruction of the
// group once on the step's operands and folds each result, with the SCC the instruction left, into
// a running word h; the step's result word is h, so a wrong result reaches every later word of its
// wave. The operands are scalar_operand(group, step, wave, k): a fixed function, not seeded, and
// the four waves compute different words: one table of kNumExact x 4 x 8 words.
//
// The chains are written once, as templates over an `Ops` type: the kernel instantiates them with
// one inline-assembly statement per instruction (an SCC producer shares its statement with the
// s_cselect_b32 that reads SCC), the host with HostOps below. Instructions the groups reach:
//   add    s_add_u32 + s_addc_u32 and s_sub_u32 + s_subb_u32 (64-bit pairs), s_add_u32, s_sub_u32,
//          s_add_i32, s_sub_i32, s_min_i32, s_max_i32, s_min_u32, s_max_u32, s_absdiff_i32, s_abs_i32
//   mul    s_mul_i32, s_mul_hi_u32, s_mul_hi_i32, s_lshl1_add_u32 .. s_lshl4_add_u32
//   shift  s_lshl_b32, s_lshr_b32, s_ashr_i32, s_lshl_b64, s_lshr_b64, s_ashr_i64, s_bfm_b32, s_bfm_b64
//   logic  s_and, s_or, s_xor, s_nand, s_nor, s_xnor, s_andn2, s_orn2, s_not, each _b32 and _b64
//   bits   s_bfe_u32, s_bfe_i32, s_bfe_u64, s_bfe_i64, s_brev_b32, s_brev_b64, s_bcnt0_i32_b32,
//          s_bcnt1_i32_b32, s_bcnt0_i32_b64, s_bcnt1_i32_b64, s_ff0_i32_b32, s_ff1_i32_b32,
//          s_ff0_i32_b64, s_ff1_i32_b64, s_flbit_i32_b32, s_flbit_i32_b64, s_flbit_i32,
//          s_flbit_i32_i64, s_bitset0_b32, s_bitset1_b32, s_sext_i32_i8, s_sext_i32_i16,
//          s_pack_ll_b32_b16, s_pack_lh_b32_b16, s_pack_hh_b32_b16
//   cmp    s_cmp_{eq,lg,gt,ge,lt,le}_{i32,u32}, s_cmp_eq_u64, s_cmp_lg_u64, s_bitcmp0_b32,
//          s_bitcmp1_b32, each consumed once by s_cselect_b32, s_cselect_b64 or s_cmov_b32 and once by
//          s_cbranch_scc0 or s_cbranch_scc1 over one s_mov_b32
//   vcc    v_cmp_lt_u32 into an SGPR pair (the ballot, ANDed with EXEC), s_bcnt1_i32_b64, s_ff1_i32_b64,
//          v_readfirstlane_b32, v_cndmask_b32 under an SGPR-pair mask, an SGPR as a VALU source
//          (builtins: the compiler chooses the encodings)
//   smem   s_load_dword, _dwordx2, _dwordx4, _dwordx8, _dwordx16
//   sregs  s_mul_i32, s_xor_b32, s_cmp_lg_u32, s_cselect_b32, s_or_b32 on named registers
//
// Why the host's words are the one right answer: every instruction here is integer arithmetic whose
// result and SCC the CDNA ISA states in full for the operands used. Operand corners the chains keep
// away from, because the written definition leaves them open or this project has not established
// it (the README lists them under "Not covered"): s_min / s_max with equal operands (which one SCC
// names), s_abs_i32 and s_absdiff_i32 where the magnitude is 2^31 or the difference overflows,
// s_lshlN_add_u32 with a bit shifted out of S0, shift and bit-field counts beyond the operand's
// width (32-bit shifts get 0..31, 64-bit 0..63; every extract has offset + width inside the
// operand and a width of at least 1), find-first and find-leading-bit of an operand without the bit
// sought (the -1 result).
#pragma once

#include <cstdint>
#include <vector>

#include "nanogpu/selftest_host.h"

namespace nanogpu {
namespace selftest {
namespace scalar {

constexpr int kWaves = 4;
constexpr int kWaveWords = 8;                       // steps of a chain, and result words per wave
constexpr int kGroupWords = kWaves * kWaveWords;    // [wave][word]

// The order is the bit order of the records.
enum Group : int { kAdd = 0, kMul, kShift, kLogic, kBits, kCmp, kVcc, kNumExact, kSmem = kNumExact, kSregs, kNumNames };
constexpr uint32_t kAllExact = (1u << kNumExact) - 1;
constexpr uint32_t kAllGroups = (1u << kNumNames) - 1;
constexpr int kTableWords = kNumExact * kGroupWords;   // 224

inline const char* group_name(int g) {
  static const char* const names[kNumNames] = {"add", "mul", "shift", "logic", "bits", "cmp", "vcc", "smem", "sregs"};
  return g >= 0 && g < kNumNames ? names[g] : "?";
}

NANOGPU_HD inline uint32_t scalar_operand(int g, int s, int wave, int k) {
  return mix32(0x5ca1a2b3u ^ (static_cast<uint32_t>(g) << 24) ^ (static_cast<uint32_t>(s) << 16) ^
               (static_cast<uint32_t>(wave) << 8) ^ static_cast<uint32_t>(k));
}
NANOGPU_HD inline uint32_t rotl32(uint32_t x, int r) { return (x << (r & 31)) | (x >> ((32 - r) & 31)); }
// One result d and the SCC c it came with, into the running word.
NANOGPU_HD inline uint32_t fold(uint32_t h, uint32_t d, uint32_t c) { return rotl32(h ^ d, 7) + c + 0x9e3779b9u; }
NANOGPU_HD inline uint32_t fold64(uint32_t h, uint64_t d, uint32_t c) {
  return fold(fold(h, static_cast<uint32_t>(d), c), static_cast<uint32_t>(d >> 32), 0u);
}
NANOGPU_HD inline uint64_t pair64(uint32_t hi, uint32_t lo) { return (static_cast<uint64_t>(hi) << 32) | lo; }

constexpr int kZeroStep = 5;    // the step whose operands make every "result is nonzero" SCC 0
constexpr int kEqualStep = 2;   // the step of cmp whose operands are equal

// ---- the chains -------------------------------------------------------------------------
// `out(s, h)` takes step s's result word: the host stores it, the kernel compares it at once, so
// that no chain keeps an indexed array.
// The instruction first, then its SCC: two statements, because the order in which a call's
// arguments are evaluated is the compiler's.
#define NANOGPU_FOLD(call)       \
  do {                           \
    const uint32_t d_ = (call);  \
    h = fold(h, d_, c);          \
  } while (0)
#define NANOGPU_FOLD64(call)     \
  do {                           \
    const uint64_t d_ = (call);  \
    h = fold64(h, d_, c);        \
  } while (0)
template <class Ops, class Out>
NANOGPU_HD inline void chain_add(Ops& o, int wave, Out&& out) {
  uint32_t h = scalar_operand(kAdd, 0, wave, 15), c = 0;
  for (int s = 0; s < kWaveWords; ++s) {
    const uint32_t a = scalar_operand(kAdd, s, wave, 0), p = scalar_operand(kAdd, s, wave, 2), q = scalar_operand(kAdd, s, wave, 3);
    const uint32_t b = s == kZeroStep ? a : scalar_operand(kAdd, s, wave, 1);
    NANOGPU_FOLD(o.add_u32(a, b, c));
    NANOGPU_FOLD(o.sub_u32(a, b, c));
    NANOGPU_FOLD64(o.add64(pair64(a, p), pair64(b, q), c));
    NANOGPU_FOLD64(o.sub64(pair64(p, a), pair64(q, b), c));
    NANOGPU_FOLD(o.add_i32(a, b, c));
    NANOGPU_FOLD(o.sub_i32(p, b, c));
    NANOGPU_FOLD(o.min_i32(a, p, c));      // never equal operands: p is another hash
    NANOGPU_FOLD(o.max_i32(a, p, c));
    NANOGPU_FOLD(o.min_u32(q, a, c));
    NANOGPU_FOLD(o.max_u32(q, a, c));
    const uint32_t ha = static_cast<uint32_t>(static_cast<int32_t>(a) >> 1), hb = static_cast<uint32_t>(static_cast<int32_t>(b) >> 1);
    NANOGPU_FOLD(o.absdiff_i32(ha, hb, c));    // |operands| <= 2^30: the difference cannot overflow
    NANOGPU_FOLD(o.abs_i32(s == kZeroStep ? 0u : ha, c));
    out(s, h);
  }
}

template <class Ops, class Out>
NANOGPU_HD inline void chain_mul(Ops& o, int wave, Out&& out) {
  uint32_t h = scalar_operand(kMul, 0, wave, 15), c = 0;
  for (int s = 0; s < kWaveWords; ++s) {
    const uint32_t a = scalar_operand(kMul, s, wave, 0), b = scalar_operand(kMul, s, wave, 1), p = scalar_operand(kMul, s, wave, 2);
    h = fold(h, o.mul_i32(a, b), 0u);
    h = fold(h, o.mul_hi_u32(a, b), 0u);
    h = fold(h, o.mul_hi_i32(a, b), 0u);
    h = fold(h, o.mul_hi_i32(p, a), 0u);
    NANOGPU_FOLD(o.lshl1_add_u32(a >> 1, p, c));   // no bit leaves S0
    NANOGPU_FOLD(o.lshl2_add_u32(b >> 2, p, c));
    NANOGPU_FOLD(o.lshl3_add_u32(p >> 3, a, c));
    NANOGPU_FOLD(o.lshl4_add_u32(a >> 4, b, c));
    out(s, h);
  }
}

NANOGPU_HD inline uint32_t shift_amount32(int s, uint32_t u) { return s == 0 ? 0u : s == 1 ? 1u : s == 2 ? 31u : u & 31u; }
NANOGPU_HD inline uint32_t shift_amount64(int s, uint32_t u) {
  return s == 0 ? 0u : s == 1 ? 31u : s == 2 ? 32u : s == 3 ? 63u : (u >> 8) & 63u;
}

template <class Ops, class Out>
NANOGPU_HD inline void chain_shift(Ops& o, int wave, Out&& out) {
  uint32_t h = scalar_operand(kShift, 0, wave, 15), c = 0;
  for (int s = 0; s < kWaveWords; ++s) {
    const bool z = s == kZeroStep;
    const uint32_t a = z ? 0u : scalar_operand(kShift, s, wave, 0), b = z ? 0u : scalar_operand(kShift, s, wave, 1);
    const uint32_t u = scalar_operand(kShift, s, wave, 2), v = scalar_operand(kShift, s, wave, 3);
    const uint32_t n = shift_amount32(s, u), m = shift_amount64(s, u);
    const uint64_t x = pair64(a, b);
    NANOGPU_FOLD(o.lshl_b32(a, n, c));
    NANOGPU_FOLD(o.lshr_b32(a, n, c));
    NANOGPU_FOLD(o.ashr_i32(a, n, c));
    NANOGPU_FOLD64(o.lshl_b64(x, m, c));
    NANOGPU_FOLD64(o.lshr_b64(x, m, c));
    NANOGPU_FOLD64(o.ashr_i64(x, m, c));
    h = fold(h, o.bfm_b32(v & 31u, (v >> 8) & 31u), 0u);
    h = fold64(h, o.bfm_b64((v >> 16) & 63u, (v >> 24) & 63u), 0u);
    out(s, h);
  }
}

template <class Ops, class Out>
NANOGPU_HD inline void chain_logic(Ops& o, int wave, Out&& out) {
  uint32_t h = scalar_operand(kLogic, 0, wave, 15), c = 0;
  for (int s = 0; s < kWaveWords; ++s) {
    const bool z = s == kZeroStep;   // operands whose result is 0, per instruction
    const uint32_t a = scalar_operand(kLogic, s, wave, 0), b = scalar_operand(kLogic, s, wave, 1);
    const uint64_t x = pair64(scalar_operand(kLogic, s, wave, 2), a), y = pair64(scalar_operand(kLogic, s, wave, 3), b);
    NANOGPU_FOLD(o.and_b32(a, z ? ~a : b, c));
    NANOGPU_FOLD(o.or_b32(z ? 0u : a, z ? 0u : b, c));
    NANOGPU_FOLD(o.xor_b32(a, z ? a : b, c));
    NANOGPU_FOLD(o.nand_b32(z ? ~0u : a, z ? ~0u : b, c));
    NANOGPU_FOLD(o.nor_b32(a, z ? ~a : b, c));
    NANOGPU_FOLD(o.xnor_b32(a, z ? ~a : b, c));
    NANOGPU_FOLD(o.andn2_b32(a, z ? a : b, c));
    NANOGPU_FOLD(o.orn2_b32(z ? 0u : a, z ? ~0u : b, c));
    NANOGPU_FOLD(o.not_b32(z ? ~0u : a, c));
    NANOGPU_FOLD64(o.and_b64(x, z ? ~x : y, c));
    NANOGPU_FOLD64(o.or_b64(z ? 0u : x, z ? 0u : y, c));
    NANOGPU_FOLD64(o.xor_b64(x, z ? x : y, c));
    NANOGPU_FOLD64(o.nand_b64(z ? ~uint64_t(0) : x, z ? ~uint64_t(0) : y, c));
    NANOGPU_FOLD64(o.nor_b64(x, z ? ~x : y, c));
    NANOGPU_FOLD64(o.xnor_b64(x, z ? ~x : y, c));
    NANOGPU_FOLD64(o.andn2_b64(x, z ? x : y, c));
    NANOGPU_FOLD64(o.orn2_b64(z ? 0u : x, z ? ~uint64_t(0) : y, c));
    NANOGPU_FOLD64(o.not_b64(z ? ~uint64_t(0) : y, c));
    out(s, h);
  }
}

// S1 of s_bfe: offset in bits 5:0 (4:0 for 32 bits), width in 22:16. offset + width stays inside the operand.
NANOGPU_HD inline uint32_t bfe_field32(uint32_t u) {
  const uint32_t off = u & 31u;
  return off | ((1u + (u >> 8) % (32u - off)) << 16);
}
NANOGPU_HD inline uint32_t bfe_field64(uint32_t u) {
  const uint32_t off = (u >> 16) & 63u;
  return off | ((1u + (u >> 24) % (64u - off)) << 16);
}

template <class Ops, class Out>
NANOGPU_HD inline void chain_bits(Ops& o, int wave, Out&& out) {
  uint32_t h = scalar_operand(kBits, 0, wave, 15), c = 0;
  for (int s = 0; s < kWaveWords; ++s) {
    const bool z = s == kZeroStep;
    const uint32_t a = z ? 0u : scalar_operand(kBits, s, wave, 0), b = z ? 0u : scalar_operand(kBits, s, wave, 1);
    const uint32_t u = scalar_operand(kBits, s, wave, 2), p = scalar_operand(kBits, s, wave, 3);
    const uint64_t x = pair64(a, b);
    NANOGPU_FOLD(o.bfe_u32(a, bfe_field32(u), c));
    NANOGPU_FOLD(o.bfe_i32(a, bfe_field32(p), c));
    NANOGPU_FOLD64(o.bfe_u64(x, bfe_field64(u), c));
    NANOGPU_FOLD64(o.bfe_i64(x, bfe_field64(p), c));
    h = fold(h, o.brev_b32(a), 0u);
    h = fold64(h, o.brev_b64(x), 0u);
    NANOGPU_FOLD(o.bcnt0_i32_b32(~a, c));
    NANOGPU_FOLD(o.bcnt1_i32_b32(a, c));
    NANOGPU_FOLD(o.bcnt0_i32_b64(~x, c));
    NANOGPU_FOLD(o.bcnt1_i32_b64(x, c));
    h = fold(h, o.ff0_i32_b32(a & 0x7fffffffu), 0u);                  // a zero exists
    h = fold(h, o.ff1_i32_b32(a | 0x80000000u), 0u);                  // a one exists
    h = fold(h, o.ff0_i32_b64(x & ~(uint64_t(1) << 63)), 0u);
    h = fold(h, o.ff1_i32_b64(x | (uint64_t(1) << 63)), 0u);
    h = fold(h, o.flbit_i32_b32(a | 1u), 0u);
    h = fold(h, o.flbit_i32_b64(x | 1u), 0u);
    h = fold(h, o.flbit_i32((a & ~1u) | (~a >> 31)), 0u);             // bit 0 is unlike the sign
    h = fold(h, o.flbit_i32_i64((x & ~uint64_t(1)) | (~x >> 63)), 0u);
    h = fold(h, o.bitset0_b32(p, u & 31u), 0u);
    h = fold(h, o.bitset1_b32(p, (u >> 8) & 31u), 0u);
    h = fold(h, o.sext_i32_i8(p), 0u);
    h = fold(h, o.sext_i32_i16(u), 0u);
    h = fold(h, o.pack_ll_b32_b16(p, u), 0u);
    h = fold(h, o.pack_lh_b32_b16(p, u), 0u);
    h = fold(h, o.pack_hh_b32_b16(p, u), 0u);
    out(s, h);
  }
}

// Every compare of the cmp group, X(name, relation of (a, b) as the host computes it). The 32-bit
// ones take a, b; the 64-bit ones the pairs; the bit compares a and a bit number.
#define NANOGPU_SCALAR_CMP32(X)                                                                                  \
  X(eq_i32, a == b) X(lg_i32, a != b) X(gt_i32, static_cast<int32_t>(a) > static_cast<int32_t>(b))               \
  X(ge_i32, static_cast<int32_t>(a) >= static_cast<int32_t>(b)) X(lt_i32, static_cast<int32_t>(a) < static_cast<int32_t>(b)) \
  X(le_i32, static_cast<int32_t>(a) <= static_cast<int32_t>(b)) X(eq_u32, a == b) X(lg_u32, a != b) X(gt_u32, a > b) \
  X(ge_u32, a >= b) X(lt_u32, a < b) X(le_u32, a <= b) X(bitcmp0_b32, ((a >> (b & 31u)) & 1u) == 0u)              \
  X(bitcmp1_b32, ((a >> (b & 31u)) & 1u) == 1u)
#define NANOGPU_SCALAR_CMP64(X) X(eq_u64, a == b) X(lg_u64, a != b)

// sel_NAME(a, b, x, y) and br_NAME(a, b, x, y) both give SCC ? x : y, through a select and through a branch.
template <class Ops, class Out>
NANOGPU_HD inline void chain_cmp(Ops& o, int wave, Out&& out) {
  uint32_t h = scalar_operand(kCmp, 0, wave, 15);
  for (int s = 0; s < kWaveWords; ++s) {
    const uint32_t a = scalar_operand(kCmp, s, wave, 0), b = s == kEqualStep ? a : scalar_operand(kCmp, s, wave, 1);
    const uint32_t x = scalar_operand(kCmp, s, wave, 2), y = scalar_operand(kCmp, s, wave, 3);
    const uint32_t ah = scalar_operand(kCmp, s, wave, 4), bh = s == kEqualStep ? ah : (s & 1) ? ah : scalar_operand(kCmp, s, wave, 5);
#define NANOGPU_X(name, rel)              \
  h = fold(h, o.sel_##name(a, b, x, y), 0u); \
  h = fold(h, o.br_##name(b, a, y, x), 0u);
    NANOGPU_SCALAR_CMP32(NANOGPU_X)
#undef NANOGPU_X
#define NANOGPU_X(name, rel)                                        \
  h = fold(h, o.sel_##name(pair64(ah, a), pair64(bh, b), x, y), 0u); \
  h = fold(h, o.br_##name(pair64(a, ah), pair64(b, bh), y, x), 0u);
    NANOGPU_SCALAR_CMP64(NANOGPU_X)
#undef NANOGPU_X
    out(s, h);
  }
}

#undef NANOGPU_FOLD
#undef NANOGPU_FOLD64

// ---- vcc: the boundary between the vector and the scalar unit -----------------------------
// Step s of wave w, with the wave's running word h (uniform): lane l holds v = mix32(u0 ^ l * kHiMul).
//   mask = the lanes with v < thr            (a vector compare into an SGPR pair, ANDed with EXEC)
//   cnt = ones of mask, ff = lowest one of mask | 2^63   (64-bit count and find-first)
//   r = lane 0's v ^ h                        (v_readfirstlane_b32)
//   w = lane l of the pair m ? v + k : v ^ k  (v_cndmask_b32 under an SGPR pair; k an SGPR source)
//   mask2 = the lanes with w < k
constexpr int kLanes = 64;
NANOGPU_HD inline uint32_t vcc_lane_value(uint32_t u0, int lane) { return mix32(u0 ^ static_cast<uint32_t>(lane) * kHiMul); }
NANOGPU_HD inline uint32_t vcc_fold(uint32_t h, uint64_t mask, uint32_t cnt, uint32_t ff, uint32_t r, uint64_t mask2) {
  h = fold(h, static_cast<uint32_t>(mask), cnt);
  h = fold(h, static_cast<uint32_t>(mask >> 32), ff);
  h = fold(h, r, 0u);
  return fold64(h, mask2, 0u);
}

inline void vcc_expected(int wave, uint32_t* out) {
  uint32_t h = scalar_operand(kVcc, 0, wave, 15);
  for (int s = 0; s < kWaveWords; ++s) {
    const uint32_t u0 = scalar_operand(kVcc, s, wave, 0), thr = scalar_operand(kVcc, s, wave, 1), k = scalar_operand(kVcc, s, wave, 4);
    const uint64_t m = pair64(scalar_operand(kVcc, s, wave, 3), scalar_operand(kVcc, s, wave, 2));
    uint64_t mask = 0, mask2 = 0;
    uint32_t cnt = 0;
    for (int l = 0; l < kLanes; ++l) {
      const uint32_t v = vcc_lane_value(u0, l);
      if (v < thr) mask |= uint64_t(1) << l, ++cnt;
      const uint32_t w = ((m >> l) & 1u) ? v + k : v ^ k;
      if (w < k) mask2 |= uint64_t(1) << l;
    }
    uint32_t ff = 0;
    while (!(((mask | (uint64_t(1) << 63)) >> ff) & 1u)) ++ff;
    h = vcc_fold(h, mask, cnt, ff, vcc_lane_value(u0, 0) ^ h, mask2);
    out[s] = h;
  }
}

// ---- smem ---------------------------------------------------------------------------------
// A read-only table of kSmemWords words; wave w reads quarter w, in five spans, one per load width.
constexpr int kSmemWords = 4096;
constexpr int kSmemQuarter = kSmemWords / kWaves;
constexpr uint32_t kSmemSalt = 0x51ed270bu;
NANOGPU_HD inline uint32_t smem_word(uint32_t index) { return mix32(index ^ kSmemSalt); }
// Words of a quarter each width reads, in the order x16, x8, x4, x2, x1 (about a fifth each).
constexpr int kSmemSpanX16 = 320, kSmemSpanX8 = 256, kSmemSpanX4 = 192, kSmemSpanX2 = 128, kSmemSpanX1 = 128;
static_assert(kSmemSpanX16 + kSmemSpanX8 + kSmemSpanX4 + kSmemSpanX2 + kSmemSpanX1 == kSmemQuarter, "the spans tile a quarter");
static_assert(kSmemSpanX16 % 32 == 0 && kSmemSpanX8 % 16 == 0 && kSmemSpanX4 % 16 == 0 && kSmemSpanX2 % 8 == 0 && kSmemSpanX1 % 4 == 0,
              "whole statements: 2 loads of x16 and x8, 4 of x4, x2 and x1");

inline std::vector<uint32_t> smem_table() {
  std::vector<uint32_t> t(kSmemWords);
  for (int i = 0; i < kSmemWords; ++i) t[i] = smem_word(static_cast<uint32_t>(i));
  return t;
}

// ---- sregs --------------------------------------------------------------------------------
// Slot i is register s(12 + i). Pass 0 holds key * odd_i ^ c_i, pass 1 the complement; key = seed ^ wave.
constexpr int kSregSlots = 88;
constexpr int kSregFirst = 12;
constexpr int kSregFlags = 3;
NANOGPU_HD inline uint32_t sreg_odd(uint32_t slot) { return 0x9e3779b1u + 2u * slot; }
NANOGPU_HD inline uint32_t sreg_const(uint32_t slot) { return 0x7f4a7c15u + 0x01000193u * slot; }
NANOGPU_HD inline uint32_t sreg_word(uint32_t slot, uint32_t key, uint32_t pass) {
  const uint32_t v = key * sreg_odd(slot) ^ sreg_const(slot);
  return pass ? ~v : v;
}

// ---- record -------------------------------------------------------------------------------
// xcc, hw_id of wave 0, fail (bits 0..3 exact groups of wave w, 4..7 smem, 8..11 sregs), SIMD ids
// seen, failed exact-group bits, first bad index (sregs slot before smem word) or kNoBad, its wave,
// which of the two it was (kBadSregs | kBadSmem) or kNoBad.
constexpr int kScalarRecordWords = 8;
constexpr uint32_t kNoBad = 0xffffffffu;
constexpr int kFailExactShift = 0, kFailSmemShift = 4, kFailSregsShift = 8;
constexpr uint32_t kBadSregs = 0, kBadSmem = 1;
NANOGPU_HD inline uint32_t pack_bad(uint32_t which, uint32_t index, uint32_t wave) { return (which << 24) | (index << 8) | wave; }

struct ScalarRecord {
  uint32_t xcc, hw_id, fail, simds, groups, bad_index, bad_wave, bad_which;
};

inline ScalarRecord decode_scalar_record(const uint32_t* words, size_t block) {
  const uint32_t* w = words + block * static_cast<size_t>(kScalarRecordWords);
  return ScalarRecord{w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]};
}

// ---- host arithmetic ------------------------------------------------------------------------
// Every instruction whose SCC a chain consumes, and every compare through both consumers.
#define NANOGPU_SCALAR_SCC(X)                                                                                       \
  X(add_u32) X(sub_u32) X(addc_u32) X(subb_u32) X(add_i32) X(sub_i32) X(min_i32) X(max_i32) X(min_u32) X(max_u32)   \
  X(absdiff_i32) X(abs_i32) X(lshl1_add_u32) X(lshl2_add_u32) X(lshl3_add_u32) X(lshl4_add_u32) X(lshl_b32)         \
  X(lshr_b32) X(ashr_i32) X(lshl_b64) X(lshr_b64) X(ashr_i64) X(and_b32) X(or_b32) X(xor_b32) X(nand_b32)           \
  X(nor_b32) X(xnor_b32) X(andn2_b32) X(orn2_b32) X(not_b32) X(and_b64) X(or_b64) X(xor_b64) X(nand_b64) X(nor_b64) \
  X(xnor_b64) X(andn2_b64) X(orn2_b64) X(not_b64) X(bfe_u32) X(bfe_i32) X(bfe_u64) X(bfe_i64) X(bcnt0_i32_b32)      \
  X(bcnt1_i32_b32) X(bcnt0_i32_b64) X(bcnt1_i32_b64) X(sel_eq_i32) X(sel_lg_i32) X(sel_gt_i32) X(sel_ge_i32)        \
  X(sel_lt_i32) X(sel_le_i32) X(sel_eq_u32) X(sel_lg_u32) X(sel_gt_u32) X(sel_ge_u32) X(sel_lt_u32) X(sel_le_u32)   \
  X(sel_bitcmp0_b32) X(sel_bitcmp1_b32) X(sel_eq_u64) X(sel_lg_u64) X(br_eq_i32) X(br_lg_i32) X(br_gt_i32)          \
  X(br_ge_i32) X(br_lt_i32) X(br_le_i32) X(br_eq_u32) X(br_lg_u32) X(br_gt_u32) X(br_ge_u32) X(br_lt_u32)           \
  X(br_le_u32) X(br_bitcmp0_b32) X(br_bitcmp1_b32) X(br_eq_u64) X(br_lg_u64)

enum SccId : int {
#define NANOGPU_X(name) kScc_##name,
  NANOGPU_SCALAR_SCC(NANOGPU_X)
#undef NANOGPU_X
      kNumScc
};

inline const char* scc_name(int id) {
  static const char* const names[kNumScc] = {
#define NANOGPU_X(name) #name,
      NANOGPU_SCALAR_SCC(NANOGPU_X)
#undef NANOGPU_X
  };
  return id >= 0 && id < kNumScc ? names[id] : "?";
}

struct Conds {
  int scc[kNumScc][2] = {};          // times the instruction's SCC was consumed as 0 and as 1
  int carry31[2] = {}, carry63[2] = {}, borrow31[2] = {}, borrow63[2] = {};   // not taken, taken
  int overflow_pos = 0, overflow_neg = 0;       // signed add / subtract past 2^31 - 1 and past -2^31
  int equal_operands = 0;                        // compares whose operands were equal
  int abnormal = 0;                              // an operand outside what the header allows
};

struct HostOps {
  Conds c;

  uint32_t note(int id, bool scc) {
    ++c.scc[id][scc ? 1 : 0];
    return scc ? 1u : 0u;
  }
  static int32_t i(uint32_t v) { return static_cast<int32_t>(v); }
  static int64_t i(uint64_t v) { return static_cast<int64_t>(v); }

  // add
  uint32_t add_u32(uint32_t a, uint32_t b, uint32_t& s) {
    s = note(kScc_add_u32, (uint64_t(a) + b) >> 32);
    return a + b;
  }
  uint32_t sub_u32(uint32_t a, uint32_t b, uint32_t& s) {
    s = note(kScc_sub_u32, b > a);
    return a - b;
  }
  uint64_t add64(uint64_t a, uint64_t b, uint32_t& s) {   // s_add_u32 of the low words, s_addc_u32 of the high ones
    const uint64_t lo = (a & 0xffffffffu) + (b & 0xffffffffu);
    const uint32_t c0 = note(kScc_add_u32, lo >> 32);
    ++c.carry31[c0];
    const uint64_t hi = (a >> 32) + (b >> 32) + c0;
    s = note(kScc_addc_u32, hi >> 32);
    ++c.carry63[s];
    return (hi << 32) | (lo & 0xffffffffu);
  }
  uint64_t sub64(uint64_t a, uint64_t b, uint32_t& s) {   // s_sub_u32, s_subb_u32
    const uint32_t al = static_cast<uint32_t>(a), bl = static_cast<uint32_t>(b), ah = static_cast<uint32_t>(a >> 32),
                   bh = static_cast<uint32_t>(b >> 32);
    const uint32_t c0 = note(kScc_sub_u32, bl > al);
    ++c.borrow31[c0];
    s = note(kScc_subb_u32, uint64_t(bh) + c0 > ah);
    ++c.borrow63[s];
    return pair64(ah - bh - c0, al - bl);
  }
  uint32_t add_i32(uint32_t a, uint32_t b, uint32_t& s) {
    const int64_t r = int64_t(i(a)) + i(b);
    if (r > INT32_MAX) ++c.overflow_pos;
    if (r < INT32_MIN) ++c.overflow_neg;
    s = note(kScc_add_i32, r > INT32_MAX || r < INT32_MIN);
    return a + b;
  }
  uint32_t sub_i32(uint32_t a, uint32_t b, uint32_t& s) {
    const int64_t r = int64_t(i(a)) - i(b);
    if (r > INT32_MAX) ++c.overflow_pos;
    if (r < INT32_MIN) ++c.overflow_neg;
    s = note(kScc_sub_i32, r > INT32_MAX || r < INT32_MIN);
    return a - b;
  }
  uint32_t min_i32(uint32_t a, uint32_t b, uint32_t& s) {
    if (a == b) ++c.abnormal;
    s = note(kScc_min_i32, i(a) < i(b));
    return s ? a : b;
  }
  uint32_t max_i32(uint32_t a, uint32_t b, uint32_t& s) {
    if (a == b) ++c.abnormal;
    s = note(kScc_max_i32, i(a) > i(b));
    return s ? a : b;
  }
  uint32_t min_u32(uint32_t a, uint32_t b, uint32_t& s) {
    if (a == b) ++c.abnormal;
    s = note(kScc_min_u32, a < b);
    return s ? a : b;
  }
  uint32_t max_u32(uint32_t a, uint32_t b, uint32_t& s) {
    if (a == b) ++c.abnormal;
    s = note(kScc_max_u32, a > b);
    return s ? a : b;
  }
  uint32_t absdiff_i32(uint32_t a, uint32_t b, uint32_t& s) {
    const int64_t d = int64_t(i(a)) - i(b);
    if (d > INT32_MAX || d < -int64_t(INT32_MAX)) ++c.abnormal;
    const uint32_t r = static_cast<uint32_t>(d < 0 ? -d : d);
    s = note(kScc_absdiff_i32, r != 0);
    return r;
  }
  uint32_t abs_i32(uint32_t a, uint32_t& s) {
    if (a == 0x80000000u) ++c.abnormal;
    const uint32_t r = i(a) < 0 ? 0u - a : a;
    s = note(kScc_abs_i32, r != 0);
    return r;
  }

  // mul
  uint32_t mul_i32(uint32_t a, uint32_t b) { return a * b; }
  uint32_t mul_hi_u32(uint32_t a, uint32_t b) { return static_cast<uint32_t>((uint64_t(a) * b) >> 32); }
  uint32_t mul_hi_i32(uint32_t a, uint32_t b) { return static_cast<uint32_t>(static_cast<uint64_t>(int64_t(i(a)) * i(b)) >> 32); }
  uint32_t lshl_add(int id, int n, uint32_t a, uint32_t b, uint32_t& s) {
    if (a >> (32 - n)) ++c.abnormal;
    const uint64_t r = (uint64_t(a) << n) + b;
    s = note(id, r >> 32);
    return static_cast<uint32_t>(r);
  }
  uint32_t lshl1_add_u32(uint32_t a, uint32_t b, uint32_t& s) { return lshl_add(kScc_lshl1_add_u32, 1, a, b, s); }
  uint32_t lshl2_add_u32(uint32_t a, uint32_t b, uint32_t& s) { return lshl_add(kScc_lshl2_add_u32, 2, a, b, s); }
  uint32_t lshl3_add_u32(uint32_t a, uint32_t b, uint32_t& s) { return lshl_add(kScc_lshl3_add_u32, 3, a, b, s); }
  uint32_t lshl4_add_u32(uint32_t a, uint32_t b, uint32_t& s) { return lshl_add(kScc_lshl4_add_u32, 4, a, b, s); }

  // shift: the callers keep the counts inside the operand
  uint32_t nz(int id, uint32_t r, uint32_t& s) {
    s = note(id, r != 0);
    return r;
  }
  uint64_t nz(int id, uint64_t r, uint32_t& s) {
    s = note(id, r != 0);
    return r;
  }
  uint32_t lshl_b32(uint32_t a, uint32_t n, uint32_t& s) {
    if (n > 31) ++c.abnormal;
    return nz(kScc_lshl_b32, a << (n & 31u), s);
  }
  uint32_t lshr_b32(uint32_t a, uint32_t n, uint32_t& s) {
    if (n > 31) ++c.abnormal;
    return nz(kScc_lshr_b32, a >> (n & 31u), s);
  }
  uint32_t ashr_i32(uint32_t a, uint32_t n, uint32_t& s) {
    if (n > 31) ++c.abnormal;
    const uint32_t fill = (a >> 31) ? ~0u : 0u;
    n &= 31u;
    return nz(kScc_ashr_i32, n ? (a >> n) | (fill << (32 - n)) : a, s);
  }
  uint64_t lshl_b64(uint64_t a, uint32_t n, uint32_t& s) {
    if (n > 63) ++c.abnormal;
    return nz(kScc_lshl_b64, a << (n & 63u), s);
  }
  uint64_t lshr_b64(uint64_t a, uint32_t n, uint32_t& s) {
    if (n > 63) ++c.abnormal;
    return nz(kScc_lshr_b64, a >> (n & 63u), s);
  }
  uint64_t ashr_i64(uint64_t a, uint32_t n, uint32_t& s) {
    if (n > 63) ++c.abnormal;
    const uint64_t fill = (a >> 63) ? ~uint64_t(0) : 0;
    n &= 63u;
    return nz(kScc_ashr_i64, n ? (a >> n) | (fill << (64 - n)) : a, s);
  }
  uint32_t bfm_b32(uint32_t width, uint32_t off) {
    if (width > 31 || off > 31) ++c.abnormal;
    return ((1u << (width & 31u)) - 1u) << (off & 31u);
  }
  uint64_t bfm_b64(uint32_t width, uint32_t off) {
    if (width > 63 || off > 63) ++c.abnormal;
    return ((uint64_t(1) << (width & 63u)) - 1u) << (off & 63u);
  }

  // logic
#define NANOGPU_LOGIC(n32, n64, expr)                                                               \
  uint32_t n32(uint32_t a, uint32_t b, uint32_t& s) { return nz(kScc_##n32, uint32_t(expr), s); } \
  uint64_t n64(uint64_t a, uint64_t b, uint32_t& s) { return nz(kScc_##n64, uint64_t(expr), s); }
  NANOGPU_LOGIC(and_b32, and_b64, a & b)
  NANOGPU_LOGIC(or_b32, or_b64, a | b)
  NANOGPU_LOGIC(xor_b32, xor_b64, a ^ b)
  NANOGPU_LOGIC(nand_b32, nand_b64, ~(a & b))
  NANOGPU_LOGIC(nor_b32, nor_b64, ~(a | b))
  NANOGPU_LOGIC(xnor_b32, xnor_b64, ~(a ^ b))
  NANOGPU_LOGIC(andn2_b32, andn2_b64, a & ~b)
  NANOGPU_LOGIC(orn2_b32, orn2_b64, a | ~b)
#undef NANOGPU_LOGIC
  uint32_t not_b32(uint32_t a, uint32_t& s) { return nz(kScc_not_b32, ~a, s); }
  uint64_t not_b64(uint64_t a, uint32_t& s) { return nz(kScc_not_b64, ~a, s); }

  // bits
  uint64_t extract(uint64_t v, uint32_t field, int bits, bool sign) {
    const uint32_t off = field & (bits - 1u), width = (field >> 16) & 0x7fu;
    if (width == 0 || off + width > static_cast<uint32_t>(bits)) {
      ++c.abnormal;
      return 0;
    }
    uint64_t f = v >> off;
    if (width < 64) f &= (uint64_t(1) << width) - 1;
    if (sign && width < 64 && ((f >> (width - 1)) & 1u)) f |= ~uint64_t(0) << width;
    return bits == 32 ? f & 0xffffffffu : f;
  }
  uint32_t bfe_u32(uint32_t a, uint32_t f, uint32_t& s) { return nz(kScc_bfe_u32, static_cast<uint32_t>(extract(a, f, 32, false)), s); }
  uint32_t bfe_i32(uint32_t a, uint32_t f, uint32_t& s) { return nz(kScc_bfe_i32, static_cast<uint32_t>(extract(a, f, 32, true)), s); }
  uint64_t bfe_u64(uint64_t a, uint32_t f, uint32_t& s) { return nz(kScc_bfe_u64, extract(a, f, 64, false), s); }
  uint64_t bfe_i64(uint64_t a, uint32_t f, uint32_t& s) { return nz(kScc_bfe_i64, extract(a, f, 64, true), s); }
  uint64_t brev(uint64_t v, int bits) {
    uint64_t r = 0;
    for (int k = 0; k < bits; ++k) r |= ((v >> k) & 1u) << (bits - 1 - k);
    return r;
  }
  uint32_t brev_b32(uint32_t a) { return static_cast<uint32_t>(brev(a, 32)); }
  uint64_t brev_b64(uint64_t a) { return brev(a, 64); }
  static uint32_t ones(uint64_t v) {
    uint32_t n = 0;
    for (; v; v &= v - 1) ++n;
    return n;
  }
  uint32_t bcnt0_i32_b32(uint32_t a, uint32_t& s) { return nz(kScc_bcnt0_i32_b32, 32u - ones(a), s); }
  uint32_t bcnt1_i32_b32(uint32_t a, uint32_t& s) { return nz(kScc_bcnt1_i32_b32, ones(a), s); }
  uint32_t bcnt0_i32_b64(uint64_t a, uint32_t& s) { return nz(kScc_bcnt0_i32_b64, 64u - ones(a), s); }
  uint32_t bcnt1_i32_b64(uint64_t a, uint32_t& s) { return nz(kScc_bcnt1_i32_b64, ones(a), s); }
  uint32_t first(uint64_t v, int bits, uint32_t bit, bool from_top) {   // index of the first `bit`, from bit 0 or from the top
    for (int k = 0; k < bits; ++k)
      if (((v >> (from_top ? bits - 1 - k : k)) & 1u) == bit) return static_cast<uint32_t>(k);
    ++c.abnormal;
    return ~0u;
  }
  uint32_t ff0_i32_b32(uint32_t a) { return first(a, 32, 0, false); }
  uint32_t ff1_i32_b32(uint32_t a) { return first(a, 32, 1, false); }
  uint32_t ff0_i32_b64(uint64_t a) { return first(a, 64, 0, false); }
  uint32_t ff1_i32_b64(uint64_t a) { return first(a, 64, 1, false); }
  uint32_t flbit_i32_b32(uint32_t a) { return first(a, 32, 1, true); }
  uint32_t flbit_i32_b64(uint64_t a) { return first(a, 64, 1, true); }
  uint32_t flbit_i32(uint32_t a) { return first(a, 32, (a >> 31) ^ 1u, true); }          // the first bit unlike the sign
  uint32_t flbit_i32_i64(uint64_t a) { return first(a, 64, static_cast<uint32_t>(a >> 63) ^ 1u, true); }
  uint32_t bitset0_b32(uint32_t d, uint32_t n) {
    if (n > 31) ++c.abnormal;
    return d & ~(1u << (n & 31u));
  }
  uint32_t bitset1_b32(uint32_t d, uint32_t n) {
    if (n > 31) ++c.abnormal;
    return d | (1u << (n & 31u));
  }
  uint32_t sext_i32_i8(uint32_t a) { return (a & 0x80u) ? a | 0xffffff00u : a & 0xffu; }
  uint32_t sext_i32_i16(uint32_t a) { return (a & 0x8000u) ? a | 0xffff0000u : a & 0xffffu; }
  uint32_t pack_ll_b32_b16(uint32_t a, uint32_t b) { return (a & 0xffffu) | (b << 16); }
  uint32_t pack_lh_b32_b16(uint32_t a, uint32_t b) { return (a & 0xffffu) | (b & 0xffff0000u); }
  uint32_t pack_hh_b32_b16(uint32_t a, uint32_t b) { return (a >> 16) | (b & 0xffff0000u); }

  // cmp
  uint32_t pick(int id, bool scc, bool equal, uint32_t x, uint32_t y) {
    note(id, scc);
    if (equal) ++c.equal_operands;
    return scc ? x : y;
  }
#define NANOGPU_X(name, rel)                                                                                           \
  uint32_t sel_##name(uint32_t a, uint32_t b, uint32_t x, uint32_t y) { return pick(kScc_sel_##name, rel, a == b, x, y); } \
  uint32_t br_##name(uint32_t a, uint32_t b, uint32_t x, uint32_t y) { return pick(kScc_br_##name, rel, a == b, x, y); }
  NANOGPU_SCALAR_CMP32(NANOGPU_X)
#undef NANOGPU_X
#define NANOGPU_X(name, rel)                                                                                           \
  uint32_t sel_##name(uint64_t a, uint64_t b, uint32_t x, uint32_t y) { return pick(kScc_sel_##name, rel, a == b, x, y); } \
  uint32_t br_##name(uint64_t a, uint64_t b, uint32_t x, uint32_t y) { return pick(kScc_br_##name, rel, a == b, x, y); }
  NANOGPU_SCALAR_CMP64(NANOGPU_X)
#undef NANOGPU_X
};

// Group g's kGroupWords expected words, [wave][word]; `conds` (optional) gets the counters.
inline void group_expected(int g, uint32_t* out, Conds* conds = nullptr) {
  HostOps o;
  for (int wave = 0; wave < kWaves; ++wave) {
    uint32_t* w = out + wave * kWaveWords;
    auto put = [w](int s, uint32_t h) { w[s] = h; };
    switch (g) {
      case kAdd: chain_add(o, wave, put); break;
      case kMul: chain_mul(o, wave, put); break;
      case kShift: chain_shift(o, wave, put); break;
      case kLogic: chain_logic(o, wave, put); break;
      case kBits: chain_bits(o, wave, put); break;
      case kCmp: chain_cmp(o, wave, put); break;
      default: vcc_expected(wave, w); break;
    }
  }
  if (conds) *conds = o.c;
}

inline std::vector<uint32_t> expected_table() {
  std::vector<uint32_t> t(kTableWords);
  for (int g = 0; g < kNumExact; ++g) group_expected(g, t.data() + g * kGroupWords);
  return t;
}

// Bits that are the same in all kGroupWords words of a group.
inline uint32_t uncovered_bits(const uint32_t* words) {
  uint32_t ones = 0, zeros = 0;
  for (int i = 0; i < kGroupWords; ++i) ones |= words[i], zeros |= ~words[i];
  return ~(ones & zeros);
}

}  // namespace scalar
}  // namespace selftest
}  // namespace nanogpu
