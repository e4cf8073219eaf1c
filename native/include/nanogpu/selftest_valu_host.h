// Host/device-shared arithmetic of the deep self-test's vector-ALU part (native/hip/probe_valu.inc:
// cu_valu_kernel, valu_lanes_kernel). Plain C++ with no HIP dependency: the stand-alone program
// native/tests/selftest_valu_host_main.cpp builds it on its own, also under ASan + UBSan. The
// Python twin, in integers and fractions, is nanogpu/probe/selftest_valu.py.
//
// Every exact group is a pair of chains of kValuSteps dependent steps per lane (two result words
// per lane, both compared); each step's result is an operand of the next, so a wrong intermediate
// reaches the end. The operands are valu_operand(group, step, lane, k): a fixed function, not
// seeded, so all four waves of every visit share one table of kNumExact x 64 x 2 words.
//
// The chains are written once, as templates over an `Ops` type: the kernel instantiates them with
// the gfx950 builtins, the host with HostOps below. Instructions the groups reach in the gfx950
// code (read once in the generated ISA):
//   fma32     v_fmac_f32 (the two-operand encoding of v_fma_f32)
//   fma64     v_fmac_f64                     pkfma16   v_pk_fma_f16       pkfma32   v_pk_fma_f32
//   addmul32  v_mul_f32, v_add_f32 (separately rounded: no contraction)
//   int32     v_mul_lo_u32, v_mul_hi_u32, v_mad_u64_u32, v_add_co_u32 / v_addc_co_u32,
//             v_sub_co_u32 / v_subbrev_co_u32
//   int64     v_lshlrev_b64, v_lshrrev_b64, v_ashrrev_i64, v_lshl_add_u64 (the 64-bit add),
//             v_sub_co_u32 / v_subbrev_co_u32
//   bits      v_perm_b32, v_bfe_u32, v_bfe_i32, v_alignbit_b32, v_bcnt_u32_b32, v_ffbl_b32, v_ffbh_u32
//   dot       v_dot4_u32_u8, v_dot4c_i32_i8
//   cvt       v_cvt_pk_bf16_f32, v_cvt_f16_f32, v_cvt_pk_fp8_f32, v_cvt_pk_bf8_f32,
//             v_cvt_i32_f32, v_cvt_f32_i32
//   xlane     DPP row_ror (folded into v_xor_b32_dpp, once v_mov_b32_dpp), ds_bpermute_b32,
//             v_readlane_b32
//   approx    v_exp_f32, v_log_f32, v_rcp_f32, v_rsq_f32, v_sqrt_f32 (bounded, not exact)
// Measured on MI355X: every approx output is within 1 ulp of the rounded libm value; the bound
// of kApproxUlps = 8 is a condition that catches a result wrong on the whole device, the
// majority rule over the CUs' hashes (selftest_valu.py: fold_valu) the single deviant CU.
//
// Why the host's words are the one right answer:
//  * The integer groups are plain unsigned arithmetic.
//  * The IEEE groups are correctly rounded operations on finite normal operands, so IEEE 754
//    leaves one result. HostOps computes it in integers: every operand is sig x 2^exp with an
//    integer sig, the exact sum or product is formed in a 128-bit integer at the smaller
//    exponent (the windows below bound the shift, which is checked), and round_rne keeps the top
//    p bits, adding one when the dropped part is above half, or is half and the kept part odd.
//    The stand-alone program checks that std::fma / std::fmaf and plain float multiply and add
//    give the same words for fma32, fma64, pkfma32 and addmul32; pkfma16 has no libm
//    counterpart there and rests on the integer code and the Python twin's fractions.
//  * Windows: a step is x' = a * x + b with 1/8 <= |a| < 1/4 and 1 <= |b| < 2, and 1 <= |x0| < 2.
//    Then |x| <= 8/3 and |x'| >= 1 - (8/3)/4 = 1/3 throughout: no result is zero, subnormal or
//    infinite, whatever the denormal mode; a subtraction cancels at most two bits.
//  * cvt rounds f32 operands in [2^-2, 2^4) to bf16, f16, fp8 (OCP e4m3) and bf8 (e5m2): inside
//    every target's normal range and below its largest value, so neither saturation nor the
//    subnormal path is met; f32 -> i32 truncates, i32 -> f32 rounds 31-bit integers to 24 bits.
//    Selected (lane, step) pairs force the dropped bits to exactly one half: a tie per format.
// "Rounds up" below means the magnitude was incremented, "down" that it was truncated.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "nanogpu/selftest_host.h"

namespace nanogpu {
namespace selftest {
namespace valu {

constexpr int kValuSteps = 8;
constexpr int kLanes = 64;
constexpr int kLaneWords = 2;
constexpr int kGroupWords = kLanes * kLaneWords;

// The order is the bit order of the records.
enum Group : int {
  kFma32 = 0, kFma64, kPkFma16, kPkFma32, kAddMul32, kInt32, kInt64, kBits, kDot, kCvt, kXlane,
  kNumExact, kApprox = kNumExact, kRegs, kNumNames
};
constexpr uint32_t kAllExact = (1u << kNumExact) - 1;
constexpr uint32_t kAllGroups = (1u << kNumNames) - 1;
constexpr int kTableWords = kNumExact * kGroupWords;

inline const char* group_name(int g) {
  static const char* const names[kNumNames] = {"fma32", "fma64", "pkfma16", "pkfma32", "addmul32", "int32", "int64",
                                               "bits",  "dot",   "cvt",     "xlane",   "approx",   "regs"};
  return g >= 0 && g < kNumNames ? names[g] : "?";
}

// ---- operands ---------------------------------------------------------------------------
NANOGPU_HD inline uint32_t valu_operand(int g, int s, int lane, int k) {
  return mix32(0x5a17c0deu ^ (static_cast<uint32_t>(g) << 24) ^ (static_cast<uint32_t>(s) << 16) ^
               (static_cast<uint32_t>(lane) << 8) ^ static_cast<uint32_t>(k));
}
// sign and mantissa of u, exponent e: +-[1, 2) x 2^e
NANOGPU_HD inline uint32_t f32_win(uint32_t u, int e) { return (u & 0x807fffffu) | (static_cast<uint32_t>(127 + e) << 23); }
NANOGPU_HD inline uint64_t f64_win(uint32_t hi, uint32_t lo, int e) {
  return (static_cast<uint64_t>(hi & 0x800fffffu) << 32) | lo | (static_cast<uint64_t>(1023 + e) << 52);
}
NANOGPU_HD inline uint32_t f16_win(uint32_t u, int e) { return (u & 0x83ffu) | (static_cast<uint32_t>(15 + e) << 10); }
NANOGPU_HD inline uint32_t rotl32(uint32_t x, int r) { return (x << (r & 31)) | (x >> ((32 - r) & 31)); }

constexpr int kExpA = -3, kExpB = 0, kExpX0 = 0;   // the windows of a, b and x0 (see above)

// ---- the chains -------------------------------------------------------------------------
template <class Ops>
NANOGPU_HD inline void chain_fma32(Ops& o, int lane, uint32_t* out) {
  for (int c = 0; c < 2; ++c) {
    uint32_t x = f32_win(valu_operand(kFma32, 0, lane, 2 + 4 * c), kExpX0);
    for (int s = 0; s < kValuSteps; ++s)
      x = o.fma32(f32_win(valu_operand(kFma32, s, lane, 4 * c), kExpA), x, f32_win(valu_operand(kFma32, s, lane, 1 + 4 * c), kExpB));
    out[c] = x;
  }
}

template <class Ops>
NANOGPU_HD inline void chain_fma64(Ops& o, int lane, uint32_t* out) {
  uint64_t x = f64_win(valu_operand(kFma64, 0, lane, 4), valu_operand(kFma64, 0, lane, 5), kExpX0);
  for (int s = 0; s < kValuSteps; ++s)
    x = o.fma64(f64_win(valu_operand(kFma64, s, lane, 0), valu_operand(kFma64, s, lane, 1), kExpA), x,
                f64_win(valu_operand(kFma64, s, lane, 2), valu_operand(kFma64, s, lane, 3), kExpB));
  out[0] = static_cast<uint32_t>(x);
  out[1] = static_cast<uint32_t>(x >> 32);
}

// two halves a word: the low half is bits 0..15
NANOGPU_HD inline uint32_t f16x2_win(uint32_t u, int e) { return f16_win(u & 0xffffu, e) | (f16_win(u >> 16, e) << 16); }

template <class Ops>
NANOGPU_HD inline void chain_pkfma16(Ops& o, int lane, uint32_t* out) {
  for (int c = 0; c < 2; ++c) {
    uint32_t x = f16x2_win(valu_operand(kPkFma16, 0, lane, 2 + 4 * c), kExpX0);
    for (int s = 0; s < kValuSteps; ++s)
      x = o.pkfma16(f16x2_win(valu_operand(kPkFma16, s, lane, 4 * c), kExpA), x,
                    f16x2_win(valu_operand(kPkFma16, s, lane, 1 + 4 * c), kExpB));
    out[c] = x;
  }
}

template <class Ops>
NANOGPU_HD inline void chain_pkfma32(Ops& o, int lane, uint32_t* out) {
  uint32_t x0 = f32_win(valu_operand(kPkFma32, 0, lane, 4), kExpX0), x1 = f32_win(valu_operand(kPkFma32, 0, lane, 5), kExpX0);
  for (int s = 0; s < kValuSteps; ++s)
    o.pkfma32(f32_win(valu_operand(kPkFma32, s, lane, 0), kExpA), f32_win(valu_operand(kPkFma32, s, lane, 1), kExpA), x0, x1,
              f32_win(valu_operand(kPkFma32, s, lane, 2), kExpB), f32_win(valu_operand(kPkFma32, s, lane, 3), kExpB));
  out[0] = x0;
  out[1] = x1;
}

template <class Ops>
NANOGPU_HD inline void chain_addmul32(Ops& o, int lane, uint32_t* out) {
  for (int c = 0; c < 2; ++c) {
    uint32_t x = f32_win(valu_operand(kAddMul32, 0, lane, 2 + 4 * c), kExpX0);
    for (int s = 0; s < kValuSteps; ++s)
      x = o.add32(o.mul32(f32_win(valu_operand(kAddMul32, s, lane, 4 * c), kExpA), x),
                  f32_win(valu_operand(kAddMul32, s, lane, 1 + 4 * c), kExpB));
    out[c] = x;
  }
}

template <class Ops>
NANOGPU_HD inline void chain_int32(Ops& o, int lane, uint32_t* out) {
  uint32_t x = valu_operand(kInt32, 0, lane, 4), y = valu_operand(kInt32, 0, lane, 5);
  for (int s = 0; s < kValuSteps; ++s) {
    const uint32_t a = valu_operand(kInt32, s, lane, 0), b = valu_operand(kInt32, s, lane, 1);
    const uint32_t lo = x * a, hi = o.mulhi(y, b);
    const uint64_t t = static_cast<uint64_t>(a ^ y) * (b ^ x) + ((static_cast<uint64_t>(hi) << 32) | lo);   // mad_u64_u32
    uint64_t acc = (static_cast<uint64_t>(y) << 32) | x;
    acc = o.add64(acc, t);
    acc = o.sub64(acc, (static_cast<uint64_t>(valu_operand(kInt32, s, lane, 2)) << 32) | valu_operand(kInt32, s, lane, 3));
    x = static_cast<uint32_t>(acc);
    y = static_cast<uint32_t>(acc >> 32);
  }
  out[0] = x;
  out[1] = y;
}

template <class Ops>
NANOGPU_HD inline void chain_int64(Ops& o, int lane, uint32_t* out) {
  uint64_t x = (static_cast<uint64_t>(valu_operand(kInt64, 0, lane, 6)) << 32) | valu_operand(kInt64, 0, lane, 7);
  for (int s = 0; s < kValuSteps; ++s) {
    const uint64_t k1 = (static_cast<uint64_t>(valu_operand(kInt64, s, lane, 0)) << 32) | valu_operand(kInt64, s, lane, 1);
    const uint64_t k2 = (static_cast<uint64_t>(valu_operand(kInt64, s, lane, 2)) << 32) | valu_operand(kInt64, s, lane, 3);
    const uint32_t sh = valu_operand(kInt64, s, lane, 4);
    x = o.add64(x, k1);
    x = (x << (sh & 63)) ^ (x >> ((sh >> 8) & 63));
    x = o.sub64(x, k2);
    x = o.asr64(x, (sh >> 16) & 63) ^ (x << 7);
  }
  out[0] = static_cast<uint32_t>(x);
  out[1] = static_cast<uint32_t>(x >> 32);
}

template <class Ops>
NANOGPU_HD inline void chain_bits(Ops& o, int lane, uint32_t* out) {
  for (int c = 0; c < 2; ++c) {
    uint32_t x = valu_operand(kBits, 0, lane, 3 + 4 * c);
    for (int s = 0; s < kValuSteps; ++s) {
      const uint32_t a = valu_operand(kBits, s, lane, 4 * c), sel = valu_operand(kBits, s, lane, 1 + 4 * c);
      const uint32_t u = valu_operand(kBits, s, lane, 2 + 4 * c);
      const uint32_t p = o.perm(x, a, sel & 0x07070707u);                    // bytes 0..3: a's, 4..7: x's
      const uint32_t e = o.bfe_u(p, u & 15u, 1u + ((u >> 4) & 15u));         // offset + width <= 31
      const uint32_t sb = o.bfe_i(p, (u >> 8) & 15u, 1u + ((u >> 12) & 15u));
      const uint32_t al = o.alignbit(p, a, (u >> 16) & 31u);
      const uint32_t cnt = o.bcnt(al, e);                                    // popcount(al) + e
      const uint32_t fl = o.ffbl(al | 0x80000000u), fh = o.ffbh(al | 1u);
      x = (al ^ rotl32(sb, 9)) + (cnt << 20) + (fl << 5) + (fh << 27) + x;
    }
    out[c] = x;
  }
}

template <class Ops>
NANOGPU_HD inline void chain_dot(Ops& o, int lane, uint32_t* out) {
  for (int c = 0; c < 2; ++c) {
    uint32_t x = valu_operand(kDot, 0, lane, 3 + 4 * c);
    for (int s = 0; s < kValuSteps; ++s) {
      const uint32_t a = valu_operand(kDot, s, lane, 4 * c), b = valu_operand(kDot, s, lane, 1 + 4 * c);
      x = o.udot4(a ^ x, b, x);
      x = o.sdot4(b ^ x, valu_operand(kDot, s, lane, 2 + 4 * c), x);
    }
    out[c] = x;
  }
}

// Which conversion's tie lane `lane` forces at step s (0 bf16, 1 f16, 2 fp8, 3 bf8, 4 i32 -> f32), or -1.
NANOGPU_HD inline int cvt_tie_target(int s, int lane) {
  const int t = (lane + 3 * s) & 7;
  return t < 5 ? t : -1;
}

template <class Ops>
NANOGPU_HD inline void chain_cvt(Ops& o, int lane, uint32_t* out) {
  uint32_t h0 = valu_operand(kCvt, 0, lane, 6), h1 = valu_operand(kCvt, 0, lane, 7);
  for (int s = 0; s < kValuSteps; ++s) {
    const uint32_t u2 = valu_operand(kCvt, s, lane, 2);
    uint32_t ma = valu_operand(kCvt, s, lane, 0) ^ h0, mb = valu_operand(kCvt, s, lane, 1) ^ h1;
    const int tie = cvt_tie_target(s, lane);
    // dropped bits of the f32 mantissa: bf16 16, f16 13, fp8 20, bf8 21; exactly one half of them
    if (tie == 0) ma = (ma & ~0xffffu) | 0x8000u, mb = (mb & ~0xffffu) | 0x8000u;
    if (tie == 1) ma = (ma & ~0x1fffu) | 0x1000u, mb = (mb & ~0x1fffu) | 0x1000u;
    if (tie == 2) ma = (ma & ~0xfffffu) | 0x80000u, mb = (mb & ~0xfffffu) | 0x80000u;
    if (tie == 3) ma = (ma & ~0x1fffffu) | 0x100000u, mb = (mb & ~0x1fffffu) | 0x100000u;
    const uint32_t xa = f32_win(ma, static_cast<int>(u2 % 6u) - 2), xb = f32_win(mb, static_cast<int>((u2 >> 8) % 6u) - 2);
    const uint32_t w_bf = o.pk_bf16(xa, xb);
    const uint32_t w_h = o.f16(xa) | (o.f16(xb) << 16);
    const uint32_t w_8 = o.pk_fp8(xa, xb) | (o.pk_bf8(xa, xb) << 16);
    // f32 -> i32 of +-[2^20, 2^28): truncates a fraction below 2^23
    const uint32_t xc = f32_win(valu_operand(kCvt, s, lane, 3) ^ h0, 20 + static_cast<int>((u2 >> 16) & 7u));
    const uint32_t ii = o.f2i(xc);
    // i32 -> f32 of +-[2^30, 2^31): 31 bits to 24, the tie is 0x40 in the low 7
    uint32_t mag = ((valu_operand(kCvt, s, lane, 4) ^ ii) & 0x3fffffffu) | 0x40000000u;
    if (tie == 4) mag = (mag & ~0x7fu) | 0x40u;
    const uint32_t iv = (valu_operand(kCvt, s, lane, 5) & 1u) ? 0u - mag : mag;
    const uint32_t fi = o.i2f(iv);
    h0 = rotl32(h0, 5) ^ w_bf ^ rotl32(w_8, 11);
    h1 = rotl32(h1, 7) ^ w_h ^ rotl32(fi, 3) ^ ii;
  }
  out[0] = h0;
  out[1] = h1;
}

// xlane: the three cross-lane reads of step s. Lane l of a row of 16 reads lane (l - n) mod 16
// (DPP row_ror:n), lane l ^ 32 (ds_bpermute) and lane xlane_readlane(s) (v_readlane).
NANOGPU_HD constexpr int xlane_ror(int s) { return 1 + (s * 5) % 15; }
NANOGPU_HD constexpr int xlane_readlane(int s) { return (s * 27 + 5) & 63; }
NANOGPU_HD inline uint32_t xlane_combine(uint32_t d, uint32_t b, uint32_t r, uint32_t k) {
  return (d ^ rotl32(b, 7)) + rotl32(r, 13) + k;
}

// ---- approx -----------------------------------------------------------------------------
enum ApproxOp : int { kExp2 = 0, kLog2, kRcp, kRsq, kSqrt, kNumApprox };
constexpr int kApproxUlps = 8;   // a condition, not a measurement: see the README's self-test bullet
constexpr int kApproxWords = kNumApprox * kLanes * 2;   // [op][lane]{lo, hi}

inline const char* approx_name(int op) {
  static const char* const names[kNumApprox] = {"exp2", "log2", "rcp", "rsq", "sqrt"};
  return op >= 0 && op < kNumApprox ? names[op] : "?";
}

// exp2: +-[2^-4, 2^4), inside [-20, 20]; log2: [2, 2^20); the others [2^-20, 2^20).
NANOGPU_HD inline uint32_t approx_input(int op, int lane) {
  const uint32_t u = valu_operand(kApprox, op, lane, 0), v = valu_operand(kApprox, op, lane, 1);
  if (op == kExp2) return f32_win(u, static_cast<int>(v % 8u) - 4);
  if (op == kLog2) return f32_win(u & 0x7fffffffu, 1 + static_cast<int>(v % 19u));
  return f32_win(u & 0x7fffffffu, static_cast<int>(v % 40u) - 20);
}

// A float's bits as an integer ordered like the floats.
NANOGPU_HD inline uint32_t ordered_key(uint32_t bits) { return (bits & 0x80000000u) ? ~bits : bits | 0x80000000u; }

NANOGPU_HD inline uint32_t approx_lane_hash(const uint32_t out[kNumApprox], int lane) {
  uint32_t h = static_cast<uint32_t>(lane) * kHiMul;
  for (int op = 0; op < kNumApprox; ++op) h = mix32(h ^ out[op]);
  return h;   // a wave's hash is the wrapping sum over its lanes
}

inline double approx_libm(int op, double x) {
  switch (op) {
    case kExp2: return std::exp2(x);
    case kLog2: return std::log2(x);
    case kRcp: return 1.0 / x;
    case kRsq: return 1.0 / std::sqrt(x);
    default: return std::sqrt(x);
  }
}

inline float bits_float(uint32_t b) {
  float f;
  std::memcpy(&f, &b, 4);
  return f;
}
inline uint32_t float_bits(float f) {
  uint32_t b;
  std::memcpy(&b, &f, 4);
  return b;
}

// The double-precision libm value rounded to f32, as a key; the range is that +- kApproxUlps.
inline uint32_t approx_center(int op, int lane) {
  return ordered_key(float_bits(static_cast<float>(approx_libm(op, static_cast<double>(bits_float(approx_input(op, lane)))))));
}

inline std::vector<uint32_t> approx_ranges() {
  std::vector<uint32_t> r(kApproxWords);
  for (int op = 0; op < kNumApprox; ++op)
    for (int lane = 0; lane < kLanes; ++lane) {
      const uint32_t c = approx_center(op, lane);
      r[(op * kLanes + lane) * 2] = c - kApproxUlps;
      r[(op * kLanes + lane) * 2 + 1] = c + kApproxUlps;
    }
  return r;
}

// ---- register file ----------------------------------------------------------------------
constexpr int kRegSlots = 448;
constexpr int kRegFlagSlots = 32;                      // slots a flag word covers
constexpr int kRegFlags = kRegSlots / kRegFlagSlots;
static_assert(kRegSlots % kRegFlagSlots == 0, "whole flag words");

// The value lane `thread` (0..255: wave and lane) holds in slot `slot`; pass 1 holds the complement.
NANOGPU_HD inline uint32_t reg_word(uint32_t slot, uint32_t thread, uint32_t seed, uint32_t pass) {
  const uint32_t v = mix32(((slot << 8) | thread) ^ seed);
  return pass ? ~v : v;
}

// ---- record -----------------------------------------------------------------------------
// xcc, hw_id of wave 0, fail (bits 0..3 exact groups of wave w, 4..7 register file, 8..11 approx
// bound, 12..15 approx hash unlike wave 0's), SIMD ids seen, failed-group bits, first bad register
// slot and its thread (wave << 6 | lane) or kNoBad, hash of wave 0's approx outputs.
constexpr int kValuRecordWords = 8;
constexpr uint32_t kNoBad = 0xffffffffu;
constexpr int kFailExactShift = 0, kFailRegsShift = 4, kFailBoundShift = 8, kFailHashShift = 12;

struct ValuRecord {
  uint32_t xcc, hw_id, fail, simds, groups, bad_slot, bad_thread, approx_hash;
};

inline ValuRecord decode_valu_record(const uint32_t* words, size_t block) {
  const uint32_t* w = words + block * static_cast<size_t>(kValuRecordWords);
  return ValuRecord{w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]};
}

// ---- host arithmetic --------------------------------------------------------------------
struct Conds {              // counted over one group's 64 lanes
  int eff_add = 0, eff_sub = 0, round_up = 0, round_down = 0, exact = 0;
  int abnormal = 0;         // an operand or result that is zero, subnormal, infinite or NaN, or a shift out of bounds
  int carry31 = 0, carry63 = 0, borrow63 = 0;
  int tie_up[5] = {0, 0, 0, 0, 0}, tie_down[5] = {0, 0, 0, 0, 0};
};

using u128 = unsigned __int128;

struct Fmt {
  int p, ebits, bias;   // precision with the hidden bit, exponent bits, bias
};
constexpr Fmt kF64{53, 11, 1023}, kF32{24, 8, 127}, kF16{11, 5, 15}, kBf16{8, 8, 127}, kE4m3{4, 4, 7}, kE5m2{3, 5, 15};

struct Num {   // (-1)^neg * sig * 2^exp
  bool neg;
  u128 sig;
  int exp;
};

struct HostOps {
  Conds c;

  Num unpack(uint64_t bits, Fmt f) {
    const int mbits = f.p - 1;
    const uint64_t ef = (bits >> mbits) & ((uint64_t(1) << f.ebits) - 1);
    if (ef == 0 || ef == (uint64_t(1) << f.ebits) - 1) ++c.abnormal;
    return Num{((bits >> (mbits + f.ebits)) & 1) != 0, (bits & ((uint64_t(1) << mbits) - 1)) | (uint64_t(1) << mbits),
               static_cast<int>(ef) - f.bias - mbits};
  }

  // v rounded to nearest, ties to even, in format f; `tie` (optional) is set to +1 / -1 when the
  // dropped part was exactly one half and the magnitude went up / down.
  uint64_t round_pack(Num v, Fmt f, int* tie = nullptr) {
    if (v.sig == 0) {
      ++c.abnormal;
      return 0;
    }
    int top = 0;
    for (u128 t = v.sig; t >>= 1;) ++top;          // index of the leading one
    const int drop = top + 1 - f.p;
    u128 kept = v.sig;
    int exp = v.exp;
    if (drop > 0) {
      kept = v.sig >> drop;
      const u128 rest = v.sig & ((u128(1) << drop) - 1), half = u128(1) << (drop - 1);
      const bool up = rest > half || (rest == half && (kept & 1));
      if (rest == 0) ++c.exact;
      else if (up) ++c.round_up;
      else ++c.round_down;
      if (tie && rest == half) *tie = up ? 1 : -1;
      if (up) ++kept;
      exp += drop;
      if (kept >> f.p) kept >>= 1, ++exp;          // 1.11..1 rounded up to 10.0..0
    } else {
      ++c.exact;
      kept <<= -drop;
      exp += drop;
    }
    const int mbits = f.p - 1;
    const int ef = exp + mbits + f.bias;
    const int ef_max = (1 << f.ebits) - 2 + (f.ebits == 4 ? 1 : 0);   // e4m3 has no infinity: field 15 holds values
    if (ef < 1 || ef > ef_max || (f.ebits == 4 && ef == 15 && (kept & 7) == 7)) ++c.abnormal;
    return (static_cast<uint64_t>(v.neg) << (mbits + f.ebits)) | (static_cast<uint64_t>(ef) << mbits) |
           (static_cast<uint64_t>(kept) & ((uint64_t(1) << mbits) - 1));
  }

  Num product(Num a, Num b) { return Num{a.neg != b.neg, a.sig * b.sig, a.exp + b.exp}; }

  Num sum(Num a, Num b) {
    ++(a.neg == b.neg ? c.eff_add : c.eff_sub);
    const int e = a.exp < b.exp ? a.exp : b.exp;
    if (a.exp - e > 64 || b.exp - e > 64 || (a.sig >> 110) || (b.sig >> 60)) {
      ++c.abnormal;   // outside the windows: the 128-bit sum is not promised
      return Num{false, 0, 0};
    }
    const u128 x = a.sig << (a.exp - e), y = b.sig << (b.exp - e);
    if (a.neg == b.neg) return Num{a.neg, x + y, e};
    return x >= y ? Num{a.neg, x - y, e} : Num{b.neg, y - x, e};
  }

  uint64_t fma(uint64_t a, uint64_t x, uint64_t b, Fmt f) {
    return round_pack(sum(product(unpack(a, f), unpack(x, f)), unpack(b, f)), f);
  }
  uint32_t fma32(uint32_t a, uint32_t x, uint32_t b) { return static_cast<uint32_t>(fma(a, x, b, kF32)); }
  uint64_t fma64(uint64_t a, uint64_t x, uint64_t b) { return fma(a, x, b, kF64); }
  uint32_t pkfma16(uint32_t a, uint32_t x, uint32_t b) {
    return static_cast<uint32_t>(fma(a & 0xffffu, x & 0xffffu, b & 0xffffu, kF16)) |
           (static_cast<uint32_t>(fma(a >> 16, x >> 16, b >> 16, kF16)) << 16);
  }
  void pkfma32(uint32_t a0, uint32_t a1, uint32_t& x0, uint32_t& x1, uint32_t b0, uint32_t b1) {
    x0 = fma32(a0, x0, b0);
    x1 = fma32(a1, x1, b1);
  }
  uint32_t mul32(uint32_t a, uint32_t b) { return static_cast<uint32_t>(round_pack(product(unpack(a, kF32), unpack(b, kF32)), kF32)); }
  uint32_t add32(uint32_t a, uint32_t b) { return static_cast<uint32_t>(round_pack(sum(unpack(a, kF32), unpack(b, kF32)), kF32)); }

  uint32_t mulhi(uint32_t a, uint32_t b) { return static_cast<uint32_t>((static_cast<uint64_t>(a) * b) >> 32); }
  uint64_t add64(uint64_t a, uint64_t b) {
    const uint64_t r = a + b;
    if ((static_cast<uint64_t>(static_cast<uint32_t>(a)) + static_cast<uint32_t>(b)) >> 32) ++c.carry31;
    if (r < a) ++c.carry63;
    return r;
  }
  uint64_t sub64(uint64_t a, uint64_t b) {
    if (static_cast<uint32_t>(a) < static_cast<uint32_t>(b)) ++c.carry31;
    if (a < b) ++c.borrow63;
    return a - b;
  }
  uint64_t asr64(uint64_t x, uint32_t n) {   // arithmetic, without a signed shift
    const uint64_t fill = (x >> 63) ? ~uint64_t(0) : 0;
    return n ? (x >> n) | (fill << (64 - n)) : x;
  }

  uint32_t perm(uint32_t s0, uint32_t s1, uint32_t sel) {
    const uint64_t both = (static_cast<uint64_t>(s0) << 32) | s1;
    uint32_t r = 0;
    for (int i = 0; i < 4; ++i) r |= static_cast<uint32_t>((both >> (8 * ((sel >> (8 * i)) & 7u))) & 0xffu) << (8 * i);
    return r;
  }
  uint32_t bfe_u(uint32_t v, uint32_t off, uint32_t width) { return (v >> off) & ((1u << width) - 1u); }
  uint32_t bfe_i(uint32_t v, uint32_t off, uint32_t width) {
    const uint32_t f = bfe_u(v, off, width), sign = 1u << (width - 1);
    return (f ^ sign) - sign;
  }
  uint32_t alignbit(uint32_t hi, uint32_t lo, uint32_t sh) {
    return static_cast<uint32_t>(((static_cast<uint64_t>(hi) << 32) | lo) >> (sh & 31u));
  }
  uint32_t bcnt(uint32_t v, uint32_t add) {
    uint32_t n = 0;
    for (; v; v &= v - 1) ++n;
    return n + add;
  }
  uint32_t ffbl(uint32_t v) {   // v != 0
    uint32_t n = 0;
    while (!((v >> n) & 1u)) ++n;
    return n;
  }
  uint32_t ffbh(uint32_t v) {   // v != 0
    uint32_t n = 0;
    while (!((v << n) & 0x80000000u)) ++n;
    return n;
  }
  uint32_t udot4(uint32_t a, uint32_t b, uint32_t acc) {
    for (int i = 0; i < 4; ++i) acc += ((a >> (8 * i)) & 0xffu) * ((b >> (8 * i)) & 0xffu);
    return acc;
  }
  uint32_t sdot4(uint32_t a, uint32_t b, uint32_t acc) {
    for (int i = 0; i < 4; ++i) {
      const int32_t x = static_cast<int32_t>((a >> (8 * i)) & 0xffu), y = static_cast<int32_t>((b >> (8 * i)) & 0xffu);
      acc += static_cast<uint32_t>((x >= 128 ? x - 256 : x) * (y >= 128 ? y - 256 : y));
    }
    return acc;
  }

  uint32_t cvt(uint32_t x, Fmt f, int target) {
    int tie = 0;
    const uint32_t r = static_cast<uint32_t>(round_pack(unpack(x, kF32), f, &tie));
    if (tie > 0) ++c.tie_up[target];
    if (tie < 0) ++c.tie_down[target];
    return r;
  }
  uint32_t pk_bf16(uint32_t a, uint32_t b) { return cvt(a, kBf16, 0) | (cvt(b, kBf16, 0) << 16); }
  uint32_t f16(uint32_t a) { return cvt(a, kF16, 1); }
  uint32_t pk_fp8(uint32_t a, uint32_t b) { return cvt(a, kE4m3, 2) | (cvt(b, kE4m3, 2) << 8); }
  uint32_t pk_bf8(uint32_t a, uint32_t b) { return cvt(a, kE5m2, 3) | (cvt(b, kE5m2, 3) << 8); }
  uint32_t f2i(uint32_t x) {   // toward zero; |x| < 2^31
    const Num v = unpack(x, kF32);
    const uint32_t mag = static_cast<uint32_t>(v.exp >= 0 ? v.sig << v.exp : v.sig >> -v.exp);
    if (v.exp > 7) ++c.abnormal;
    return v.neg ? 0u - mag : mag;
  }
  uint32_t i2f(uint32_t i) {
    const bool neg = (i >> 31) != 0;
    int tie = 0;
    const uint32_t r = static_cast<uint32_t>(round_pack(Num{neg, neg ? 0u - i : i, 0}, kF32, &tie));
    if (tie > 0) ++c.tie_up[4];
    if (tie < 0) ++c.tie_down[4];
    return r;
  }
};

// All 64 lanes of the xlane group in lockstep.
inline void xlane_expected(uint32_t* out) {
  for (int c = 0; c < 2; ++c) {
    uint32_t x[kLanes], n[kLanes];
    for (int l = 0; l < kLanes; ++l) x[l] = valu_operand(kXlane, 0, l, 1 + 4 * c);
    for (int s = 0; s < kValuSteps; ++s) {
      for (int l = 0; l < kLanes; ++l)
        n[l] = xlane_combine(x[(l & 48) | ((l - xlane_ror(s)) & 15)], x[l ^ 32], x[xlane_readlane(s)],
                             valu_operand(kXlane, s, l, 4 * c));
      for (int l = 0; l < kLanes; ++l) x[l] = n[l];
    }
    for (int l = 0; l < kLanes; ++l) out[l * kLaneWords + c] = x[l];
  }
}

// Group g's kGroupWords expected words, [lane][word]; `conds` (optional) gets the counters.
inline void group_expected(int g, uint32_t* out, Conds* conds = nullptr) {
  HostOps o;
  if (g == kXlane) {
    xlane_expected(out);
  } else {
    for (int lane = 0; lane < kLanes; ++lane) {
      uint32_t* w = out + lane * kLaneWords;
      switch (g) {
        case kFma32: chain_fma32(o, lane, w); break;
        case kFma64: chain_fma64(o, lane, w); break;
        case kPkFma16: chain_pkfma16(o, lane, w); break;
        case kPkFma32: chain_pkfma32(o, lane, w); break;
        case kAddMul32: chain_addmul32(o, lane, w); break;
        case kInt32: chain_int32(o, lane, w); break;
        case kInt64: chain_int64(o, lane, w); break;
        case kBits: chain_bits(o, lane, w); break;
        case kDot: chain_dot(o, lane, w); break;
        default: chain_cvt(o, lane, w); break;
      }
    }
  }
  if (conds) *conds = o.c;
}

inline std::vector<uint32_t> expected_table() {
  std::vector<uint32_t> t(kTableWords);
  for (int g = 0; g < kNumExact; ++g) group_expected(g, t.data() + g * kGroupWords);
  return t;
}

// Result bits that need not take both values over the 64 lanes, per group and word: none. The
// FP results' exponents are windowed to 2^-2..2^1, but the fields of 2^0 (0111..1) and 2^1
// (1000..0) differ in every bit, and both occur in every FP group.
constexpr uint32_t kConstantBits[kNumExact][kLaneWords] = {};

// Bits of group g's word w that are constant over the lanes although kConstantBits does not list them.
inline uint32_t uncovered_bits(int g, int w, const uint32_t* words) {
  uint32_t ones = 0, zeros = 0;
  for (int lane = 0; lane < kLanes; ++lane) ones |= words[lane * kLaneWords + w], zeros |= ~words[lane * kLaneWords + w];
  return ~(ones & zeros) & ~kConstantBits[g][w];
}

constexpr bool group_is_fp(int g) { return g <= kAddMul32; }

}  // namespace valu
}  // namespace selftest
}  // namespace nanogpu
