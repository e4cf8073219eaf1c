// Host/device-shared arithmetic of the deep self-test's matrix paths (native/hip/probe_sweep.inc:
// matrix_tile, cu_sweep_paths). A path is one MFMA instruction plus its operand formats.
// Plain C++ with no HIP dependency: native/tests/selftest_paths_host_main.cpp builds and runs
// the host side on its own, under sanitizers too. The Python twin is nanogpu/probe/selftest.py.
//
// The data is generated as operand CODES (bit patterns), never as values: the kernel packs the
// codes as they are and the host decodes them, so every bit of every format is driven
// directly and no encoder exists that could share a bug with the hardware's decoder.
//
// Exactness. Every decoded operand is sig * 2^exp with sig an odd integer (or 0), an E8M0
// scale only adds to exp, so every product of the chain is an integer multiple of
// u = 2^unit_exp, the smallest product exponent of the path. path_expected sums the chain in
// integers on that unit and returns sum_abs_max, the largest sum over one accumulator of the
// absolute values of all its terms. While sum_abs_max < 2^24 (fp32 accumulators), 2^31 (i32)
// or 2^53 (f64), every partial sum in any order or grouping is a multiple of u below that
// limit, hence representable, and the hardware's result is the integer sum whatever its
// internal order: the assumption the bf16 chain of selftest_host.h already rests on.
// Worst cases by format (the data's own figures are smaller; both mains assert them):
//   fp8    e4m3, exponent field 5..8: |sig| <= 15 << 3, product < 2^13.9, 128 terms: < 2^20.9
//   bf8    e5m2, exponent field 14..17: |sig| <= 7 << 3, product < 2^11.7, 128 terms: < 2^18.7
//   i8     |a b| <= 2^14, 256 terms: <= 2^22 (limit 2^31)
//   mxfp8  e4m3 7..8 and scales 2^0..2^1: product < 2^9.9 * 4, 512 terms: < 2^20.9
//   mxfp6  e2m3, all 64 codes: |units| <= 60, product <= 3600 * 4, 512 terms: < 2^22.9
//   mxfp4  e2m1, all 16 codes: |units| <= 12, product <= 144 * 4, 512 terms: < 2^18.2
//   f16 / f32 / f64: a significand with its last mantissa bit set is as wide as the
//     accumulator's, so an accumulator can hold one such term at most. Each accumulator gets
//     exactly one FINE term, [2, 3) with every mantissa bit below the top one hashed, times
//     +-1: at most 3 * 2^(M-1) units of 2^(1-M); all its other terms are COARSE x COARSE,
//     below 2^-6 each. Even rows take the FINE value in A (step 0, k 0), odd rows meet the
//     FINE value of B (step 1, k 0), where A holds 0 for the even rows.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <vector>

#include "nanogpu/selftest_host.h"

namespace nanogpu {
namespace selftest {
namespace paths {

// ---- the paths --------------------------------------------------------------------------
enum Path : int { kF16 = 0, kFp8, kBf8, kI8, kMxFp8, kMxFp6, kMxFp4, kF32, kF64, kNumPaths };
constexpr uint32_t kAllPaths = (1u << kNumPaths) - 1;
constexpr int kPathSteps = 8;          // accumulating instructions of one chain
constexpr int kTileWords = 1024;       // 32-bit words of one expected tile in the upload (f64 uses 512)

inline const char* path_name(int p) {
  static const char* const names[kNumPaths] = {"f16", "fp8", "bf8", "i8", "mxfp8", "mxfp6", "mxfp4", "f32", "f64"};
  return p >= 0 && p < kNumPaths ? names[p] : "?";
}

NANOGPU_HD constexpr int path_k(int p) {          // K of one instruction
  return p == kI8 ? 32 : p == kMxFp8 || p == kMxFp6 || p == kMxFp4 ? 64 : p == kF32 ? 2 : p == kF64 ? 4 : 16;
}
NANOGPU_HD constexpr int path_code_bits(int p) {
  return p == kF16 ? 16 : p == kMxFp6 ? 6 : p == kMxFp4 ? 4 : p == kF32 ? 32 : p == kF64 ? 64 : 8;
}
NANOGPU_HD constexpr int path_dim(int p) { return p == kF64 ? 16 : 32; }                    // the tile is dim x dim
NANOGPU_HD constexpr int path_row_dwords(int p) { return path_k(p) * path_code_bits(p) / 32; }
NANOGPU_HD constexpr bool path_scaled(int p) { return p == kMxFp8 || p == kMxFp6 || p == kMxFp4; }
NANOGPU_HD constexpr int path_limit_bits(int p) { return p == kI8 ? 31 : p == kF64 ? 53 : 24; }
// cbsz / blgp of v_mfma_scale_f32_32x32x64_f8f6f4: 0 = e4m3, 2 = e2m3, 4 = e2m1
NANOGPU_HD constexpr int path_fmt_select(int p) { return p == kMxFp6 ? 2 : p == kMxFp4 ? 4 : 0; }

// ---- formats ----------------------------------------------------------------------------
struct Format {
  int ebits, mbits, bias;   // ebits == 0: two's complement int8
};
NANOGPU_HD constexpr Format path_format(int p) {
  return p == kF16   ? Format{5, 10, 15}
         : p == kBf8 ? Format{5, 2, 15}
         : p == kI8  ? Format{0, 8, 0}
         : p == kMxFp6 ? Format{2, 3, 1}
         : p == kMxFp4 ? Format{2, 1, 1}
         : p == kF32 ? Format{8, 23, 127}
         : p == kF64 ? Format{11, 52, 1023}
                     : Format{4, 3, 7};     // fp8, mxfp8: e4m3
}

// The exponent fields a path's codes may hold: base + i for every bit i of offsets.
struct ExpWindow {
  int base;
  uint32_t offsets;
};
NANOGPU_HD constexpr ExpWindow path_exp_window(int p) {
  return p == kFp8     ? ExpWindow{5, 0xf}       // 5..8
         : p == kBf8   ? ExpWindow{14, 0xf}      // 14..17
         : p == kMxFp8 ? ExpWindow{7, 0x3}       // 7..8
         : p == kMxFp6 || p == kMxFp4 ? ExpWindow{0, 0xf}   // every code
         : p == kF16   ? ExpWindow{8, 0x18f}     // COARSE 8..11, ONE 15, FINE 16
         : p == kF32   ? ExpWindow{120, 0x18f}
         : p == kF64   ? ExpWindow{1016, 0x18f}
                       : ExpWindow{0, 0};
}
constexpr int kScaleLo = 127, kScaleHi = 128;   // E8M0 window: 2^0 and 2^1; every scale bit takes both values

// ---- decoders (OCP definitions) ---------------------------------------------------------
// value = sig * 2^exp, sig odd or 0.
struct Dec {
  int64_t sig;
  int exp;
};

inline Dec normalised(int64_t sig, int exp) {
  if (sig == 0) return Dec{0, 0};
  while ((sig & 1) == 0) {
    sig /= 2;
    ++exp;
  }
  return Dec{sig, exp};
}

// A finite code of a sign / exponent / mantissa format without special exponents handled
// here: e == 0 is subnormal (0.m * 2^(1-bias)), anything else 1.m * 2^(e-bias).
inline Dec decode_minifloat(uint64_t code, Format f) {
  const uint64_t m = code & ((1ull << f.mbits) - 1);
  const int e = static_cast<int>((code >> f.mbits) & ((1ull << f.ebits) - 1));
  const bool neg = (code >> (f.ebits + f.mbits)) & 1;
  const int64_t sig = static_cast<int64_t>(e ? (1ull << f.mbits) + m : m);
  return normalised(neg ? -sig : sig, (e ? e : 1) - f.bias - f.mbits);
}

inline double dec_value(Dec d) { return std::ldexp(static_cast<double>(d.sig), d.exp); }

inline double decode_e4m3fn(uint8_t c) {   // no Inf; S.1111.111 is NaN; 0x7e = 448
  if ((c & 0x7f) == 0x7f) return std::numeric_limits<double>::quiet_NaN();
  const double v = dec_value(decode_minifloat(c, Format{4, 3, 7}));
  return (c & 0x80) && v == 0.0 ? -0.0 : v;
}
inline double decode_e5m2(uint8_t c) {     // IEEE-like: exponent 31 is Inf (m == 0) or NaN
  if (((c >> 2) & 0x1f) == 0x1f) {
    if (c & 3) return std::numeric_limits<double>::quiet_NaN();
    return (c & 0x80) ? -std::numeric_limits<double>::infinity() : std::numeric_limits<double>::infinity();
  }
  const double v = dec_value(decode_minifloat(c, Format{5, 2, 15}));
  return (c & 0x80) && v == 0.0 ? -0.0 : v;
}
inline double decode_e2m3(uint8_t c) {     // 6 bits, no Inf / NaN; max 7.5
  const double v = dec_value(decode_minifloat(c & 0x3f, Format{2, 3, 1}));
  return (c & 0x20) && v == 0.0 ? -0.0 : v;
}
inline double decode_e2m1(uint8_t c) {     // 4 bits, no Inf / NaN; max 6
  const double v = dec_value(decode_minifloat(c & 0xf, Format{2, 1, 1}));
  return (c & 0x8) && v == 0.0 ? -0.0 : v;
}
inline double decode_e8m0(uint8_t c) {     // 2^(c - 127); 255 is NaN
  return c == 0xff ? std::numeric_limits<double>::quiet_NaN() : std::ldexp(1.0, static_cast<int>(c) - 127);
}

inline Dec path_decode(int p, uint64_t code) {
  if (p == kI8) return normalised(static_cast<int8_t>(code & 0xff), 0);
  return decode_minifloat(code, path_format(p));
}

// ---- generators of operand codes --------------------------------------------------------
// Operand `op` (0: A, indexed by row; 1: B, indexed by column) of step `s` is, per row or
// column `idx`, a little-endian bit string of K codes in path_row_dwords(p) dwords; code k is
// bits [k * code_bits, (k + 1) * code_bits). The generator is cheap on purpose, because every
// wave of every visit of a CU runs it (a visit must not get longer): one mix32 per
// (p, op, idx), three operations to vary it by step, one rotation per dword. A and B differ
// through `op`, and idx enters through the hash while k only selects a rotation, so no
// generator is symmetric in (row, k) / (k, col).
NANOGPU_HD inline uint32_t rotl32(uint32_t x, int r) {
  r &= 31;
  return r ? (x << r) | (x >> (32 - r)) : x;
}
NANOGPU_HD inline uint32_t path_base(int p, int op, int idx) {
  return mix32(0x9e3779b9u ^ (static_cast<uint32_t>(p) << 27) ^ (static_cast<uint32_t>(op) << 26) ^
               (static_cast<uint32_t>(idx) << 8));
}
NANOGPU_HD inline uint32_t path_step_hash(int p, int op, int s, int idx) {
  const uint32_t base = path_base(p, op, idx);
  return (base ^ (base >> (s + 3))) + static_cast<uint32_t>(s) * 0x9e3779b9u;
}
// d = 0..15: the rotations 7 d + 3 (mod 32) are all different
NANOGPU_HD inline uint32_t path_hash(int p, int op, int s, int idx, int d) {
  return rotl32(path_step_hash(p, op, s, idx), 7 * d + 3);
}

// f16 / f32 / f64: see "Exactness" above. `hv` is the hash, as wide as the code (`bits`).
template <class U>   // uint32_t for f16 and f32, uint64_t for f64
NANOGPU_HD inline U wide_code(int bits, int mbits, int bias, int op, int s, int idx, int k, U hv) {
  const U sign = hv & (U(1) << (bits - 1));
  // sign, exponent field bias - 7 + (2 hashed bits), top 3 mantissa bits hashed: bias - 7 ends in 00
  const U coarse = (static_cast<U>(bias - 7) << mbits) | (hv & ((U(1) << (bits - 1)) | (U(3) << mbits) | (U(7) << (mbits - 3))));
  if (k != 0 || s > 1) return coarse;
  const U fine = sign | (static_cast<U>(bias + 1) << mbits) | (hv & ((U(1) << (mbits - 1)) - 1));
  const U one = sign | (static_cast<U>(bias) << mbits);
  if (s == 0) return op == 0 ? ((idx & 1) ? coarse : fine) : one;
  return op == 0 ? ((idx & 1) ? one : U(0)) : fine;
}

NANOGPU_HD inline uint64_t path_code_f64(int op, int s, int idx, int k) {
  const uint64_t hv = (static_cast<uint64_t>(path_hash(kF64, op, s, idx, 2 * k + 1)) << 32) |
                      path_hash(kF64, op, s, idx, 2 * k);
  return wide_code<uint64_t>(64, 52, 1023, op, s, idx, k, hv);
}

// Dword d of the packed operand, as the kernel loads it into its registers.
NANOGPU_HD inline uint32_t path_dword(int p, int op, int s, int idx, int d) {
  if (p == kF64) return static_cast<uint32_t>(path_code_f64(op, s, idx, d >> 1) >> (32 * (d & 1)));
  const uint32_t h = path_hash(p, op, s, idx, d);
  switch (p) {
    case kFp8:     // sign | 5 + (2 bits) | 3 mantissa bits, per byte; no carry leaves a byte
      return 0x28282828u + (h & 0x9f9f9f9fu);
    case kBf8:     // e5m2: sign | 14 + (2 bits) | 2 mantissa bits
    case kMxFp8:   // e4m3: sign | 7 + (1 bit) | 3 mantissa bits: the same constants
      return 0x38383838u + (h & 0x8f8f8f8fu);
    case kF16: {   // two COARSE halves at once; k = 0 (the low half of dword 0) is the special one
      const uint32_t w = 0x20002000u | (h & 0x8f808f80u);
      if (d != 0 || s > 1) return w;
      return (w & 0xffff0000u) | wide_code<uint32_t>(16, 10, 15, op, s, idx, 0, h & 0xffffu);
    }
    case kF32:
      return wide_code<uint32_t>(32, 23, 127, op, s, idx, d, h);
    default:       // i8, e2m3, e2m1: every code is valid
      return h;
  }
}

// code = f(step, row | col, k)
inline uint64_t path_code(int p, int op, int s, int idx, int k) {
  if (p == kF64) return path_code_f64(op, s, idx, k);
  const int cb = path_code_bits(p), bit = k * cb, d = bit / 32, sh = bit % 32;
  uint64_t w = path_dword(p, op, s, idx, d);
  if (sh + cb > 32) w |= static_cast<uint64_t>(path_dword(p, op, s, idx, d + 1)) << 32;   // e2m3 across two dwords
  return (w >> sh) & ((1ull << cb) - 1);
}

// E8M0 scales of the scaled paths: one per (row | col, 32-element k block). The kernel hands
// the instruction a whole dword and the byte to take (opsel); the other bytes hold other
// scales of the window, so a wrong byte changes the result.
NANOGPU_HD constexpr int path_opsel(int op, int s) { return op == 0 ? (s & 3) : ((s >> 1) & 3); }
NANOGPU_HD inline uint32_t path_scale_dword(int p, int op, int s, int idx, int block) {
  return 0x7f7f7f7fu + (rotl32(path_step_hash(p, op, s, idx), 19 + 6 * block) & 0x01010101u);
}
NANOGPU_HD inline uint32_t path_scale(int p, int op, int s, int idx, int block) {
  return (path_scale_dword(p, op, s, idx, block) >> (8 * path_opsel(op, s))) & 0xffu;
}

// ---- the expected tile ------------------------------------------------------------------
struct PathTile {
  int dim = 0;
  int unit_exp = 0;                 // u = 2^unit_exp
  std::vector<int64_t> units;       // dim x dim, row-major: the chain's sum in units of u
  int64_t sum_abs_max = 0;          // conservative: max over accumulators of the sum of |term| / u
  bool overflow = false;            // the integer arithmetic itself ran out of range (never, by the bounds)
  bool exact() const { return !overflow && sum_abs_max < (int64_t(1) << limit_bits); }
  int limit_bits = 24;
};

inline PathTile path_expected(int p) {
  const int dim = path_dim(p), K = path_k(p);
  PathTile t;
  t.dim = dim;
  t.limit_bits = path_limit_bits(p);
  std::vector<Dec> a(static_cast<size_t>(kPathSteps) * dim * K), b(a.size());
  auto at = [&](int s, int idx, int k) { return (static_cast<size_t>(s) * dim + idx) * K + k; };
  for (int op = 0; op < 2; ++op)
    for (int s = 0; s < kPathSteps; ++s)
      for (int idx = 0; idx < dim; ++idx)
        for (int k = 0; k < K; ++k) {
          Dec d = path_decode(p, path_code(p, op, s, idx, k));
          if (path_scaled(p) && d.sig != 0) d.exp += static_cast<int>(path_scale(p, op, s, idx, k / 32)) - 127;
          (op ? b : a)[at(s, idx, k)] = d;
        }
  // sig is odd, so a product's lowest set bit is exactly 2^(ea + eb): the unit is the smallest
  bool any = false;
  int emin = 0;
  for (int s = 0; s < kPathSteps; ++s)
    for (int k = 0; k < K; ++k)
      for (int r = 0; r < dim; ++r)
        for (int c = 0; c < dim; ++c) {
          const Dec &x = a[at(s, r, k)], &y = b[at(s, c, k)];
          if (x.sig == 0 || y.sig == 0) continue;
          if (!any || x.exp + y.exp < emin) emin = x.exp + y.exp;
          any = true;
        }
  t.unit_exp = emin;
  t.units.assign(static_cast<size_t>(dim) * dim, 0);
  const __int128 cap = static_cast<__int128>(1) << 62;
  for (int r = 0; r < dim; ++r)
    for (int c = 0; c < dim; ++c) {
      __int128 acc = 0, abs_sum = 0;
      for (int s = 0; s < kPathSteps; ++s)
        for (int k = 0; k < K; ++k) {
          const Dec &x = a[at(s, r, k)], &y = b[at(s, c, k)];
          if (x.sig == 0 || y.sig == 0) continue;
          const int sh = x.exp + y.exp - emin;
          if (sh > 62) {
            t.overflow = true;
            continue;
          }
          const __int128 term = (static_cast<__int128>(x.sig) * y.sig) * (static_cast<__int128>(1) << sh);
          acc += term;
          abs_sum += term < 0 ? -term : term;
          if (abs_sum >= cap) t.overflow = true;
        }
      if (t.overflow) return t;
      t.units[static_cast<size_t>(r) * dim + c] = static_cast<int64_t>(acc);
      if (static_cast<int64_t>(abs_sum) > t.sum_abs_max) t.sum_abs_max = static_cast<int64_t>(abs_sum);
    }
  return t;
}

// The tile as the kernel compares it: kTileWords 32-bit words, row-major; fp32 bit patterns,
// i32 for i8, and for f64 256 x (low word, high word). Only meaningful when t.exact().
inline void path_expected_words(int p, const PathTile& t, uint32_t out[kTileWords]) {
  for (int i = 0; i < kTileWords; ++i) out[i] = 0;
  for (size_t i = 0; i < t.units.size(); ++i) {
    const double v = std::ldexp(static_cast<double>(t.units[i]), t.unit_exp);   // exact: |units| < 2^53
    if (p == kI8) {
      out[i] = static_cast<uint32_t>(static_cast<int32_t>(v));
    } else if (p == kF64) {
      uint64_t bits;
      static_assert(sizeof(bits) == sizeof(v), "double is 64 bits");
      __builtin_memcpy(&bits, &v, 8);
      out[2 * i] = static_cast<uint32_t>(bits);
      out[2 * i + 1] = static_cast<uint32_t>(bits >> 32);
    } else {
      const float f = static_cast<float>(v);                                    // exact: |units| < 2^24
      uint32_t bits;
      __builtin_memcpy(&bits, &f, 4);
      out[i] = bits;
    }
  }
}

// FNV-1a over the tile's words, low byte first: what both mains and the Python twin pin.
inline uint32_t tile_checksum(const uint32_t* words, int n) {
  uint32_t h = 0x811c9dc5u;
  for (int i = 0; i < n; ++i)
    for (int b = 0; b < 4; ++b) {
      h ^= (words[i] >> (8 * b)) & 0xffu;
      h *= 0x01000193u;
    }
  return h;
}
inline int path_tile_words(int p) { return p == kF64 ? 512 : 1024; }

// ---- coverage of the data ---------------------------------------------------------------
// Unmet conditions of path p's data; 0 when all hold.
constexpr uint32_t kCovBits = 1;      // sign, every mantissa bit, every exponent bit the window varies: both values, in A and in B
constexpr uint32_t kCovWindow = 2;    // an exponent field outside the window (subnormal, NaN, Inf included)
constexpr uint32_t kCovAsym = 4;      // A(row,k) == A(k,row), B likewise, or A == B transposed
constexpr uint32_t kCovScale = 8;     // scales equal across rows, across the two k blocks, or between A and B; or outside the window
constexpr uint32_t kCovOpsel = 16;    // no step takes its scale from another byte than byte 0

inline uint32_t path_coverage(int p) {
  const int dim = path_dim(p), K = path_k(p);
  const Format f = path_format(p);
  const ExpWindow w = path_exp_window(p);
  const bool wide = p == kF16 || p == kF32 || p == kF64;
  uint32_t unmet = 0;
  uint64_t need = 0xff;                               // i8: all 8 bits
  if (f.ebits) {
    uint64_t e_or = 0, e_and = ~0ull;
    for (int i = 0; i < 32; ++i)
      if (w.offsets >> i & 1) {
        e_or |= static_cast<uint64_t>(w.base + i);
        e_and &= static_cast<uint64_t>(w.base + i);
      }
    need = (1ull << (f.ebits + f.mbits)) | ((e_or & ~e_and) << f.mbits) | ((1ull << f.mbits) - 1);
  }
  for (int op = 0; op < 2; ++op) {
    uint64_t ones = 0, zeros = 0;
    for (int s = 0; s < kPathSteps; ++s)
      for (int idx = 0; idx < dim; ++idx)
        for (int k = 0; k < K; ++k) {
          const uint64_t c = path_code(p, op, s, idx, k);
          ones |= c;
          zeros |= ~c;
          if (f.ebits && !(wide && c == 0)) {         // the wide paths' ZERO is the one code outside
            const int e = static_cast<int>((c >> f.mbits) & ((1ull << f.ebits) - 1)) - w.base;
            if (e < 0 || e > 31 || !(w.offsets >> e & 1)) unmet |= kCovWindow;
          }
        }
    if ((ones & zeros & need) != need) unmet |= kCovBits;
  }
  const int n = dim < K ? dim : K;
  bool a_sym = true, b_sym = true, ab_t = true;
  for (int s = 0; s < kPathSteps; ++s)
    for (int i = 0; i < dim; ++i)
      for (int k = 0; k < K; ++k) {
        if (path_code(p, 0, s, i, k) != path_code(p, 1, s, i, k)) ab_t = false;   // B[k][col i] against A[row i][k]
        if (i < n && k < n) {
          if (path_code(p, 0, s, i, k) != path_code(p, 0, s, k, i)) a_sym = false;
          if (path_code(p, 1, s, i, k) != path_code(p, 1, s, k, i)) b_sym = false;
        }
      }
  if (a_sym || b_sym || ab_t) unmet |= kCovAsym;
  if (path_scaled(p)) {
    bool rows = false, blocks = false, ab = false, other_byte = false;
    for (int s = 0; s < kPathSteps; ++s) {
      if (path_opsel(0, s) || path_opsel(1, s)) other_byte = true;
      for (int idx = 0; idx < dim; ++idx)
        for (int op = 0; op < 2; ++op)
          for (int blk = 0; blk < 2; ++blk) {
            const uint32_t sc = path_scale(p, op, s, idx, blk);
            if (sc < static_cast<uint32_t>(kScaleLo) || sc > static_cast<uint32_t>(kScaleHi)) unmet |= kCovScale;
            if (sc != path_scale(p, op, s, 0, blk)) rows = true;
            if (sc != path_scale(p, op, s, idx, 0)) blocks = true;
            if (sc != path_scale(p, 0, s, idx, blk)) ab = true;
          }
    }
    if (!rows || !blocks || !ab) unmet |= kCovScale;
    if (!other_byte) unmet |= kCovOpsel;
  }
  return unmet;
}

// ---- sweep record of cu_sweep_paths -----------------------------------------------------
// Words 0..4 are cu_sweep's record, with the same meaning (the bf16 chain and the LDS test
// still run). Word 5: bit p is set when path p's chain differed from its tile on any wave.
// Word 6: bit w (0..3) is set when wave w saw any path differ.
constexpr int kPathRecordWords = 7;   // decoded by decode_record(words, block, kPathRecordWords)

}  // namespace paths
}  // namespace selftest
}  // namespace nanogpu
