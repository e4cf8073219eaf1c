// Stand-alone check of the vector-ALU self-test's host arithmetic (nanogpu/selftest_valu_host.h),
// with no GPU code involved: `python native/build.py --selftest-host valu-asan` builds it under
// ASan + UBSan. It asserts the header's conditions on every group (normal operands and results,
// effective additions and subtractions, both rounding directions, bit coverage, conversion ties,
// distinct cross-lane results, carries), checks the integer rounding of fma32, fma64, pkfma32 and
// addmul32 against std::fma / std::fmaf and plain float arithmetic, pins spot values, and prints each group's checksum and counters and
// the approx ranges' checksum as one JSON line, which tests/test_selftest_valu.py compares with
// the Python twin's.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "nanogpu/selftest_paths_host.h"
#include "nanogpu/selftest_valu_host.h"

namespace sv = nanogpu::selftest::valu;
namespace sp = nanogpu::selftest::paths;

static int failures = 0;

#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);  \
      ++failures;                                                      \
    }                                                                  \
  } while (0)

// fma32, fma64, pkfma32 and addmul32 again, through the C library and the compiler's own float
// arithmetic. pkfma16 is not overridden, so it is left out of the comparison.
struct LibmOps : sv::HostOps {
  static double d(uint64_t b) {
    double v;
    std::memcpy(&v, &b, 8);
    return v;
  }
  static uint64_t bits(double v) {
    uint64_t b;
    std::memcpy(&b, &v, 8);
    return b;
  }
  uint32_t fma32(uint32_t a, uint32_t x, uint32_t b) {
    return sv::float_bits(std::fmaf(sv::bits_float(a), sv::bits_float(x), sv::bits_float(b)));
  }
  uint64_t fma64(uint64_t a, uint64_t x, uint64_t b) { return bits(std::fma(d(a), d(x), d(b))); }
  void pkfma32(uint32_t a0, uint32_t a1, uint32_t& x0, uint32_t& x1, uint32_t b0, uint32_t b1) {
    x0 = fma32(a0, x0, b0);
    x1 = fma32(a1, x1, b1);
  }
  uint32_t mul32(uint32_t a, uint32_t b) {
    volatile float p = sv::bits_float(a) * sv::bits_float(b);
    return sv::float_bits(p);
  }
  uint32_t add32(uint32_t a, uint32_t b) {
    volatile float s = sv::bits_float(a) + sv::bits_float(b);
    return sv::float_bits(s);
  }
};

int main() {
  sv::HostOps o;
  // spot values of the rounding, written out by hand
  CHECK(o.fma32(0x3e000000u, 0x3f800000u, 0x3f800000u) == 0x3f900000u);            // 1/8 * 1 + 1 = 1.125
  CHECK(o.fma32(0x3e000001u, 0x3fffffffu, 0xbf800000u) == 0xbf400000u);            // (1/8 + ulp)(2 - ulp) - 1 = -0.75 - 2^-49..: to -0.75
  CHECK(o.pk_bf16(0x3f808000u, 0x3f818000u) == 0x3f823f80u);                       // ties: 1 + 2^-8 -> 1 (even), 1 + 3 * 2^-8 -> 1 + 2^-6
  CHECK(o.f16(0x3f801000u) == 0x3c00u && o.f16(0x3f803000u) == 0x3c02u);           // f16 ties to even
  CHECK(o.pk_fp8(0x3f880000u, 0x40700000u) == 0x4738u);                            // 1.0625 ties to 1 (even); 3.75 = 1.111b x 2 is exact
  CHECK(o.pk_fp8(0x3f980000u, 0x3fb00000u) == 0x3b3au);                            // 1.1875 ties to 1.25 (even); 1.375 is exact
  CHECK(o.pk_bf8(0x3fa00000u, 0x3fe00000u) == 0x3f3du);                            // 1.25 and 1.75 are exact in e5m2
  CHECK(o.pk_bf8(0x3f900000u, 0x3fb00000u) == 0x3e3cu);                            // 1.125 ties to 1, 1.375 ties to 1.5
  CHECK(o.f2i(0x49f42478u) == 2000015u && o.f2i(0xc9f4247cu) == 0u - 2000015u);    // 2000015.0 and -2000015.5 truncate
  CHECK(o.i2f(0x40000040u) == 0x4e800000u && o.i2f(0x400000c0u) == 0x4e800002u);   // 31-bit ties to even
  CHECK(o.perm(0x44332211u, 0x88776655u, 0x07040300u) == 0x44118855u);             // bytes 0..3 of s1, 4..7 of s0
  CHECK(o.bfe_u(0xabcd1234u, 4, 8) == 0x23u && o.bfe_i(0xabcd1234u, 12, 4) == 0x1u && o.bfe_i(0xabcd1234u, 16, 4) == 0xfffffffdu);
  CHECK(o.alignbit(0x00000001u, 0x80000000u, 31) == 0x3u && o.bcnt(0xf0f0u, 5) == 13u);
  CHECK(o.ffbl(0x80000000u) == 31 && o.ffbh(1u) == 31 && o.ffbl(0x18u) == 3 && o.ffbh(0x18u) == 27);
  CHECK(o.udot4(0x01020304u, 0x05060708u, 10u) == 10u + 5 + 12 + 21 + 32);
  CHECK(o.sdot4(0xff020304u, 0x05fe0708u, 0u) == static_cast<uint32_t>(-5 - 4 + 21 + 32));
  CHECK(o.mulhi(0xffffffffu, 0xffffffffu) == 0xfffffffeu && o.asr64(0x8000000000000000ull, 63) == ~0ull);
  CHECK(o.c.abnormal == 0);
  CHECK(sv::ordered_key(0x3f800000u) == 0xbf800000u && sv::ordered_key(0xbf800000u) == 0x407fffffu);
  CHECK(sv::ordered_key(0x80000000u) + 1 == sv::ordered_key(0u));

  std::string json = "{\"groups\": {";
  std::vector<uint32_t> words(sv::kGroupWords), again(sv::kGroupWords);
  for (int g = 0; g < sv::kNumExact; ++g) {
    sv::Conds c;
    sv::group_expected(g, words.data(), &c);
    CHECK(c.abnormal == 0);
    if (sv::group_is_fp(g)) {
      CHECK(c.eff_add > 0 && c.eff_sub > 0 && c.round_up > 0 && c.round_down > 0);
      LibmOps lo;   // the same chains through libm
      for (int lane = 0; g != sv::kPkFma16 && lane < sv::kLanes; ++lane) {
        uint32_t* w = again.data() + lane * sv::kLaneWords;
        if (g == sv::kFma32) sv::chain_fma32(lo, lane, w);
        else if (g == sv::kFma64) sv::chain_fma64(lo, lane, w);
        else if (g == sv::kPkFma32) sv::chain_pkfma32(lo, lane, w);
        else sv::chain_addmul32(lo, lane, w);
      }
      CHECK(g == sv::kPkFma16 || again == words);
    }
    if (g == sv::kInt32 || g == sv::kInt64) CHECK(c.carry31 > 0 && c.carry63 > 0 && c.borrow63 > 0);
    if (g == sv::kCvt) {
      CHECK(c.round_up > 0 && c.round_down > 0);
      for (int t = 0; t < 5; ++t) CHECK(c.tie_up[t] > 0 && c.tie_down[t] > 0);
    }
    if (g == sv::kXlane)
      for (int a = 0; a < sv::kLanes; ++a)
        for (int b = a + 1; b < sv::kLanes; ++b)
          for (int w = 0; w < sv::kLaneWords; ++w) CHECK(words[a * sv::kLaneWords + w] != words[b * sv::kLaneWords + w]);
    for (int w = 0; w < sv::kLaneWords; ++w) {
      const uint32_t un = sv::uncovered_bits(g, w, words.data());
      if (un) {
        std::fprintf(stderr, "group %s word %d: bits %#010x are constant over the lanes\n", sv::group_name(g), w, un);
        ++failures;
      }
    }
    const uint32_t sum = sp::tile_checksum(words.data(), sv::kGroupWords);
    char buf[320];
    std::snprintf(buf, sizeof buf,
                  "%s\"%s\": {\"checksum\": %u, \"eff_add\": %d, \"eff_sub\": %d, \"round_up\": %d, \"round_down\": %d, "
                  "\"carry31\": %d, \"carry63\": %d, \"borrow63\": %d, \"tie_up\": [%d, %d, %d, %d, %d], "
                  "\"tie_down\": [%d, %d, %d, %d, %d]}",
                  g ? ", " : "", sv::group_name(g), sum, c.eff_add, c.eff_sub, c.round_up, c.round_down, c.carry31, c.carry63,
                  c.borrow63, c.tie_up[0], c.tie_up[1], c.tie_up[2], c.tie_up[3], c.tie_up[4], c.tie_down[0], c.tie_down[1],
                  c.tie_down[2], c.tie_down[3], c.tie_down[4]);
    json += buf;
  }
  const std::vector<uint32_t> table = sv::expected_table();
  CHECK(static_cast<int>(table.size()) == sv::kTableWords);

  // approx: inputs inside the stated intervals, results normal, ranges 2 * kApproxUlps wide
  for (int op = 0; op < sv::kNumApprox; ++op)
    for (int lane = 0; lane < sv::kLanes; ++lane) {
      const double x = sv::bits_float(sv::approx_input(op, lane));
      if (op == sv::kExp2) CHECK(std::fabs(x) <= 20.0 && x != 0.0);
      else if (op == sv::kLog2) CHECK(x >= 2.0 && x <= 1048576.0);
      else CHECK(x >= std::ldexp(1.0, -20) && x <= 1048576.0);
      const float y = static_cast<float>(sv::approx_libm(op, x));
      CHECK(std::isnormal(y));
    }
  const std::vector<uint32_t> ranges = sv::approx_ranges();
  for (size_t i = 0; i < ranges.size(); i += 2) CHECK(ranges[i + 1] - ranges[i] == 2u * sv::kApproxUlps);
  char buf[160];
  std::snprintf(buf, sizeof buf, "}, \"approx_checksum\": %u, \"reg_slots\": %d, \"record_words\": %d}",
                sp::tile_checksum(ranges.data(), sv::kApproxWords), sv::kRegSlots, sv::kValuRecordWords);
  json += buf;

  // register pattern and record
  CHECK(sv::reg_word(3, 200, 0x5eed5eedu, 1) == ~sv::reg_word(3, 200, 0x5eed5eedu, 0));
  CHECK(sv::reg_word(3, 200, 0x5eed5eedu, 0) != sv::reg_word(3, 201, 0x5eed5eedu, 0));
  const uint32_t rec[16] = {2, 0x0000a5b0u, 0x0a0, 0xf, 0, 17, 130, 0x12345678u, 0xffffffffu, 0xffffffffu, 0xffffffffu,
                            0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
  const sv::ValuRecord r0 = sv::decode_valu_record(rec, 0), r1 = sv::decode_valu_record(rec, 1);
  CHECK(nanogpu::selftest::record_written(rec) && !nanogpu::selftest::record_written(rec + sv::kValuRecordWords));
  CHECK(r0.xcc == 2 && r1.fail == sv::kNoBad && r0.bad_slot == 17 && r0.bad_thread == 130 && r0.approx_hash == 0x12345678u);

  if (failures) return 1;
  std::puts(json.c_str());
  return 0;
}
