// Stand-alone check of the matrix paths' host arithmetic (nanogpu/selftest_paths_host.h), with
// no GPU code involved: `python native/build.py --selftest-host paths-asan` builds it under
// ASan + UBSan. It asserts every path's exactness bound and coverage conditions, pins decoded
// values and a checksum of each expected tile, and prints the checksums as one JSON line,
// which tests/test_selftest_paths.py compares with the Python twin's.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "nanogpu/selftest_paths_host.h"

namespace sp = nanogpu::selftest::paths;

static int failures = 0;

#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);  \
      ++failures;                                                      \
    }                                                                  \
  } while (0)

int main() {
  // decoders, per the OCP definitions
  CHECK(sp::decode_e4m3fn(0x00) == 0.0 && std::signbit(sp::decode_e4m3fn(0x80)));
  CHECK(sp::decode_e4m3fn(0x01) == std::ldexp(1.0, -9));          // smallest subnormal
  CHECK(sp::decode_e4m3fn(0x08) == std::ldexp(1.0, -6));          // smallest normal
  CHECK(sp::decode_e4m3fn(0x38) == 1.0 && sp::decode_e4m3fn(0xbc) == -1.5);
  CHECK(sp::decode_e4m3fn(0x7e) == 448.0 && std::isnan(sp::decode_e4m3fn(0x7f)) && std::isnan(sp::decode_e4m3fn(0xff)));
  CHECK(sp::decode_e5m2(0x01) == std::ldexp(1.0, -16) && sp::decode_e5m2(0x04) == std::ldexp(1.0, -14));
  CHECK(sp::decode_e5m2(0x3c) == 1.0 && sp::decode_e5m2(0xbe) == -1.5 && sp::decode_e5m2(0x7b) == 57344.0);
  CHECK(std::isinf(sp::decode_e5m2(0x7c)) && sp::decode_e5m2(0xfc) < 0 && std::isnan(sp::decode_e5m2(0x7d)));
  CHECK(sp::decode_e2m3(0x00) == 0.0 && sp::decode_e2m3(0x01) == 0.125 && sp::decode_e2m3(0x07) == 0.875);
  CHECK(sp::decode_e2m3(0x08) == 1.0 && sp::decode_e2m3(0x1f) == 7.5 && sp::decode_e2m3(0x3f) == -7.5);
  const double e2m1[8] = {0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0};
  for (int c = 0; c < 8; ++c) {
    CHECK(sp::decode_e2m1(static_cast<uint8_t>(c)) == e2m1[c]);
    CHECK(sp::decode_e2m1(static_cast<uint8_t>(c | 8)) == -e2m1[c]);
  }
  CHECK(sp::decode_e8m0(127) == 1.0 && sp::decode_e8m0(128) == 2.0 && sp::decode_e8m0(120) == std::ldexp(1.0, -7));
  CHECK(sp::decode_e8m0(0) == std::ldexp(1.0, -127) && std::isnan(sp::decode_e8m0(255)));
  // sig * 2^exp with sig odd
  const sp::Dec d = sp::path_decode(sp::kFp8, 0x7e);
  CHECK(d.sig == 7 && d.exp == 6);
  CHECK(sp::path_decode(sp::kI8, 0x80).sig == -1 && sp::path_decode(sp::kI8, 0x80).exp == 7);
  CHECK(sp::dec_value(sp::path_decode(sp::kF16, 0x3c00)) == 1.0 && sp::dec_value(sp::path_decode(sp::kF16, 0xc001)) == -2.001953125);
  CHECK(sp::dec_value(sp::path_decode(sp::kF32, 0x40490fdbu)) == static_cast<double>(3.14159274101257324f));
  CHECK(sp::dec_value(sp::path_decode(sp::kF64, 0x3ff8000000000000ull)) == 1.5);

  // generators: the packed dwords and the per-code view agree; opsel reaches every byte
  CHECK(sp::path_code(sp::kMxFp6, 0, 3, 7, 5) ==
        (((static_cast<uint64_t>(sp::path_dword(sp::kMxFp6, 0, 3, 7, 1)) << 32 | sp::path_dword(sp::kMxFp6, 0, 3, 7, 0)) >> 30) & 0x3f));
  CHECK((sp::path_code(sp::kF16, 0, 0, 2, 0) >> 10 & 0x1f) == 16 && sp::path_code(sp::kF16, 0, 1, 2, 0) == 0);
  CHECK((sp::path_code(sp::kF32, 1, 0, 9, 0) & 0x7fffffffu) == 0x3f800000u);
  uint32_t bytes_used = 0;
  for (int s = 0; s < sp::kPathSteps; ++s) bytes_used |= 1u << sp::path_opsel(0, s) | 1u << sp::path_opsel(1, s);
  CHECK(bytes_used == 0xf);

  // every path: exactness bound, coverage, pinned checksum
  const uint32_t pinned[sp::kNumPaths] = {0xcfef13d6u, 0x463d5c6bu, 0xaa2486afu, 0xfdf409a7u, 0xf6ca01cbu,
                                          0x5cce04a9u, 0x48843475u, 0xe1d698bcu, 0x82c5fef6u};
  std::string json = "{";
  for (int p = 0; p < sp::kNumPaths; ++p) {
    const sp::PathTile t = sp::path_expected(p);
    CHECK(!t.overflow);
    CHECK(t.exact());
    CHECK(t.sum_abs_max > 0 && t.sum_abs_max < (int64_t(1) << sp::path_limit_bits(p)));
    CHECK(sp::path_coverage(p) == 0);
    CHECK(static_cast<int>(t.units.size()) == sp::path_dim(p) * sp::path_dim(p));
    bool varied = false;
    for (int64_t v : t.units) varied |= v != t.units[0];
    CHECK(varied);
    std::vector<uint32_t> words(sp::kTileWords);
    sp::path_expected_words(p, t, words.data());
    const uint32_t sum = sp::tile_checksum(words.data(), sp::path_tile_words(p));
    if (sum != pinned[p]) {
      std::fprintf(stderr, "path %s: checksum %#010x, pinned %#010x\n", sp::path_name(p), sum, pinned[p]);
      ++failures;
    }
    char buf[160];
    std::snprintf(buf, sizeof buf, "%s\"%s\": {\"checksum\": %u, \"unit_exp\": %d, \"sum_abs_max\": %lld}", p ? ", " : "",
                  sp::path_name(p), sum, t.unit_exp, static_cast<long long>(t.sum_abs_max));
    json += buf;
  }
  json += "}";

  // record decode
  const uint32_t words[14] = {3, 0x0000a5b0u, 0, 0xf, 0xffffffffu, 0x41, 0x5, 0xffffffffu, 0xffffffffu, 0xffffffffu,
                              0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
  namespace st = nanogpu::selftest;
  const st::SweepRecord r0 = st::decode_record(words, 0, sp::kPathRecordWords),
                        r1 = st::decode_record(words, 1, sp::kPathRecordWords);
  CHECK(st::record_written(words) && !st::record_written(words + sp::kPathRecordWords) && r1.xcc == st::kRecordUnwritten);
  CHECK(r0.xcc == 3 && r0.path_fail == ((1u << sp::kF16) | (1u << sp::kMxFp4)) && r0.path_waves == 5);
  const st::SweepRecord r5 = st::decode_record(words, 0, st::kSweepRecordWords);   // the same words as a plain record
  CHECK(r5.xcc == 3 && r5.path_fail == 0 && r5.path_waves == 0);

  if (failures) return 1;
  std::puts(json.c_str());
  return 0;
}
