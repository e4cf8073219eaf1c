// Stand-alone check of the deep self-test's host arithmetic (nanogpu/selftest_host.h), with
// no GPU code involved: build it with `python native/build.py --selftest-host asan` to run it
// under ASan + UBSan. The pinned pattern values are the ones tests/test_selftest_deep.py pins
// for the Python twin, so the kernels' header and the twin cannot drift apart unnoticed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "nanogpu/selftest_host.h"

namespace st = nanogpu::selftest;

static int failures = 0;

#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);  \
      ++failures;                                                      \
    }                                                                  \
  } while (0)

static float word_float(uint32_t u) {
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}

static bool code_is_nan(uint16_t c) { return (c & 0x7f80u) == 0x7f80u && (c & 0x007fu) != 0; }

// f32_to_bf16_bits written another way: the two bf16 values on either side of f, by truncation, and the
// nearer of them in double arithmetic (the differences of two floats are exact there); a tie goes to
// the even code. The code above the largest finite one is Inf's, 2^128 by its exponent field, so an
// overflowing value rounds to Inf when it is at least half-way there. `f` is no NaN.
static uint16_t bf16_by_distance(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  const uint16_t lo = static_cast<uint16_t>(u >> 16);   // toward zero
  if ((u & 0xffffu) == 0 || (lo & 0x7fffu) == 0x7f80u) return lo;
  const uint16_t hi = static_cast<uint16_t>(lo + 1);    // away from zero: the magnitude is the code's low 15 bits
  const auto value = [](uint16_t c) {
    const int e = (c >> 7) & 0xff, m = c & 0x7f;
    const double mag = e == 0 ? std::ldexp(static_cast<double>(m), -133) : std::ldexp(static_cast<double>(128 + m), e - 134);
    return (c & 0x8000u) ? -mag : mag;
  };
  const double x = static_cast<double>(f), dlo = std::fabs(x - value(lo)), dhi = std::fabs(value(hi) - x);
  if (dlo < dhi) return lo;
  if (dhi < dlo) return hi;
  return (lo & 1u) ? hi : lo;
}

int main() {
  // bf16 rounding: every high half with the low halves that decide a rounding
  {
    const uint32_t lows[] = {0x0000u, 0x0001u, 0x7fffu, 0x8000u, 0x8001u, 0xffffu};
    long cases = 0, nans = 0, ties_up = 0, ties_down = 0, to_inf = 0, carries = 0, bad = 0;
    for (uint32_t high = 0; high < 0x10000u; ++high)
      for (uint32_t low : lows) {
        const uint32_t u = (high << 16) | low;
        const uint16_t got = st::f32_to_bf16_bits(word_float(u));
        ++cases;
        if ((u & 0x7fffffffu) > 0x7f800000u) {   // NaN in: NaN out, same sign
          ++nans;
          if (!(code_is_nan(got) && (got >> 15) == (u >> 31))) ++bad;
          continue;
        }
        const uint16_t want = bf16_by_distance(word_float(u));
        if (got != want) ++bad;
        if (low == 0x8000u) ++(want == high ? ties_down : ties_up);
        if ((want & 0x7fffu) == 0x7f80u && (high & 0x7fffu) != 0x7f80u) ++to_inf;
        if ((want & 0x7fu) == 0 && (high & 0x7fu) == 0x7fu) ++carries;
      }
    CHECK(bad == 0);
    CHECK(cases == 393216);
    CHECK(nans == 2 * (127 * 6 + 5));   // high halves 0x7f81..0x7fff with any low half, 0x7f80 with a non-zero one
    CHECK(ties_up == ties_down && ties_up > 0);
    CHECK(to_inf == 2 * 3);             // 0x7f7f with the low halves 0x8000 and above rounds to Inf, either sign
    CHECK(carries > 0);
    CHECK(st::f32_to_bf16_bits(word_float(0x7f800001u)) == 0x7fc0u);   // payload in the low half alone
    CHECK(st::f32_to_bf16_bits(word_float(0xff800001u)) == 0xffc0u);
    CHECK(st::f32_to_bf16_bits(word_float(0x7f7fffffu)) == 0x7f80u);   // the largest float -> Inf
    CHECK(st::f32_to_bf16_bits(word_float(0x7f7f7fffu)) == 0x7f7fu);   // below half-way: the largest bf16
    CHECK(st::f32_to_bf16_bits(word_float(0x7f800000u)) == 0x7f80u && st::f32_to_bf16_bits(word_float(0xff800000u)) == 0xff80u);
    CHECK(st::f32_to_bf16_bits(word_float(0x00000000u)) == 0x0000u && st::f32_to_bf16_bits(word_float(0x80000000u)) == 0x8000u);
    CHECK(st::f32_to_bf16_bits(word_float(0x3f808000u)) == 0x3f80u);   // tie, even neighbour below
    CHECK(st::f32_to_bf16_bits(word_float(0x3f818000u)) == 0x3f82u);   // tie, even neighbour above
    CHECK(st::f32_to_bf16_bits(word_float(0x3fffffffu)) == 0x4000u);   // carry from the mantissa into the exponent
    CHECK(st::f32_to_bf16_bits(word_float(0x00008000u)) == 0x0000u);   // subnormal tie to +0
    CHECK(st::f32_to_bf16_bits(word_float(0x00008001u)) == 0x0001u);   // the smallest bf16 subnormal
    CHECK(st::f32_to_bf16_bits(word_float(0x007fffffu)) == 0x0080u);   // the largest subnormal float -> the smallest normal
  }

  // pattern
  CHECK(st::mix32(1) == 0x514e28b7u);
  CHECK(st::mix32(0xdeadbeefu) == 0x0de5c6a9u);
  CHECK(st::pattern_word(0, 0, 0, 0) == 0u);
  CHECK(st::pattern_word(0, 3, 0x1234abcdu, 0) == 0x00d1e6ccu);
  CHECK(st::pattern_word(4095, 1, 0x1234abcdu, 1) == 0x72a42e3du);
  CHECK(st::pattern_word(1ull << 30, 2, 7, 0) == 0x523a2a7cu);
  CHECK(st::pattern_word((1ull << 32) + 5, 0, 0x1234abcdu, 0) == 0x47fe4badu);
  CHECK(st::pattern_word((1ull << 32) + 5, 0, 0x1234abcdu, 1) == 0xb801b452u);
  CHECK(st::pattern_word((1ull << 34) + 123456789ull, 3, 0xffffffffu, 2) == 0x71ca6542u);
  for (uint64_t i : {0ull, 77ull, (1ull << 33) + 1})
    for (uint32_t k = 0; k < 4; ++k) CHECK(st::pattern_word(i, k, 9, 1) == ~st::pattern_word(i, k, 9, 0));
  // words 2^32 apart (16 GiB) differ: the high half of the word index is in the value
  CHECK(st::pattern_word(5, 1, 3, 0) != st::pattern_word(5 + (1ull << 30), 1, 3, 0));

  // launch spans: contiguous from 0, whole blocks but the last, within the bound, below 2^32 work-items
  const uint64_t ns[] = {1, 1023, 1024, 1025, (1ull << 34) - 1, 1ull << 34, (1ull << 34) + 1, 19ull << 30};   // 19 * 2^30 elements: 304 GiB
  for (uint64_t max_blocks : {uint64_t(1), uint64_t(3), uint64_t(65535), st::kMaxLaunchBlocks}) {
    CHECK(st::launch_spans(0, max_blocks).empty());
    for (uint64_t n : ns) {
      const auto spans = st::launch_spans(n, max_blocks);
      CHECK(!spans.empty());
      uint64_t next = 0;
      for (size_t j = 0; j < spans.size(); ++j) {
        const uint64_t first = spans[j].first, elements = spans[j].second;
        CHECK(first == next);
        CHECK(elements > 0 && elements <= max_blocks * st::kBlockElements);
        CHECK(first % st::kBlockElements == 0);
        if (j + 1 < spans.size()) CHECK(elements == max_blocks * st::kBlockElements);   // only the last one is short
        CHECK(st::span_blocks(elements) <= max_blocks);
        CHECK(st::span_blocks(elements) * st::kLaunchThreads < st::kWorkItemLimit);
        CHECK(st::span_blocks(elements) * st::kBlockElements >= elements);              // the grid covers the span
        next = first + elements;
      }
      CHECK(next == n);
      CHECK(spans.size() == (n + max_blocks * st::kBlockElements - 1) / (max_blocks * st::kBlockElements));
    }
  }
  CHECK(st::launch_spans(7 * 1024 + 5, 3) ==
        (std::vector<std::pair<uint64_t, uint64_t>>{{0, 3072}, {3072, 3072}, {6144, 1029}}));
  CHECK(st::launch_spans(19ull << 30, st::kMaxLaunchBlocks).size() == 5);   // 304 GiB: 4 launches of 64 GiB and one of 48
  CHECK(st::span_blocks(1) == 1 && st::span_blocks(1024) == 1 && st::span_blocks(1025) == 2);

  // expected tile: operand ranges, the exactness bound, and one entry by hand
  for (int s = 0; s < st::kSweepSteps; ++s)
    for (int i = 0; i < 32; ++i)
      for (int k = 0; k < 16; ++k) {
        CHECK(std::abs(st::sweep_a(s, i, k)) <= 3);
        CHECK(std::abs(st::sweep_b(s, k, i)) <= 2);
      }
  std::vector<int32_t> tile(32 * 32);
  st::sweep_expected(tile.data());
  bool varied = false;
  for (int32_t v : tile) {
    CHECK(std::abs(v) <= 768);
    varied |= v != tile[0];
  }
  CHECK(varied);
  int32_t acc = 0;
  for (int s = 0; s < st::kSweepSteps; ++s)
    for (int k = 0; k < 16; ++k) acc += ((17 * 5 + k * 3 + s * 2) % 7 - 3) * ((k * 3 + 9 * 2 + s) % 5 - 2);
  CHECK(tile[17 * 32 + 9] == acc);

  // record decode
  const uint32_t words[10] = {3, 0x0000a5b0u, 0x12, 0xf, 40959, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu,
                              0xffffffffu};
  const st::SweepRecord r0 = st::decode_record(words, 0, st::kSweepRecordWords),
                        r1 = st::decode_record(words, 1, st::kSweepRecordWords);
  CHECK(st::record_written(words) && !st::record_written(words + st::kSweepRecordWords));
  for (int i = 0; i < 3; ++i) {   // any one of the three leading words changed: written
    uint32_t w[3] = {st::kRecordUnwritten, st::kRecordUnwritten, st::kRecordUnwritten};
    CHECK(!st::record_written(w));
    w[i] ^= 1u << (7 * i);
    CHECK(st::record_written(w));
  }
  CHECK(r0.path_fail == 0 && r0.path_waves == 0);   // a 5-word record has no path words
  CHECK(r0.xcc == 3 && st::hw_cu_key(r0.hw_id) == 0xa5 && st::hw_simd(r0.hw_id) == 3);
  CHECK((r0.fail & st::kFailLds) && (r0.fail & 0xf) == 2 && r0.lds_bad == 40959);

  // mismatch -> byte offset of the lowest differing byte
  CHECK(st::mismatch_byte_offset(st::Mismatch{4096, 0x11223344u, 0x11223354u, 0, 0}) == 4096ull * 16);
  CHECK(st::mismatch_byte_offset(st::Mismatch{2, 0x11223344u, 0x91223344u, 3, 0}) == 2 * 16 + 3 * 4 + 3);
  CHECK(st::mismatch_byte_offset(st::Mismatch{(1ull << 33), 1, 0x101, 1, 0}) == (1ull << 37) + 4 + 1);

  if (failures) return 1;
  std::puts("selftest host arithmetic ok");
  return 0;
}
