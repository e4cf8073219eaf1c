// Host/device-shared arithmetic of the deep self-test (native/hip/probe_sweep.inc: cu_sweep; probe_hbm.inc:
// hbm_fill, hbm_verify) and the bf16 rounding of the basic one's tile (gemm_tile). Plain C++ with no HIP dependency, so the host side can be built
// and run under sanitizers on its own (native/tests/selftest_host_main.cpp). The Python
// twin of the pattern is nanogpu/probe/selftest.py.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#if defined(__HIPCC__)
#define NANOGPU_HD __host__ __device__
#else
#define NANOGPU_HD
#endif

namespace nanogpu {
namespace selftest {

// ---- memory pattern ---------------------------------------------------------------------
// A fixed 32-bit finaliser (the murmur3 one): every input bit reaches every output bit, so
// neighbouring addresses hold unrelated words.
NANOGPU_HD inline uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x85ebca6bu;
  x ^= x >> 13;
  x *= 0xc2b2ae35u;
  x ^= x >> 16;
  return x;
}

constexpr uint32_t kHiMul = 0x9e3779b1u;

// Word k (0..3) of 16-byte element i. The 64-bit word index w = 4 i + k is split into its
// low and high 32 bits, so no two words of a buffer below 16 TiB share both: the value is a
// function of the whole address, and aliased address lines are caught, not only stuck bits.
// Odd passes hold the complement.
NANOGPU_HD inline uint32_t pattern_word(uint64_t i, uint32_t k, uint32_t seed, uint32_t pass) {
  const uint64_t w = i * 4 + k;
  const uint32_t v = mix32(static_cast<uint32_t>(w) ^ seed) ^ (static_cast<uint32_t>(w >> 32) * kHiMul);
  return (pass & 1u) ? ~v : v;
}

// ---- launch spans ----------------------------------------------------------------------
// hbm_fill and hbm_verify run 256 threads a block and 4 elements a thread. HIP supports no
// launch of 2^32 work-items or more, which a single launch over a buffer of 256 GiB would be,
// so a buffer is covered by one launch after another of at most kMaxLaunchBlocks blocks:
// 64 GiB a launch, the largest single launch measured (profiles/gpu_calibration.md).
constexpr uint64_t kLaunchThreads = 256;
constexpr uint64_t kBlockElements = 4 * kLaunchThreads;
constexpr uint64_t kWorkItemLimit = uint64_t(1) << 32;
constexpr uint64_t kMaxLaunchBlocks = uint64_t(1) << 22;
static_assert(kMaxLaunchBlocks * kLaunchThreads < kWorkItemLimit, "a launch stays below 2^32 work-items");

// (first element, elements) of the launches that tile [0, n_elements) in order: every span is
// max_blocks whole blocks, the last one what is left (its last block may be partial).
// max_blocks in 1..kMaxLaunchBlocks is the caller's to check.
inline std::vector<std::pair<uint64_t, uint64_t>> launch_spans(uint64_t n_elements, uint64_t max_blocks) {
  std::vector<std::pair<uint64_t, uint64_t>> spans;
  const uint64_t step = max_blocks * kBlockElements;
  spans.reserve(static_cast<size_t>((n_elements + step - 1) / step));
  for (uint64_t first = 0; first < n_elements; first += step)
    spans.emplace_back(first, n_elements - first < step ? n_elements - first : step);
  return spans;
}

inline uint64_t span_blocks(uint64_t elements) { return (elements + kBlockElements - 1) / kBlockElements; }

// ---- MFMA chain -------------------------------------------------------------------------
// C = sum over steps s of A_s[32x16] * B_s[16x32], small integers rotated per step:
// |a| <= 3, |b| <= 2, so |C| <= 8 * 16 * 6 = 768 and every fp32 partial sum is exact.
constexpr int kSweepSteps = 8;

NANOGPU_HD inline int sweep_a(int s, int row, int k) { return (row * 5 + k * 3 + s * 2) % 7 - 3; }
NANOGPU_HD inline int sweep_b(int s, int k, int col) { return (k * 3 + col * 2 + s) % 5 - 2; }

// Row-major 32x32 expected tile, in integer arithmetic.
inline void sweep_expected(int32_t out[32 * 32]) {
  for (int r = 0; r < 32; ++r)
    for (int c = 0; c < 32; ++c) {
      int32_t acc = 0;
      for (int s = 0; s < kSweepSteps; ++s)
        for (int k = 0; k < 16; ++k) acc += sweep_a(s, r, k) * sweep_b(s, k, c);
      out[r * 32 + c] = acc;
    }
}

// ---- bf16 operands of the one-tile check -------------------------------------------------
// The bf16 code of a float, round to nearest even (gemm_tile's operands). A finite value beyond
// the largest bf16 rounds to Inf, Inf stays Inf, and a NaN stays a NaN of its sign: its high half
// with the quiet bit set, since the payload may lie in the low half alone (0x7f800001).
inline uint16_t f32_to_bf16_bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return static_cast<uint16_t>((u >> 16) | 0x0040u);
  if ((u & 0x7f800000u) == 0x7f800000u) return static_cast<uint16_t>(u >> 16);
  u += 0x7fffu + ((u >> 16) & 1u);
  return static_cast<uint16_t>(u >> 16);
}

// ---- sweep record -----------------------------------------------------------------------
constexpr int kSweepRecordWords = 5;     // xcc_id, hw_id of wave 0, fail bits, SIMD ids seen, first bad LDS dword
constexpr uint32_t kFailLds = 1u << 4;   // bits 0..3: the MFMA check of wave 0..3
constexpr uint32_t kNoBadOffset = 0xffffffffu;
constexpr uint32_t kRecordUnwritten = 0xffffffffu;   // the host fills the records with 0xff before the launch

// HW_ID (gfx9 family): wave 3:0, SIMD 5:4, pipe 7:6, CU 11:8, SH 12, SE 15:13.
NANOGPU_HD inline uint32_t hw_cu_key(uint32_t hw_id) { return (hw_id >> 8) & 0xffu; }
NANOGPU_HD inline uint32_t hw_simd(uint32_t hw_id) { return (hw_id >> 4) & 3u; }

// Every per-CU record (this one, and selftest_valu_host.h's) begins with xcc, hw_id, fail: `w` is a record's first word.
inline bool record_written(const uint32_t* w) {
  return !(w[0] == kRecordUnwritten && w[1] == kRecordUnwritten && w[2] == kRecordUnwritten);
}

// cu_sweep_paths appends two words (selftest_paths_host.h: kPathRecordWords); a 5-word record has them 0.
struct SweepRecord {
  uint32_t xcc, hw_id, fail, simds, lds_bad, path_fail, path_waves;
};

inline SweepRecord decode_record(const uint32_t* words, size_t block, int record_words) {
  const uint32_t* w = words + block * static_cast<size_t>(record_words);
  const bool paths = record_words > kSweepRecordWords;
  return SweepRecord{w[0], w[1], w[2], w[3], w[4], paths ? w[5] : 0u, paths ? w[6] : 0u};
}

// ---- mismatch slot ----------------------------------------------------------------------
constexpr int kMismatchSlots = 16;

struct Mismatch {
  uint64_t element;
  uint32_t expected, got, word, pad;
};

// Offset of the lowest byte in which the two words differ (little-endian), from the buffer's start.
inline uint64_t mismatch_byte_offset(const Mismatch& m) {
  const uint32_t d = m.expected ^ m.got;
  uint32_t b = 0;
  while (b < 3 && ((d >> (8 * b)) & 0xffu) == 0) ++b;
  return m.element * 16 + m.word * 4 + b;
}

}  // namespace selftest
}  // namespace nanogpu
