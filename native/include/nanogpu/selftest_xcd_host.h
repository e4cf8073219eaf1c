// Host/device-shared arithmetic of the deep self-test's XCD check (native/hip/probe_xcd.inc: xcd_write_kernel,
// xcd_read_kernel, xcd_ticket_kernel, xcd_atomic_kernel): data that one XCD wrote, read on another, by a hand-off
// across a kernel boundary, by release, ticket and acquire inside one kernel, and by memory-side atomics from every
// XCD onto the same words. Plain C++ with no HIP dependency, so that the host side can be built and run under
// sanitizers on its own (native/tests/selftest_xcd_host_main.cpp). The Python twin is nanogpu/probe/selftest_xcd.py.
//
// Every index a kernel reads from memory (a count, a list position, a block number, a ticket, a counter value) goes
// through one of the range checks below before it becomes part of an address: the memory those indices live in is
// the thing under test.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "nanogpu/selftest_host.h"

namespace nanogpu {
namespace selftest {
namespace xcd {

// ---- names ------------------------------------------------------------------------------------
enum Group { kHandoff = 0, kTicket, kAtomic, kNumNames };
constexpr uint32_t kAllGroups = (1u << kNumNames) - 1;
inline const char* group_name(int g) {
  constexpr const char* names[kNumNames] = {"handoff", "ticket", "atomic"};
  return names[g];
}

// failed kinds of a record's section
constexpr uint32_t kKindData = 1u << 0;      // a word of a slice is not the pattern's
constexpr uint32_t kKindDir = 1u << 1;       // an index read from memory is out of range
constexpr uint32_t kKindWriter = 1u << 2;    // writer[] does not name the XCD whose list holds the block
constexpr uint32_t kKindPreread = 1u << 3;   // ticket: a word read before the ticket is neither the before nor the after word
constexpr uint32_t kKindDup = 1u << 4;       // atomic: a bit that this workgroup alone sets was set already
constexpr uint32_t kAllKinds = (1u << 5) - 1;
constexpr int kNumKinds = 5;
inline const char* kind_name(int k) {
  constexpr const char* names[kNumKinds] = {"data", "dir", "writer", "preread", "dup"};
  return names[k];
}

// ---- sizes ------------------------------------------------------------------------------------
constexpr uint32_t kXcds = 8;
constexpr uint32_t kThreads = 256;
constexpr uint32_t kMaxRounds = 4;             // 4 rounds x 32 CUs x 16 KiB = 2 MiB an XCD: under its 4 MiB L2
constexpr uint32_t kMaxBlocks = 1024;          // 4 rounds x 256 CUs
constexpr uint32_t kSliceWords = 4096;         // hand-off: 16 KiB a workgroup
constexpr uint32_t kSliceBytes = kSliceWords * 4;
constexpr uint32_t kTicketWords = 1024;        // ticket: 4 KiB a workgroup
constexpr uint32_t kTicketBytes = kTicketWords * 4;
constexpr uint32_t kGroupSize = 8;             // workgroups 8g .. 8g+7 share ticket[g]
constexpr uint32_t kLineWords = 32;            // 128 bytes
constexpr uint32_t kNone = 0xffffffffu;
static_assert(kSliceWords % (4 * kThreads) == 0 && kTicketWords == 4 * kThreads, "16 bytes a thread a step");
static_assert(kNone == kNoBadOffset, "one 'none' word in every record");

NANOGPU_HD inline uint32_t ticket_groups(uint32_t n) { return (n + kGroupSize - 1) / kGroupSize; }
NANOGPU_HD inline uint32_t group_size(uint32_t n, uint32_t g) { return n - g * kGroupSize < kGroupSize ? n - g * kGroupSize : kGroupSize; }

// ---- the atomic words -------------------------------------------------------------------------
// Each on its own 128-byte line. Word kAdd64 is 64 bits wide, every other one 32.
enum AtomWord { kAdd32 = 0, kAdd64, kXor, kUmax, kSmax, kUmin, kSmin, kCounter, kOrMap };
constexpr uint32_t kOrMapWords = kMaxBlocks / 32;          // bit b: workgroup b
constexpr uint32_t kSeenMap = kOrMap + kOrMapWords;        // bit t: the counter returned t
constexpr uint32_t kSeenMapWords = 4 * kMaxBlocks / 32;    // lane 0 of each of the 4 waves increments
constexpr uint32_t kAtomWords = kSeenMap + kSeenMapWords;
static_assert(kAtomWords == 168, "8 single words and two bitmaps");

// ---- the directory ----------------------------------------------------------------------------
// One array of 32-bit words, the same layout for every N <= kMaxBlocks.
constexpr uint32_t kCountAt = 0;                                        // count[x]: writers of XCD x, a line each
constexpr uint32_t kReadersAt = kCountAt + kXcds * kLineWords;          // readers[x]: ordinals of XCD x's readers
constexpr uint32_t kTicketAt = kReadersAt + kXcds * kLineWords;         // ticket[g], a line each
constexpr uint32_t kAtomAt = kTicketAt + (kMaxBlocks / kGroupSize) * kLineWords;
constexpr uint32_t kListAt = kAtomAt + kAtomWords * kLineWords;         // list[x][position] = block
constexpr uint32_t kWriterAt = kListAt + kXcds * kMaxBlocks;            // writer[b] = (xcc, hw_id)
constexpr uint32_t kMemberAt = kWriterAt + 2 * kMaxBlocks;              // member[b] = (xcc + 1, hw_id) of the ticket kernel
constexpr uint32_t kDirWords = kMemberAt + 2 * kMaxBlocks;
static_assert(kDirWords == 22272 && kAtomAt % kLineWords == 0 && kAtomAt % 2 == 0, "lines; the 64-bit word is aligned");

NANOGPU_HD inline uint32_t count_at(uint32_t x) { return kCountAt + x * kLineWords; }
NANOGPU_HD inline uint32_t readers_at(uint32_t x) { return kReadersAt + x * kLineWords; }
NANOGPU_HD inline uint32_t ticket_at(uint32_t g) { return kTicketAt + g * kLineWords; }
NANOGPU_HD inline uint32_t atom_at(uint32_t w) { return kAtomAt + w * kLineWords; }
NANOGPU_HD inline uint32_t list_at(uint32_t x, uint32_t position) { return kListAt + x * kMaxBlocks + position; }
NANOGPU_HD inline uint32_t writer_at(uint32_t b) { return kWriterAt + 2 * b; }
NANOGPU_HD inline uint32_t member_at(uint32_t b) { return kMemberAt + 2 * b; }

// ---- range checks of what a kernel reads from memory --------------------------------------------
NANOGPU_HD inline bool xcc_ok(uint32_t xcc) { return xcc < kXcds; }
NANOGPU_HD inline bool block_ok(uint32_t n, uint32_t block) { return block < n; }
NANOGPU_HD inline bool count_ok(uint32_t n, uint32_t count) { return count <= n; }
// The list position reader ordinal q of an XCD takes of an XCD with `count` writers: kNone when it has none, or when
// the count is out of range (then count_ok is false too).
NANOGPU_HD inline uint32_t pick_position(uint32_t n, uint32_t count, uint32_t q) {
  return count == 0 || !count_ok(n, count) ? kNone : q % count;
}

// ---- patterns ---------------------------------------------------------------------------------
// Word i of workgroup b's hand-off slice.
NANOGPU_HD inline uint32_t hand_word(uint32_t seed, uint32_t b, uint32_t i) { return mix32(((b << 12) | i) ^ seed); }
// Word i of workgroup b's ticket slice: `after` 0 before the workgroup's own store, 1 after it (the complement).
NANOGPU_HD inline uint32_t ticket_word(uint32_t seed, uint32_t b, uint32_t i, uint32_t after) {
  const uint32_t v = mix32(((b << 10) | i) ^ seed ^ 0x7e1c4e70u) ^ kHiMul;
  return after ? ~v : v;
}
// Constant k of workgroup b for the atomic words.
NANOGPU_HD inline uint32_t atom_const(uint32_t seed, uint32_t b, uint32_t k) { return mix32(mix32(b * 8 + k + 0xa7000000u) ^ seed); }
// The 64-bit addend: bit 31 of the low half is set, so the sum of any two carries across bit 32.
NANOGPU_HD inline uint64_t atom_add64(uint32_t seed, uint32_t b) {
  return (static_cast<uint64_t>(atom_const(seed, b, 1) & 0xffffu) << 32) | (atom_const(seed, b, 2) | 0x80000000u);
}

// What the directory holds before the kernels run: zero but for the min / max words.
inline uint64_t atom_initial(uint32_t w) {
  return w == kSmax ? 0x80000000u : w == kUmin ? 0xffffffffu : w == kSmin ? 0x7fffffffu : 0u;
}

// The final atomic words after n workgroups: functions of seed and n alone.
inline std::vector<uint64_t> atomic_expected(uint32_t seed, uint32_t n) {
  std::vector<uint64_t> w(kAtomWords);
  for (uint32_t i = 0; i < kAtomWords; ++i) w[i] = atom_initial(i);
  for (uint32_t b = 0; b < n; ++b) {
    w[kAdd32] = static_cast<uint32_t>(w[kAdd32] + atom_const(seed, b, 0));
    w[kAdd64] += atom_add64(seed, b);
    w[kXor] ^= atom_const(seed, b, 3);
    const uint32_t umax = atom_const(seed, b, 4), smax = atom_const(seed, b, 5), umin = atom_const(seed, b, 6), smin = atom_const(seed, b, 7);
    if (umax > w[kUmax]) w[kUmax] = umax;
    if (static_cast<int32_t>(smax) > static_cast<int32_t>(static_cast<uint32_t>(w[kSmax]))) w[kSmax] = smax;
    if (umin < w[kUmin]) w[kUmin] = umin;
    if (static_cast<int32_t>(smin) < static_cast<int32_t>(static_cast<uint32_t>(w[kSmin]))) w[kSmin] = smin;
    w[kOrMap + b / 32] |= 1u << (b % 32);
  }
  w[kCounter] = 4 * n;
  for (uint32_t t = 0; t < 4 * n; ++t) w[kSeenMap + t / 32] |= 1u << (t % 32);
  return w;
}

// The directory's initial words.
inline std::vector<uint32_t> dir_initial() {
  std::vector<uint32_t> d(kDirWords, 0u);
  for (uint32_t w = 0; w < kAtomWords; ++w) {
    d[atom_at(w)] = static_cast<uint32_t>(atom_initial(w));
    d[atom_at(w) + 1] = static_cast<uint32_t>(atom_initial(w) >> 32);
  }
  return d;
}

inline uint64_t atom_read(const uint32_t* dir, uint32_t w) {
  return dir[atom_at(w)] | (w == kAdd64 ? static_cast<uint64_t>(dir[atom_at(w) + 1]) << 32 : 0u);
}

// ---- record -----------------------------------------------------------------------------------
// One record a workgroup, one section a kernel: workgroup b of each kernel writes section b's words, so a section
// names the CU that ran that kernel's workgroup b. A section of a kernel that did not run stays 0xff.
constexpr int kWriteAt = 0;      // xcc, hw_id, kinds, list position
constexpr int kReadAt = 4;       // xcc, hw_id, kinds, writer XCDs verified, writer XCDs failed, ordinal, then First
constexpr int kTickAt = 16;      // xcc, hw_id, kinds, last arriver, ticket, slices verified, writer XCDs verified, failed, then First, fold
constexpr int kAtomRecAt = 32;   // xcc, hw_id, kinds, duplicates
constexpr int kRecordWords = 36;
constexpr int kReadFirst = kReadAt + 6, kTickFirst = kTickAt + 8, kTickFold = kTickAt + 14;
// First: the first failure (lowest writer block, then lowest word): block, the writer's xcc and hw_id, word, expected, observed.
constexpr int kFirstWords = 6;
static_assert(kReadFirst + kFirstWords == kTickAt && kTickFold + 1 < kAtomRecAt + 0 && kAtomRecAt + 4 == kRecordWords, "the sections do not meet");

NANOGPU_HD inline uint32_t pack_first(uint32_t block, uint32_t word) { return (block << 12) | word; }   // block < 2^10, word < 2^12
static_assert(kMaxBlocks <= 1u << 10 && kSliceWords <= 1u << 12, "pack_first");

inline bool section_written(const uint32_t* record, int at) { return record_written(record + at); }

// ---- what one launch touches, for the bounds proof -----------------------------------------------
// Byte ranges [at, at + bytes) of the three buffers, as the kernels form them.
NANOGPU_HD inline uint64_t slice_byte(uint32_t block, uint32_t thread, uint32_t step) {   // the 16 bytes thread `thread` moves in step 0..3
  return static_cast<uint64_t>(block) * kSliceBytes + (static_cast<uint64_t>(step) * kThreads + thread) * 16;
}
NANOGPU_HD inline uint64_t ticket_byte(uint32_t block, uint32_t thread) { return static_cast<uint64_t>(block) * kTicketBytes + static_cast<uint64_t>(thread) * 16; }

}  // namespace xcd
}  // namespace selftest
}  // namespace nanogpu
