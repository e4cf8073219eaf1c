// Stand-alone check of the XCD check's host definitions (nanogpu/selftest_xcd_host.h), with no GPU code
// involved: `python native/build.py --selftest-host xcd-asan` builds it under ASan + UBSan. The kernels form
// addresses from indices they read from memory, so before anything runs on a GPU this program asserts, for
// N = 1, 3, 8, 9, 256 and 1,024 workgroups and for directories with every XCD filled, with empty XCDs and with
// one XCD alone, that every access every legal directory can produce lies inside the directory, inside the N
// hand-off slices or inside the N ticket slices, and that an index out of range is refused by the header's checks
// and never becomes a position. It pins spot values and prints, as one JSON line, the checksums and sizes that
// tests/test_selftest_xcd.py compares with the Python twin's.
#include <cstdio>
#include <string>
#include <vector>

#include "nanogpu/selftest_paths_host.h"
#include "nanogpu/selftest_xcd_host.h"

namespace st = nanogpu::selftest;
namespace sx = nanogpu::selftest::xcd;
namespace sp = nanogpu::selftest::paths;

static int failures = 0;

#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);  \
      ++failures;                                                      \
    }                                                                  \
  } while (0)

// The XCD workgroup b of a launch runs on, in four placements: dealt round robin, all on XCD 5, on XCDs 2 and 5
// only, and dealt backwards in runs of three.
static uint32_t placement(int kind, uint32_t b) {
  return kind == 0 ? b % 8 : kind == 1 ? 5u : kind == 2 ? (b % 2 ? 5u : 2u) : 7u - (b / 3) % 8;
}

// The directory the write kernel leaves for n workgroups placed by `kind`, written through the header's offsets.
static std::vector<uint32_t> directory(uint32_t n, int kind) {
  std::vector<uint32_t> dir = sx::dir_initial();
  for (uint32_t b = 0; b < n; ++b) {
    const uint32_t x = placement(kind, b);
    CHECK(sx::xcc_ok(x));
    const uint32_t position = dir[sx::count_at(x)]++;
    CHECK(position < n && sx::list_at(x, position) >= sx::kListAt && sx::list_at(x, position) < sx::kWriterAt);
    dir[sx::list_at(x, position)] = b;
    CHECK(sx::writer_at(b) >= sx::kWriterAt && sx::writer_at(b) + 1 < sx::kMemberAt);
    dir[sx::writer_at(b)] = x;
    dir[sx::writer_at(b) + 1] = 0x100u * b;
  }
  return dir;
}

static void check_bounds(uint32_t n) {
  CHECK(n >= 1 && n <= sx::kMaxBlocks);
  const uint64_t slices = static_cast<uint64_t>(n) * sx::kSliceBytes, tslices = static_cast<uint64_t>(n) * sx::kTicketBytes;
  for (int kind = 0; kind < 4; ++kind) {
    const std::vector<uint32_t> dir = directory(n, kind);
    uint32_t total = 0, empty = 0;
    for (uint32_t x = 0; x < sx::kXcds; ++x) total += dir[sx::count_at(x)], empty += dir[sx::count_at(x)] == 0;
    CHECK(total == n && (kind != 1 || empty == 7) && (kind != 2 || empty >= 6));
    std::vector<uint32_t> read_by(n, 0u);
    // the read kernel: readers placed by another placement than the writers, ordinals as its atomic add deals them
    for (int rkind = 0; rkind < 4; ++rkind) {
      uint32_t readers[sx::kXcds] = {};
      for (uint32_t c = 0; c < n; ++c) {
        const uint32_t y = placement(rkind, c), q = readers[y]++;
        CHECK(sx::readers_at(y) >= sx::kReadersAt && sx::readers_at(y) < sx::kTicketAt);
        for (uint32_t i = 0; i < sx::kXcds; ++i) {
          const uint32_t count = dir[sx::count_at(i)], position = sx::pick_position(n, count, q);
          CHECK((position == sx::kNone) == (count == 0));
          if (position == sx::kNone) continue;
          CHECK(position < count && sx::list_at(i, position) >= sx::kListAt + i * sx::kMaxBlocks && sx::list_at(i, position) < sx::kListAt + (i + 1) * sx::kMaxBlocks);
          const uint32_t block = dir[sx::list_at(i, position)];
          CHECK(sx::block_ok(n, block) && dir[sx::writer_at(block)] == i);
          if (!sx::block_ok(n, block)) continue;
          ++read_by[block];
          for (uint32_t t : {0u, 1u, sx::kThreads - 1})
            for (uint32_t step = 0; step < 4; ++step) CHECK(sx::slice_byte(block, t, step) % 16 == 0 && sx::slice_byte(block, t, step) + 16 <= slices);
        }
      }
    }
    if (kind == 0 && n % 8 == 0)
      for (uint32_t b = 0; b < n; ++b) CHECK(read_by[b] >= 8);   // equal counts: every slice is read from every XCD
  }
  // the last step of the last thread ends the slice; the steps tile it
  CHECK(sx::slice_byte(n - 1, sx::kThreads - 1, 3) + 16 == slices && sx::slice_byte(0, 0, 1) == sx::kThreads * 16);
  // indices out of range never become a position or a block
  for (uint32_t bad : {n + 1, 0x80000000u, 0xffffffffu}) {
    CHECK(!sx::count_ok(n, bad) && sx::pick_position(n, bad, 0) == sx::kNone && sx::pick_position(n, bad, n - 1) == sx::kNone);
    CHECK(!sx::block_ok(n, bad) && !sx::block_ok(n, n));
  }
  CHECK(sx::xcc_ok(7) && !sx::xcc_ok(8) && !sx::xcc_ok(0xffffffffu));
  CHECK(sx::count_ok(n, n) && sx::pick_position(n, n, n - 1) == n - 1 && sx::block_ok(n, n - 1));
  // the ticket kernel
  const uint32_t groups = sx::ticket_groups(n);
  uint32_t members = 0;
  for (uint32_t g = 0; g < groups; ++g) {
    const uint32_t size = sx::group_size(n, g);
    CHECK(size >= 1 && size <= sx::kGroupSize && sx::ticket_at(g) >= sx::kTicketAt && sx::ticket_at(g) < sx::kAtomAt && sx::ticket_at(g) % sx::kLineWords == 0);
    members += size;
    for (uint32_t j = 0; j < size; ++j) {
      const uint32_t block = g * sx::kGroupSize + j;
      CHECK(block < n && sx::member_at(block) >= sx::kMemberAt && sx::member_at(block) + 1 < sx::kDirWords);
      CHECK(sx::ticket_byte(block, sx::kThreads - 1) + 16 <= tslices && sx::ticket_byte(block, 0) % 16 == 0);
    }
  }
  CHECK(members == n && sx::group_size(n, groups - 1) == (n % 8 ? n % 8 : 8));
  // the atomic kernel
  for (uint32_t w = 0; w < sx::kAtomWords; ++w) CHECK(sx::atom_at(w) >= sx::kAtomAt && sx::atom_at(w) + 1 < sx::kListAt && sx::atom_at(w) % sx::kLineWords == 0);
  CHECK(sx::kOrMap + (n - 1) / 32 < sx::kSeenMap && sx::kSeenMap + (4 * n - 1) / 32 < sx::kAtomWords);
}

static uint32_t checksum64(const std::vector<uint64_t>& words) {
  std::vector<uint32_t> halves;
  for (uint64_t w : words) halves.push_back(static_cast<uint32_t>(w)), halves.push_back(static_cast<uint32_t>(w >> 32));
  return sp::tile_checksum(halves.data(), static_cast<int>(halves.size()));
}

int main() {
  const uint32_t seed = 0x1234abcdu;
  // spot values, written out by hand
  CHECK(sx::hand_word(0, 0, 0) == st::mix32(0) && sx::hand_word(seed, 3, 17) == st::mix32((3u << 12 | 17u) ^ seed));
  CHECK(sx::ticket_word(seed, 2, 5, 1) == ~sx::ticket_word(seed, 2, 5, 0));
  CHECK(sx::ticket_word(0, 0, 0, 0) == (st::mix32(0x7e1c4e70u) ^ 0x9e3779b1u));
  CHECK((sx::atom_add64(seed, 7) & 0x80000000u) && (sx::atom_add64(seed, 7) >> 48) == 0);
  CHECK(sx::kDirWords == 22272 && sx::kAtomWords == 168 && sx::kRecordWords == 36);
  CHECK(sx::ticket_groups(1) == 1 && sx::ticket_groups(9) == 2 && sx::group_size(9, 0) == 8 && sx::group_size(9, 1) == 1 && sx::group_size(3, 0) == 3);
  CHECK(sx::pick_position(8, 3, 7) == 1 && sx::pick_position(8, 0, 7) == sx::kNone && sx::pick_position(8, 9, 7) == sx::kNone);
  CHECK(sx::pack_first(1023, 4095) < sx::kNone && sx::pack_first(1, 0) > sx::pack_first(0, 4095));
  {
    const std::vector<uint64_t> one = sx::atomic_expected(seed, 1), three = sx::atomic_expected(seed, 3);
    CHECK(one[sx::kAdd32] == sx::atom_const(seed, 0, 0) && one[sx::kAdd64] == sx::atom_add64(seed, 0) && one[sx::kXor] == sx::atom_const(seed, 0, 3));
    CHECK(one[sx::kCounter] == 4 && one[sx::kOrMap] == 1 && one[sx::kSeenMap] == 0xf && one[sx::kSeenMap + 1] == 0 && one[sx::kOrMap + 1] == 0);
    CHECK(three[sx::kCounter] == 12 && three[sx::kOrMap] == 7 && three[sx::kSeenMap] == 0xfff);
    CHECK(three[sx::kAdd64] >> 32 >= 1);   // three low halves with bit 31 set: a carry crossed bit 32
    CHECK(three[sx::kUmax] >= one[sx::kUmax] && three[sx::kUmin] <= one[sx::kUmin]);
    CHECK(static_cast<int32_t>(three[sx::kSmax]) >= static_cast<int32_t>(one[sx::kSmax]) && static_cast<int32_t>(three[sx::kSmin]) <= static_cast<int32_t>(one[sx::kSmin]));
    const std::vector<uint64_t> full = sx::atomic_expected(seed, 1024);
    CHECK(full[sx::kSeenMap + sx::kSeenMapWords - 1] == 0xffffffffu && full[sx::kOrMap + sx::kOrMapWords - 1] == 0xffffffffu && full[sx::kCounter] == 4096);
    const std::vector<uint32_t> dir = sx::dir_initial();
    CHECK(sx::atom_read(dir.data(), sx::kUmin) == 0xffffffffu && sx::atom_read(dir.data(), sx::kSmin) == 0x7fffffffu && sx::atom_read(dir.data(), sx::kSmax) == 0x80000000u);
  }
  // before and after differ in every word, and no bit of the hand-off pattern is constant over a slice
  {
    uint32_t ones = 0, zeros = 0;
    for (uint32_t i = 0; i < sx::kSliceWords; ++i) ones |= sx::hand_word(seed, 5, i), zeros |= ~sx::hand_word(seed, 5, i);
    CHECK(ones == 0xffffffffu && zeros == 0xffffffffu);
  }
  const uint32_t sizes[] = {1, 3, 8, 9, 256, 1024};
  for (uint32_t n : sizes) check_bounds(n);
  // records
  {
    std::vector<uint32_t> rec(2 * sx::kRecordWords, 0xffffffffu);
    rec[sx::kReadAt] = 3, rec[sx::kReadAt + 1] = 0x400, rec[sx::kReadAt + 2] = 0;
    CHECK(sx::section_written(rec.data(), sx::kReadAt) && !sx::section_written(rec.data(), sx::kWriteAt) && !sx::section_written(rec.data() + sx::kRecordWords, sx::kReadAt));
  }

  std::string json = "{";
  char buf[256];
  std::vector<uint32_t> hand, tick;
  for (uint32_t b : {0u, 5u, 1023u})
    for (uint32_t i = 0; i < sx::kSliceWords; ++i) hand.push_back(sx::hand_word(seed, b, i));
  for (uint32_t b : {0u, 5u, 1023u})
    for (uint32_t after = 0; after < 2; ++after)
      for (uint32_t i = 0; i < sx::kTicketWords; ++i) tick.push_back(sx::ticket_word(seed, b, i, after));
  std::snprintf(buf, sizeof buf, "\"seed\": %u, \"hand_checksum\": %u, \"ticket_checksum\": %u, \"atomic\": {", seed,
                sp::tile_checksum(hand.data(), static_cast<int>(hand.size())), sp::tile_checksum(tick.data(), static_cast<int>(tick.size())));
  json += buf;
  for (size_t k = 0; k < sizeof sizes / sizeof sizes[0]; ++k) {
    std::snprintf(buf, sizeof buf, "%s\"%u\": %u", k ? ", " : "", sizes[k], checksum64(sx::atomic_expected(seed, sizes[k])));
    json += buf;
  }
  std::snprintf(buf, sizeof buf, "}, \"dir_words\": %u, \"atom_words\": %u, \"record_words\": %d, \"slice_bytes\": %u, \"ticket_bytes\": %u, \"dir_checksum\": %u}",
                sx::kDirWords, sx::kAtomWords, sx::kRecordWords, sx::kSliceBytes, sx::kTicketBytes,
                sp::tile_checksum(sx::dir_initial().data(), static_cast<int>(sx::kDirWords)));
  json += buf;
  if (failures) return 1;
  std::puts(json.c_str());
  return 0;
}
