// Stand-alone check of the memory self-test's host definitions (nanogpu/selftest_mem_host.h), with no
// GPU code involved: `python native/build.py --selftest-host mem-asan` builds it under ASan + UBSan.
// A wrong address in the kernel's asm statements would be a GPU fault, so before anything runs on a
// GPU this program asserts, for every (group, wave, lane, step), that the accessed range is aligned
// to its size and lies inside the table, inside the wave's region of the workgroup's slice, or
// inside the wave's region of the kernel's LDS array. It also asserts the header's other
// conditions (store maps injective, every byte offset and both signs in the sub-dword loads, every
// buffer instruction with lanes in range and out of range up to the boundary, min and max picking
// each side, cmpswap succeeding and failing, inc and dec wrapping and not, no constant bit in the
// compared data), pins spot values, and prints each group's checksum and the sizes as one JSON line,
// which tests/test_selftest_mem.py compares with the Python twin's.
#include <cstdio>
#include <set>
#include <string>
#include <vector>

#include "nanogpu/selftest_mem_host.h"
#include "nanogpu/selftest_paths_host.h"

namespace sm = nanogpu::selftest::mem;
namespace sp = nanogpu::selftest::paths;

static int failures = 0;

#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond);  \
      ++failures;                                                      \
    }                                                                  \
  } while (0)

static void check_accesses() {
  CHECK(sm::kWaves * sm::kLdsWaveBytes + 16 <= sm::kLdsArrayBytes && sm::kWaves * sm::kWaveBytes == sm::kSliceBytes && sm::kSliceBytes <= 8192);
  for (int g = 0; g < sm::kNumNames; ++g)
    for (int wave = 0; wave < sm::kWaves; ++wave)
      for (int lane = 0; lane < sm::kLanes; ++lane)
        sm::for_each_access(g, wave, lane, [&](const sm::Access& a) {
          const uint32_t limit = a.space == sm::kTable ? sm::kTableBytes : a.space == sm::kSlice ? sm::kWaveBytes : sm::kLdsWaveBytes;
          const bool ok = a.bytes > 0 && a.at % a.align == 0 && a.at + a.bytes <= limit && !(a.space == sm::kTable && a.store);
          if (!ok) {
            std::fprintf(stderr, "group %s wave %d lane %d: %u bytes at %u of space %d\n", sm::group_name(g), wave, lane, a.bytes, a.at, a.space);
            ++failures;
          }
        });
  // the st64 forms and the 2-address reads stay inside the region as well
  for (int m = 0; m < sm::kLdsMaps; ++m)
    for (int lane = 0; lane < sm::kLanes; ++lane) CHECK(sm::lds_chunk(m, lane) + 16 <= sm::kLdsUpper && 2 * sm::kLdsUpper <= sm::kLdsWaveBytes);
}

static void check_injective() {
  for (int wave = 0; wave < sm::kWaves; ++wave)
    for (int f = 0; f < sm::kGstoreForms; ++f) {
      std::set<uint32_t> seen;
      for (int lane = 0; lane < sm::kLanes; ++lane) {
        seen.insert(sm::gstore_chunk(wave, lane, f));
        CHECK(sm::gstore_sub(lane, f) + sm::gstore_bytes(f) <= 16 && sm::gstore_sub(lane, f) % (sm::gstore_bytes(f) == 12 ? 16 : sm::gstore_bytes(f)) == 0);
      }
      CHECK(seen.size() == 64);
    }
  for (int m = 0; m < sm::kLdsMaps; ++m) {
    std::set<uint32_t> seen;
    for (int lane = 0; lane < sm::kLanes; ++lane) seen.insert(sm::lds_chunk(m, lane));
    CHECK(seen.size() == 64);
  }
  for (int lane = 0; lane < 32; ++lane)   // map 2: a half-wave on one of the 32 banks a write and a 32-bit read see
    CHECK((sm::lds_chunk(2, lane) / 4) % 32 == 0 && (sm::lds_chunk(2, lane + 32) / 4) % 32 == 4);
  for (int map = 0; map < sm::kGloadMaps; ++map)
    for (int f = 0; f < sm::kGloadForms; ++f) {
      std::set<uint32_t> lines;
      for (int lane = 0; lane < sm::kLanes; ++lane) lines.insert(sm::gload_chunk(map, 1, lane, f) / 128);
      CHECK(map == 0 ? lines.size() <= 9 : lines.size() == 64);   // unit stride: 8 lanes a line; map 1: a line a lane
    }
  for (int f = 0; f + 1 < sm::kDmaForms; ++f) CHECK(sm::dma_dst(f) + 64 * 16 <= sm::dma_dst(f + 1));
  for (int s = 0; s < sm::kLdstrSteps; ++s) {
    std::set<uint32_t> seen;
    for (int lane = 0; lane < sm::kLanes; ++lane) seen.insert(sm::ldstr_addr(s, lane));
    CHECK(seen.size() == 64 && sm::ldstr_stride(s) % 8 == 0 && sm::ldstr_stride(s) >= 32);
  }
  // l1: each pass reads every word of the table exactly once, in different orders
  for (int p = 0; p < sm::kL1Passes; ++p) {
    std::set<uint32_t> seen;
    for (int s = 0; s < sm::kL1Steps; ++s)
      for (int lane = 0; lane < sm::kLanes; ++lane) seen.insert(sm::l1_chunk(p, s, lane));
    CHECK(seen.size() == sm::kTableWords / 4 && *seen.rbegin() == sm::kTableWords / 4 - 1);
  }
  CHECK(sm::l1_chunk(0, 0, 5) != sm::l1_chunk(1, 0, 5));
}

static void check_subdword() {
  std::set<int> byte_offsets, short_offsets;
  for (int f = 0; f < 8; ++f) byte_offsets.insert(sm::gload_sub(f) & 3);
  for (int f = 8; f < 12; ++f) short_offsets.insert(sm::gload_sub(f) & 3);
  CHECK(byte_offsets == (std::set<int>{0, 1, 2, 3}) && short_offsets == (std::set<int>{0, 2}));
  for (int f : {4, 5, 6, 7, 10, 11, 14, 15}) {   // the sign-extending forms: both signs, in every wave
    for (int wave = 0; wave < sm::kWaves; ++wave) {
      int neg = 0, pos = 0;
      for (int map = 0; map < sm::kGloadMaps; ++map)
        for (int lane = 0; lane < sm::kLanes; ++lane) {
          const uint32_t v = sm::gload_expected(map, wave, lane, f, 0);
          const bool n = f >= 14 ? (v & 0x8000u) != 0 : (v >> 31) != 0;   // a d16 form's value is its 16 bits
          ++(n ? neg : pos);
        }
      CHECK(neg > 0 && pos > 0);
    }
  }
  for (int f : {1, 3})
    for (int wave = 0; wave < sm::kWaves; ++wave) {
      int neg = 0, pos = 0;
      std::set<uint32_t> offs;
      for (int lane = 0; lane < sm::kLanes; ++lane) {
        ++((sm::lds_read_expected(wave, lane, 0, f, 0) >> 31) ? neg : pos);
        offs.insert(static_cast<uint32_t>(sm::lds_read_sub(lane, f)) & 3u);
      }
      CHECK(neg > 0 && pos > 0 && offs.size() == (f == 1 ? 4u : 2u));
    }
}

static void check_buffer() {
  for (int w = 0; w < sm::kBufWidths; ++w)
    for (int m = 0; m < sm::kBufModes; ++m) {
      const uint32_t imm = m == 2 ? sm::kBufImm : 0u, soff = m == 1 ? sm::kBufSoffset : 0u;
      int in = 0, out = 0;
      for (int lane = 0; lane < sm::kLanes; ++lane) {
        const uint32_t vo = sm::buf_voffset(w, m, lane), n = static_cast<uint32_t>(sm::buf_bytes(w));
        CHECK(vo + imm + soff == sm::buf_addr(w, m, lane) && vo % (n == 12 ? 16 : n) == 0);
        // in range only if so with soffset counted, out of range only if so without it: no partly covered access
        const bool inside = vo + imm + soff + n <= sm::kBufRecords, outside = vo + imm >= sm::kBufRecords;
        CHECK(inside != outside && inside == sm::buf_in_range(lane));
        ++(inside ? in : out);
      }
      CHECK(in == 32 && out == 32);
      CHECK(sm::buf_addr(w, m, 31) + sm::buf_stride(w) == sm::kBufRecords);             // the last slot in range
      CHECK(sm::buf_voffset(w, m, 32) + imm == sm::kBufRecords);                        // the first byte out of range
    }
  // a store of an out-of-range lane leaves the background; of an in-range one its bytes and no others
  CHECK(sm::buf_store_expected(0, 40, 2, 0, 1) == sm::buf_bg(0, 1 + 3 * 2 + 0, (sm::buf_addr(2, 0, 40) & ~15u) / 4 + 1));
  CHECK(sm::buf_store_expected(0, 3, 2, 0, 3) == sm::buf_val(0, 3, 2, 0, 0) && sm::buf_load_expected(1, 32, 5, 2, 0) == 0u);
  CHECK(sm::buf_store_expected(2, 5, 4, 1, 3) == sm::buf_bg(2, 1 + 3 * 4 + 1, sm::buf_addr(4, 1, 5) / 4 + 3));   // the 4th word of a 12-byte slot
}

static void check_atomics() {
  for (int m = 0; m < 2; ++m)
    for (int wave = 0; wave < sm::kWaves; ++wave) {
      for (int op : {sm::kSmin, sm::kUmin, sm::kSmax, sm::kUmax, sm::kUmax64}) {
        int kept = 0, taken = 0;
        for (int lane = 0; lane < sm::kLanes; ++lane) {
          CHECK(sm::atom_a(m, wave, lane, op) != sm::atom_v(m, wave, lane, op));
          ++(sm::atom_after(m, wave, lane, op) == sm::atom_a(m, wave, lane, op) ? kept : taken);
        }
        CHECK(kept > 0 && taken > 0);
      }
      for (int op : {sm::kCmpswap, sm::kCmpswap64, sm::kInc, sm::kDec}) {
        int one = 0, other = 0;
        for (int lane = 0; lane < sm::kLanes; ++lane) {
          const uint64_t a = sm::atom_a(m, wave, lane, op), v = sm::atom_v(m, wave, lane, op), after = sm::atom_after(m, wave, lane, op);
          const bool first = op == sm::kInc ? after == 0 : op == sm::kDec ? after == v : after == v && a != v;
          ++(first ? one : other);
          if (op == sm::kInc) CHECK(after == 0 || after == a + 1);
          if (op == sm::kDec) CHECK(after == v || after == a - 1);
        }
        CHECK(one > 0 && other > 0);
      }
      const uint32_t b = sm::atom_cont_b(m, wave), c = sm::atom_cont_c(m, wave);
      CHECK(b + 64ull * c < (1ull << 32) && (c & 1u) && sm::atom_cont_q(m, wave, b + 63 * c) == 63 && sm::atom_cont_q(m, wave, b + 64 * c) == sm::kNoBad &&
            sm::atom_cont_q(m, wave, b + 1) == (c == 1 ? 1u : sm::kNoBad));
    }
}

int main() {
  // spot values, written out by hand
  CHECK(sm::sext8(0x80u) == 0xffffff80u && sm::sext8(0x7fu) == 0x7fu && sm::sext16(0x8000u) == 0xffff8000u);
  CHECK(sm::table_word(0) == nanogpu::selftest::mix32(sm::kSalt) && sm::table_byte(5) == ((sm::table_word(1) >> 8) & 0xffu));
  {
    const uint32_t src[4] = {0x44332211u, 0x88776655u, 0xccbbaa99u, 0x00ffeeddu};
    auto s = [&](int i) { return src[i]; };
    CHECK(sm::overlay(0xa0b0c0d0u, 0, 1, 2, s) == 0xa02211d0u);             // 2 bytes at byte 1 of word 0
    CHECK(sm::overlay(0xa0b0c0d0u, 1, 3, 4, s) == 0xa0443322u);             // 4 bytes at byte 3: the last three reach word 1
    CHECK(sm::overlay(0xa0b0c0d0u, 3, 0, 12, s) == 0xa0b0c0d0u && sm::overlay(0xa0b0c0d0u, 2, 0, 12, s) == 0xccbbaa99u);
  }
  CHECK(sm::gload_first(25) + 4 == sm::kGloadMapWords && sm::lds_read_first(11) + 4 == sm::kLdsReadMapWords);
  CHECK(sm::group_words(sm::kBuffer) == 108 && sm::group_words(sm::kLds) == 222 && sm::group_words(sm::kAtomic) == 92 && sm::kAtomMemWords == 46);
  for (int g = 0; g < sm::kNumNames; ++g) CHECK(sm::group_words(g) <= sm::kMaxGroupWords);
  // ldstr: lane 0 of group 0 receives column 0 of rows 0..3; lane 17 (group 1, i = 1) column 1 of rows 4..7
  CHECK(sm::ldstr_expected(2, 0, 0, 0) == (sm::ldstr_elem(2, 0, 0, 0) | sm::ldstr_elem(2, 0, 1, 0) << 16));
  CHECK(sm::ldstr_expected(2, 1, 17, 1) == (sm::ldstr_elem(2, 1, 6, 1) | sm::ldstr_elem(2, 1, 7, 1) << 16));
  CHECK(sm::ldstr_addr(1, 23) == (4 * 1 + 1) * 48 + 8 * 3);                  // lane 23 = 16 + 4 * 1 + 3: row 5, columns 12..15
  CHECK(sm::ldstr_written(0, 0, 23, 1) == (sm::ldstr_elem(0, 0, 5, 14) | sm::ldstr_elem(0, 0, 5, 15) << 16));
  check_accesses();
  check_injective();
  check_subdword();
  check_buffer();
  check_atomics();

  std::string json = "{\"groups\": {";
  for (int g = 0; g < sm::kNumNames; ++g) {
    const std::vector<uint32_t> words = sm::group_expected(g);
    const uint32_t un = sm::uncovered_bits(words);
    if (un) {
      std::fprintf(stderr, "group %s: bits %#010x are the same in all %zu words\n", sm::group_name(g), un, words.size());
      ++failures;
    }
    char buf[96];
    std::snprintf(buf, sizeof buf, "%s\"%s\": [%d, %u]", g ? ", " : "", sm::group_name(g), sm::group_words(g),
                  sp::tile_checksum(words.data(), static_cast<int>(words.size())));
    json += buf;
  }
  const std::vector<uint32_t> table = sm::mem_table();
  for (int i = 0; i < sm::kTableWords; ++i)   // no two words at indices differing in one bit are equal
    for (int b = 1; b < sm::kTableWords; b <<= 1) CHECK(table[i] != table[i ^ b]);
  const uint32_t rec[16] = {2, 0x0000a5b0u, 0x4, 0xf, 0x2, 1, 4097, 2, 0xffffffffu, 0xffffffffu, 0xffffffffu,
                            0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
  const sm::MemRecord r0 = sm::decode_mem_record(rec, 0), r1 = sm::decode_mem_record(rec, 1);
  CHECK(nanogpu::selftest::record_written(rec) && !nanogpu::selftest::record_written(rec + sm::kMemRecordWords));
  CHECK(r0.xcc == 2 && r0.bad_group == 1 && r0.bad_index == 4097 && r0.bad_wave == 2 && r1.fail == sm::kNoBad);
  CHECK(sm::pack_bad(0, 5631, 3) < sm::pack_bad(1, 0, 0) && sm::pack_bad(7, 14207, 3) < sm::kNoBad);

  char buf[200];
  std::snprintf(buf, sizeof buf, "}, \"table_checksum\": %u, \"table_words\": %d, \"slice_bytes\": %u, \"record_words\": %d}",
                sp::tile_checksum(table.data(), sm::kTableWords), sm::kTableWords, sm::kSliceBytes, sm::kMemRecordWords);
  json += buf;
  if (failures) return 1;
  std::puts(json.c_str());
  return 0;
}
