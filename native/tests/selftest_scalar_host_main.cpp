// Stand-alone check of the scalar self-test's host arithmetic (nanogpu/selftest_scalar_host.h), with
// no GPU code involved: `python native/build.py --selftest-host scalar-asan` builds it under ASan +
// UBSan. It asserts the header's conditions (every result bit takes both values in every group,
// every SCC is consumed as 0 and as 1, carries, borrows and overflows both ways, the shift amounts,
// every compare true, false and on equal operands, extracts inside the operand, the load table's
// address lines, distinct register values), pins spot values, and prints each group's words, the
// load table's checksum and the sizes as one JSON line, which tests/test_selftest_scalar.py compares
// with the Python twin's.
#include <cstdio>
#include <set>
#include <string>
#include <vector>

#include "nanogpu/selftest_paths_host.h"
#include "nanogpu/selftest_scalar_host.h"

namespace ss = nanogpu::selftest::scalar;
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
  ss::HostOps o;
  uint32_t c = 9;
  // spot values, written out by hand
  CHECK(o.add_u32(0xffffffffu, 1u, c) == 0u && c == 1u);                       // carry out of bit 31
  CHECK(o.sub_u32(0u, 1u, c) == 0xffffffffu && c == 1u);                       // borrow
  CHECK(o.add64(0x00000000ffffffffull, 1ull, c) == 0x0000000100000000ull && c == 0u);   // the low carry enters the high word
  CHECK(o.sub64(0x0000000100000000ull, 1ull, c) == 0x00000000ffffffffull && c == 0u);
  CHECK(o.add_i32(0x7fffffffu, 1u, c) == 0x80000000u && c == 1u);              // signed overflow upward
  CHECK(o.sub_i32(0x80000000u, 1u, c) == 0x7fffffffu && c == 1u);              // and downward
  CHECK(o.min_i32(0xffffffffu, 1u, c) == 0xffffffffu && c == 1u && o.min_u32(0xffffffffu, 1u, c) == 1u && c == 0u);
  CHECK(o.absdiff_i32(3u, 0xfffffffbu, c) == 8u && c == 1u && o.abs_i32(0xfffffff9u, c) == 7u);
  CHECK(o.mul_hi_u32(0xffffffffu, 0xffffffffu) == 0xfffffffeu && o.mul_hi_i32(0xffffffffu, 0xffffffffu) == 0u);   // (-1)(-1) = 1
  CHECK(o.mul_hi_i32(0x80000000u, 2u) == 0xffffffffu);                         // -2^32: high word -1
  CHECK(o.lshl3_add_u32(0x1fffffffu, 8u, c) == 0u && c == 1u);                 // 2^32 - 8 + 8
  CHECK(o.ashr_i32(0x80000000u, 31, c) == 0xffffffffu && o.lshr_b32(0x80000000u, 31, c) == 1u && o.lshl_b32(1u, 31, c) == 0x80000000u);
  CHECK(o.ashr_i64(0x8000000000000000ull, 63, c) == ~0ull && o.lshl_b64(3ull, 63, c) == 0x8000000000000000ull);
  CHECK(o.bfm_b32(4, 8) == 0xf00u && o.bfm_b64(33, 4) == 0x1fffffffF0ull);
  CHECK(o.nand_b32(~0u, ~0u, c) == 0u && c == 0u && o.orn2_b32(0u, ~0u, c) == 0u && o.andn2_b32(0xffu, 0x0fu, c) == 0xf0u);
  CHECK(o.bfe_u32(0xabcd1234u, 4u | 8u << 16, c) == 0x23u && o.bfe_i32(0xabcd1234u, 16u | 4u << 16, c) == 0xfffffffdu);
  CHECK(o.bfe_i64(0x00000f0000000000ull, 40u | 4u << 16, c) == ~0ull && o.bfe_u64(0x00000f0000000000ull, 40u | 4u << 16, c) == 15ull);
  CHECK(o.brev_b32(1u) == 0x80000000u && o.brev_b64(2ull) == 0x4000000000000000ull);
  CHECK(o.bcnt0_i32_b32(0xfffffff0u, c) == 4u && o.bcnt1_i32_b64(0xf0000000f0ull, c) == 8u);
  CHECK(o.ff0_i32_b32(0x0000ffffu) == 16u && o.ff1_i32_b64(0x100000000ull) == 32u);
  CHECK(o.flbit_i32_b32(0x00ff0000u) == 8u && o.flbit_i32(0xff00ffffu) == 8u && o.flbit_i32(0x7fffffffu) == 1u);
  CHECK(o.flbit_i32_b64(1ull) == 63u && o.flbit_i32_i64(0xfffffffffffffffeull) == 63u);
  CHECK(o.bitset0_b32(0xffu, 3) == 0xf7u && o.bitset1_b32(0u, 31) == 0x80000000u);
  CHECK(o.sext_i32_i8(0x1280u) == 0xffffff80u && o.sext_i32_i16(0x12347fffu) == 0x7fffu);
  CHECK(o.pack_ll_b32_b16(0x11112222u, 0x33334444u) == 0x44442222u && o.pack_lh_b32_b16(0x11112222u, 0x33334444u) == 0x33332222u &&
        o.pack_hh_b32_b16(0x11112222u, 0x33334444u) == 0x33331111u);
  CHECK(o.sel_gt_i32(0xffffffffu, 1u, 7, 8) == 8u && o.sel_gt_u32(0xffffffffu, 1u, 7, 8) == 7u);
  CHECK(o.br_bitcmp0_b32(0x10u, 4u, 7, 8) == 8u && o.br_bitcmp1_b32(0x10u, 36u, 7, 8) == 7u);   // the bit number is S1[4:0]
  CHECK(o.sel_eq_u64(0x100000000ull, 0x200000000ull, 7, 8) == 8u);
  CHECK(o.c.abnormal == 0);
  CHECK(ss::fold(0u, 0u, 0u) == 0x9e3779b9u && ss::fold(1u, 0u, 1u) == 0x9e3779b9u + 129u);

  std::string json = "{\"groups\": {";
  std::vector<uint32_t> words(ss::kGroupWords);
  ss::Conds all;
  for (int g = 0; g < ss::kNumExact; ++g) {
    ss::Conds cd;
    ss::group_expected(g, words.data(), &cd);
    CHECK(cd.abnormal == 0);
    const uint32_t un = ss::uncovered_bits(words.data());
    if (un) {
      std::fprintf(stderr, "group %s: bits %#010x are the same in all %d words\n", ss::group_name(g), un, ss::kGroupWords);
      ++failures;
    }
    for (int id = 0; id < ss::kNumScc; ++id) all.scc[id][0] += cd.scc[id][0], all.scc[id][1] += cd.scc[id][1];
    if (g == ss::kAdd) {
      for (int t = 0; t < 2; ++t) CHECK(cd.carry31[t] > 0 && cd.carry63[t] > 0 && cd.borrow31[t] > 0 && cd.borrow63[t] > 0);
      CHECK(cd.overflow_pos > 0 && cd.overflow_neg > 0);
    }
    if (g == ss::kCmp) CHECK(cd.equal_operands > 0);
    json += std::string(g ? ", \"" : "\"") + ss::group_name(g) + "\": [";
    for (int i = 0; i < ss::kGroupWords; ++i) json += (i ? ", " : "") + std::to_string(words[i]);
    json += "]";
  }
  for (int id = 0; id < ss::kNumScc; ++id)
    if (!(all.scc[id][0] > 0 && all.scc[id][1] > 0)) {
      std::fprintf(stderr, "%s: SCC consumed %d times as 0 and %d times as 1\n", ss::scc_name(id), all.scc[id][0], all.scc[id][1]);
      ++failures;
    }
  // shift amounts 0, 1, 31 in 32 bits and 0, 31, 32, 63 in 64 bits
  std::set<uint32_t> n32, n64;
  for (int s = 0; s < ss::kWaveWords; ++s) n32.insert(ss::shift_amount32(s, 0x12345678u)), n64.insert(ss::shift_amount64(s, 0x12345678u));
  for (uint32_t n : {0u, 1u, 31u}) CHECK(n32.count(n));
  for (uint32_t n : {0u, 31u, 32u, 63u}) CHECK(n64.count(n));
  for (uint32_t u = 0; u < 0x10000u; ++u) {   // every extract has offset + width inside the operand, width >= 1
    const uint32_t f32 = ss::bfe_field32(u * 0x10001u), f64 = ss::bfe_field64(u * 0x10001u);
    CHECK((f32 >> 16) >= 1 && (f32 & 31u) + (f32 >> 16) <= 32u && (f64 >> 16) >= 1 && (f64 & 63u) + (f64 >> 16) <= 64u);
  }
  const std::vector<uint32_t> table = ss::expected_table();
  CHECK(static_cast<int>(table.size()) == ss::kTableWords && ss::kTableWords == 224);

  // smem: no two words at indices differing in one bit are equal
  const std::vector<uint32_t> smem = ss::smem_table();
  for (int i = 0; i < ss::kSmemWords; ++i)
    for (int b = 1; b < ss::kSmemWords; b <<= 1) CHECK(smem[i] != smem[i ^ b]);
  // sregs: the values of a wave and pass are pairwise distinct; pass 1 is the complement
  for (uint32_t wave = 0; wave < 4; ++wave)
    for (uint32_t pass = 0; pass < 2; ++pass) {
      std::set<uint32_t> seen;
      for (uint32_t i = 0; i < ss::kSregSlots; ++i) seen.insert(ss::sreg_word(i, 0x5eed5eedu ^ wave, pass));
      CHECK(static_cast<int>(seen.size()) == ss::kSregSlots);
    }
  CHECK(ss::sreg_word(3, 77, 1) == ~ss::sreg_word(3, 77, 0) && (ss::sreg_odd(87) & 1u) == 1u);
  CHECK(ss::kSregFirst + ss::kSregSlots == 100 && ss::kSregSlots <= 32 * ss::kSregFlags);

  const uint32_t rec[16] = {2, 0x0000a5b0u, 0x100, 0xf, 0, 17, 0, 0, 0xffffffffu, 0xffffffffu, 0xffffffffu,
                            0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
  const ss::ScalarRecord r0 = ss::decode_scalar_record(rec, 0), r1 = ss::decode_scalar_record(rec, 1);
  CHECK(nanogpu::selftest::record_written(rec) && !nanogpu::selftest::record_written(rec + ss::kScalarRecordWords));
  CHECK(r0.xcc == 2 && r0.bad_index == 17 && r0.bad_which == ss::kBadSregs && r1.fail == ss::kNoBad);
  CHECK(ss::pack_bad(ss::kBadSregs, 87, 3) < ss::pack_bad(ss::kBadSmem, 0, 0));

  char buf[160];
  std::snprintf(buf, sizeof buf, "}, \"smem_checksum\": %u, \"smem_words\": %d, \"sreg_slots\": %d, \"record_words\": %d}",
                sp::tile_checksum(smem.data(), ss::kSmemWords), ss::kSmemWords, ss::kSregSlots, ss::kScalarRecordWords);
  json += buf;
  if (failures) return 1;
  std::puts(json.c_str());
  return 0;
}
