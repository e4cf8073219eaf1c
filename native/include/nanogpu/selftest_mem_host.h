// Host/device-shared definitions of the deep self-test's memory part (native/hip/probe_mem.inc:
// cu_mem_kernel, mem_lanes_kernel). Plain C++ with no HIP dependency: the stand-alone program
// native/tests/selftest_mem_host_main.cpp builds it on its own, also under ASan + UBSan. The Python
// twin, in plain integers, is nanogpu/probe/selftest_mem.py.
//
// All four waves of a CU run every selected group. A group is a fixed list of memory instructions;
// each gives every lane some result words, numbered k = 0 .. group_words(g) - 1 in the order the
// lists below state. Every result word is compared in the kernel with the value this header
// computes for (wave, lane, k). The index of a result word in the records is k * 64 + lane, except
// in `l1`, where it is the index of the table word compared.
//
// The inputs: a read-only table of kTableWords words, word i = mix32(i ^ kSalt), and for every
// workgroup a slice of kSliceBytes of device scratch memory, of which wave w owns bytes
// [w * kWaveBytes, (w + 1) * kWaveBytes), and of the kernel's LDS array bytes
// [w * kLdsWaveBytes, (w + 1) * kLdsWaveBytes). No store and no atomic leaves the wave's region.
//
//   gload   global_load_{ubyte,sbyte} at byte 0..3, _{ushort,sshort} at byte 0 and 2, _ubyte_d16,
//           _ubyte_d16_hi, _sbyte_d16, _sbyte_d16_hi, _short_d16, _short_d16_hi (the half of the register the
//           instruction names is compared), _dword, _dwordx2, _dwordx3, _dwordx4, and _dwordx4 with nt, sc0, sc1 and
//           sc0 sc1: once with unit-stride lane addresses, once with every lane on another 128-byte line
//   l1      the whole table with global_load_dwordx4, twice, in two line orders
//   gstore  global_store_{byte,short,short_d16_hi,dword,dwordx2,dwordx3,dwordx4} over a background,
//           read back with global_load_dwordx4
//   buffer  buffer_load / buffer_store of 1, 2, 4, 8, 12 and 16 bytes through a raw descriptor (stride 0)
//           whose num_records ends inside the wave's region: with offen, with a non-zero soffset, and
//           with an immediate offset; lanes 0..31 in range, lanes 32..63 out of range
//   lds     ds_write_{b8,b16,b32,b64,b96,b128}, ds_write2_{b32,b64}, ds_write2st64_{b32,b64},
//           ds_read_{u8,i8,u16,i16,b32,b64,b96,b128}, ds_read2_{b32,b64}, ds_read2st64_{b32,b64}, each under
//           three lane maps: unit stride, a permutation, a half-wave on one bank
//   ldstr   ds_read_b64_tr_b16 of a 16 x 16 image of 16-bit elements, at two row strides
//   ldsdma  global_load_lds_{dword,dwordx4} and buffer_load_dword ... lds, read back with ds_read_b32
//   atomic  with return, on the slice (agent scope) and on LDS: add, sub, smin, umin, smax, umax, and, or, xor,
//           inc, dec, swap, cmpswap in 32 bits; add, umax, swap, cmpswap in 64 bits; and 64 lanes adding
//           one constant to one word
//
// Why these values are the one right answer: every instruction above moves bytes or applies integer
// arithmetic that the CDNA ISA defines in full for the operands used. Every access is naturally
// aligned (12-byte accesses to 16 bytes). What stays out, because its definition is not established
// here (the README lists it under "Not covered"): what a d16 load leaves in the other half of its register (with
// SRAM ECC the hardware may write the whole register), sub-dword and 12-byte LDS-DMA (where a lane's 12 bytes
// land), the _tr_b8 / _tr_b4 / _tr_b6
// reads, partly out-of-range multi-dword buffer accesses, whether soffset takes part in the range
// check (a lane is in range only if it is so with soffset counted, out of range only if it is so
// without), strided or swizzled descriptors and typed formats, float and packed atomics,
// misaligned accesses, flat_ and scratch_ instructions.
#pragma once

#include <cstdint>
#include <vector>

#include "nanogpu/selftest_host.h"

namespace nanogpu {
namespace selftest {
namespace mem {

constexpr int kWaves = 4;
constexpr int kLanes = 64;
constexpr int kTableWords = 8192;               // 32 KiB: the size of a CU's L1
constexpr uint32_t kTableBytes = kTableWords * 4;
constexpr uint32_t kSalt = 0x3e3d7a11u;
constexpr uint32_t kSliceBytes = 8192;          // of device scratch memory, a workgroup
constexpr uint32_t kWaveBytes = kSliceBytes / kWaves;
constexpr uint32_t kLdsWaveBytes = 16384;       // of the kernel's LDS array, a wave
constexpr uint32_t kLdsArrayBytes = 86016;      // the kernel's static LDS array: more than half of a CU's 160 KiB
static_assert(kWaves * kLdsWaveBytes + 16 <= kLdsArrayBytes, "the waves' regions and the reduction words fit the array");
constexpr uint32_t kNoBad = 0xffffffffu;

// The order is the bit order of the records.
enum Group : int { kGload = 0, kL1, kGstore, kBuffer, kLds, kLdstr, kLdsdma, kAtomic, kNumNames };
constexpr uint32_t kAllGroups = (1u << kNumNames) - 1;

inline const char* group_name(int g) {
  static const char* const names[kNumNames] = {"gload", "l1", "gstore", "buffer", "lds", "ldstr", "ldsdma", "atomic"};
  return g >= 0 && g < kNumNames ? names[g] : "?";
}

NANOGPU_HD inline uint32_t table_word(uint32_t i) { return mix32(i ^ kSalt); }
// Byte b of a little-endian word.
NANOGPU_HD inline uint32_t byte_of(uint32_t w, uint32_t b) { return (w >> (8 * b)) & 0xffu; }
NANOGPU_HD inline uint32_t table_byte(uint32_t a) { return byte_of(table_word(a >> 2), a & 3u); }
NANOGPU_HD inline uint32_t sext8(uint32_t v) { return (v & 0x80u) ? v | 0xffffff00u : v & 0xffu; }
NANOGPU_HD inline uint32_t sext16(uint32_t v) { return (v & 0x8000u) ? v | 0xffff0000u : v & 0xffffu; }
NANOGPU_HD inline uint32_t val(uint32_t tag, uint32_t wave, uint32_t lane, uint32_t a, uint32_t b) {
  return mix32(tag ^ (wave << 28) ^ (lane << 20) ^ (a << 8) ^ b);
}

// A word of a 16-byte chunk after `n` bytes were stored at byte `sub` of the chunk over the background word `bg`:
// word j of the chunk. `src(i)` is register i of the store's data, little-endian.
template <class Src>
NANOGPU_HD inline uint32_t overlay(uint32_t bg, int j, int sub, int n, Src&& src) {
  uint32_t out = 0;
  for (int b = 0; b < 4; ++b) {
    const int pos = 4 * j + b - sub;
    const uint32_t byte = pos >= 0 && pos < n ? byte_of(src(pos >> 2), static_cast<uint32_t>(pos & 3)) : byte_of(bg, static_cast<uint32_t>(b));
    out |= byte << (8 * b);
  }
  return out;
}

// ---- gload ------------------------------------------------------------------------------
constexpr int kGloadForms = 26, kGloadMaps = 2, kGloadMapWords = 44;
constexpr uint32_t kD16Init = 0xa5a55a5au;
enum GloadKind : int { kUbyte, kSbyte, kUshort, kSshort, kUbyteD16, kUbyteD16Hi, kSbyteD16, kSbyteD16Hi, kShortD16, kShortD16Hi, kDwords };

NANOGPU_HD constexpr int gload_kind(int f) {
  return f < 4 ? kUbyte : f < 8 ? kSbyte : f < 10 ? kUshort : f < 12 ? kSshort : f < 18 ? kUbyteD16 + (f - 12) : kDwords;
}
NANOGPU_HD constexpr int gload_sub(int f) {   // the byte inside the lane's chunk
  return f < 8 ? (f & 3) : f < 12 ? 2 * (f & 1) : f == 12 ? 1 : f == 13 ? 2 : f == 14 ? 3 : f == 16 ? 2 : 0;
}
NANOGPU_HD constexpr int gload_words(int f) { return f < 19 ? 1 : f == 19 ? 2 : f == 20 ? 3 : 4; }
NANOGPU_HD constexpr int gload_first(int f) { return f < 19 ? f : f == 19 ? 19 : f == 20 ? 21 : 24 + 4 * (f - 21); }
// The 16-byte chunk of the table lane `lane` reads form f from: map 0 is unit stride, map 1 puts every lane on
// another 128-byte line.
NANOGPU_HD inline uint32_t gload_chunk(int map, int wave, int lane, int f) {
  return map == 0 ? 16u * static_cast<uint32_t>((wave * 64 + lane + 61 * f) & 2047)
                  : 128u * static_cast<uint32_t>((lane * 5 + wave * 64 + 3 * f) & 255) + 16u * static_cast<uint32_t>((lane + f) & 7);
}
NANOGPU_HD inline uint32_t gload_addr(int map, int wave, int lane, int f) { return gload_chunk(map, wave, lane, f) + gload_sub(f); }
NANOGPU_HD inline uint32_t gload_expected(int map, int wave, int lane, int f, int j) {
  const uint32_t a = gload_addr(map, wave, lane, f);
  const uint32_t b = table_byte(a), h = b | (table_byte(a + 1) << 8);
  switch (gload_kind(f)) {
    case kUbyte: return b;
    case kSbyte: return sext8(b);
    case kUshort: return h;
    case kSshort: return sext16(h);
    case kUbyteD16: case kUbyteD16Hi: return b;                       // the 16 bits written: gload_d16_half of the register
    case kSbyteD16: case kSbyteD16Hi: return sext8(b) & 0xffffu;
    case kShortD16: case kShortD16Hi: return h;
    default: return table_word((a >> 2) + static_cast<uint32_t>(j));
  }
}
// The half of the register a d16 form writes, as a 16-bit value; the other half is not compared.
NANOGPU_HD inline uint32_t gload_d16_half(uint32_t reg, bool hi) { return hi ? reg >> 16 : reg & 0xffffu; }
NANOGPU_HD constexpr int gload_k(int map, int f, int j) { return map * kGloadMapWords + gload_first(f) + j; }

// ---- l1 ---------------------------------------------------------------------------------
constexpr int kL1Passes = 2, kL1Steps = kTableWords / (4 * kLanes);   // 32 steps of 64 x 16 bytes a pass
NANOGPU_HD inline uint32_t l1_chunk(int pass, int step, int lane) {   // the 16-byte chunk of the table
  return pass == 0 ? static_cast<uint32_t>(step * 64 + lane)
                   : static_cast<uint32_t>((kL1Steps - 1 - step) * 64 + ((lane * 17 + step) & 63));
}
NANOGPU_HD constexpr int l1_k(int pass, int step, int j) { return (pass * kL1Steps + step) * 4 + j; }

// ---- gstore -----------------------------------------------------------------------------
constexpr int kGstoreForms = 7;   // byte, short, short_d16_hi, dword, dwordx2, dwordx3, dwordx4
constexpr uint32_t kTagGstore = 0x57012e00u, kTagGstoreBg = 0x0b6b6000u;
NANOGPU_HD inline int gstore_bytes(int f) { return f == 0 ? 1 : f < 3 ? 2 : f == 3 ? 4 : f == 4 ? 8 : f == 5 ? 12 : 16; }
NANOGPU_HD inline uint32_t gstore_chunk(int wave, int lane, int f) { return 16u * static_cast<uint32_t>((lane * 13 + f * 7 + wave) & 63); }
NANOGPU_HD inline int gstore_sub(int lane, int f) {
  return f == 0 ? (lane + 5) & 15 : f == 1 ? 2 * (lane & 7) : f == 2 ? 2 * ((lane + 3) & 7) : f == 3 ? 4 * (lane & 3) : f == 4 ? 8 * (lane & 1) : 0;
}
// Word `word` (of the wave's region) of the background before form f's stores.
NANOGPU_HD inline uint32_t gstore_bg(int wave, int f, uint32_t word) { return val(kTagGstoreBg, wave, 0, f, word); }
// Register j a lane stores in form f (short_d16_hi stores bits 31:16 of register 0).
NANOGPU_HD inline uint32_t gstore_val(int wave, int lane, int f, int j) { return val(kTagGstore, wave, lane, f, j); }
NANOGPU_HD inline uint32_t gstore_expected(int wave, int lane, int f, int j) {   // word j of the lane's own chunk
  return overlay(gstore_bg(wave, f, gstore_chunk(wave, lane, f) / 4 + j), j, gstore_sub(lane, f), gstore_bytes(f),
                 [=](int i) { return gstore_val(wave, lane, f, i) >> (f == 2 ? 16 : 0); });
}
NANOGPU_HD constexpr int gstore_k(int f, int j) { return 4 * f + j; }

// ---- buffer -----------------------------------------------------------------------------
// The descriptor's base is the wave's region and its num_records kBufRecords. Width w (0..5: 1, 2, 4, 8, 12, 16
// bytes; lane stride 1, 2, 4, 8, 16, 16) and mode m (0 offen, 1 soffset kBufSoffset, 2 immediate kBufImm). Lanes
// 0..31 end exactly at num_records; lanes 32..63 begin exactly at it (with soffset: their voffset alone does).
constexpr int kBufWidths = 6, kBufModes = 3;
constexpr uint32_t kBufRecords = 1024, kBufSoffset = 64, kBufImm = 48;
constexpr uint32_t kTagBuf = 0x2bf00d00u, kTagBufBg = 0x6a09e600u;
NANOGPU_HD constexpr int buf_bytes(int w) { return w == 0 ? 1 : w == 1 ? 2 : w == 2 ? 4 : w == 3 ? 8 : w == 4 ? 12 : 16; }
NANOGPU_HD constexpr int buf_stride(int w) { return w == 4 ? 16 : buf_bytes(w); }
NANOGPU_HD constexpr int buf_words(int w) { return w < 3 ? 1 : w - 1; }
NANOGPU_HD constexpr int buf_load_first(int w) { return w < 3 ? w : w == 3 ? 3 : w == 4 ? 5 : 8; }   // 12 words a mode
NANOGPU_HD inline bool buf_in_range(int lane) { return lane < 32; }
// The byte of the wave's region the lane's access begins at, and the voffset register that gives it.
NANOGPU_HD inline uint32_t buf_addr(int w, int m, int lane) {
  const uint32_t s = static_cast<uint32_t>(buf_stride(w));
  return kBufRecords - 32u * s + static_cast<uint32_t>(lane) * s + (m == 1 && !buf_in_range(lane) ? kBufSoffset : 0u);
}
NANOGPU_HD inline uint32_t buf_voffset(int w, int m, int lane) { return buf_addr(w, m, lane) - (m == 1 ? kBufSoffset : m == 2 ? kBufImm : 0u); }
// `phase` 0 is the background the loads read; 1 + 3 w + m the one form (w, m)'s stores overlay.
NANOGPU_HD inline uint32_t buf_bg(int wave, int phase, uint32_t word) { return val(kTagBufBg, wave, 0, phase, word); }
NANOGPU_HD inline uint32_t buf_val(int wave, int lane, int w, int m, int j) { return val(kTagBuf, wave, lane, 3 * w + m, j); }
NANOGPU_HD inline uint32_t buf_load_expected(int wave, int lane, int w, int m, int j) {
  if (!buf_in_range(lane)) return 0u;
  const uint32_t a = buf_addr(w, m, lane);
  const uint32_t word = buf_bg(wave, 0, a / 4 + static_cast<uint32_t>(j));
  return w == 0 ? byte_of(word, a & 3u) : w == 1 ? (word >> (8 * (a & 2u))) & 0xffffu : word;
}
// Byte `at` of the wave's region after form (w, m)'s stores: the in-range lanes tile [num_records - 32 stride, num_records).
NANOGPU_HD inline uint32_t buf_store_byte(int wave, int w, int m, uint32_t at) {
  const uint32_t s = static_cast<uint32_t>(buf_stride(w)), first = kBufRecords - 32u * s;
  if (at >= first && at < kBufRecords) {
    const uint32_t lane = (at - first) / s, pos = (at - first) % s;
    if (pos < static_cast<uint32_t>(buf_bytes(w))) return byte_of(buf_val(wave, static_cast<int>(lane), w, m, static_cast<int>(pos >> 2)), pos & 3u);
  }
  return byte_of(buf_bg(wave, 1 + 3 * w + m, at >> 2), at & 3u);
}
// Word j of the 16-byte chunk that holds the lane's address, after the stores.
NANOGPU_HD inline uint32_t buf_store_expected(int wave, int lane, int w, int m, int j) {
  const uint32_t at = (buf_addr(w, m, lane) & ~15u) + 4u * static_cast<uint32_t>(j);
  uint32_t out = 0;
  for (uint32_t b = 0; b < 4; ++b) out |= buf_store_byte(wave, w, m, at + b) << (8 * b);
  return out;
}
constexpr int kBufLoadWords = 12 * kBufModes;
NANOGPU_HD constexpr int buf_load_k(int w, int m, int j) { return 12 * m + buf_load_first(w) + j; }
NANOGPU_HD constexpr int buf_store_k(int w, int m, int j) { return kBufLoadWords + 4 * (3 * w + m) + j; }

// ---- lds --------------------------------------------------------------------------------
constexpr int kLdsMaps = 3, kLdsReadForms = 12, kLdsWriteForms = 10;
constexpr uint32_t kLdsUpper = 4096;   // the second address of the st64 forms: offset1 16 (b32) or 8 (b64)
constexpr uint32_t kTagLds = 0x1d5b6000u, kTagLdsBg = 0x4c1d5000u;
// The lane's 16-byte chunk of the wave's region: unit stride; a permutation; a half-wave on one bank (128-byte stride).
NANOGPU_HD inline uint32_t lds_chunk(int map, int lane) {
  return map == 0 ? 16u * static_cast<uint32_t>(lane) : map == 1 ? 16u * static_cast<uint32_t>((lane * 13 + 5) & 63)
                                                                   : 128u * static_cast<uint32_t>(lane & 31) + 16u * static_cast<uint32_t>(lane >> 5);
}
NANOGPU_HD inline uint32_t lds_bg(int wave, int phase, uint32_t word) { return val(kTagLdsBg, wave, 0, phase, word); }
NANOGPU_HD inline uint32_t lds_val(int wave, int lane, int map, int f, int j) { return val(kTagLds, wave, lane, 16 * map + f, j); }
// read forms: 0 u8, 1 i8, 2 u16, 3 i16, 4 b32, 5 b64, 6 b96, 7 b128, 8 read2_b32 (dwords 0 and 2), 9 read2_b64 (qwords 0, 1),
// 10 read2st64_b32 (dword 0 here and kLdsUpper on), 11 read2st64_b64 (qword 0 here and kLdsUpper on); the background is phase 0
NANOGPU_HD constexpr int lds_read_words(int f) { return f < 5 ? 1 : f == 5 ? 2 : f == 6 ? 3 : f == 7 ? 4 : f == 8 ? 2 : f == 9 ? 4 : f == 10 ? 2 : 4; }
NANOGPU_HD inline int lds_read_first(int f) {
  int k = 0;
  for (int i = 0; i < f; ++i) k += lds_read_words(i);
  return k;
}
constexpr int kLdsReadMapWords = 26;
NANOGPU_HD inline int lds_read_sub(int lane, int f) {
  return f == 0 ? (lane + 1) & 15 : f == 1 ? (lane * 3) & 15 : f == 2 ? 2 * (lane & 7) : f == 3 ? 2 * ((lane + 5) & 7) : f == 4 ? 4 * (lane & 3) : f == 5 ? 8 * (lane & 1) : 0;
}
NANOGPU_HD inline uint32_t lds_read_expected(int wave, int lane, int map, int f, int j) {
  const uint32_t c = lds_chunk(map, lane), a = c + static_cast<uint32_t>(lds_read_sub(lane, f));
  const uint32_t w = lds_bg(wave, 0, a / 4);
  switch (f) {
    case 0: return byte_of(w, a & 3u);
    case 1: return sext8(byte_of(w, a & 3u));
    case 2: return (w >> (8 * (a & 2u))) & 0xffffu;
    case 3: return sext16((w >> (8 * (a & 2u))) & 0xffffu);
    case 8: return lds_bg(wave, 0, c / 4 + 2u * static_cast<uint32_t>(j));
    case 10: return lds_bg(wave, 0, (c + kLdsUpper * static_cast<uint32_t>(j)) / 4);
    case 11: return lds_bg(wave, 0, (c + kLdsUpper * static_cast<uint32_t>(j >> 1)) / 4 + static_cast<uint32_t>(j & 1));
    default: return lds_bg(wave, 0, a / 4 + static_cast<uint32_t>(j));
  }
}
NANOGPU_HD inline int lds_read_k(int map, int f, int j) { return map * kLdsReadMapWords + lds_read_first(f) + j; }
// write forms: 0 b8, 1 b16, 2 b32, 3 b64, 4 b96, 5 b128, 6 write2_b32 (dwords 0 and 2), 7 write2_b64 (qwords 0, 1),
// 8 write2st64_b32 (dword 0 here and kLdsUpper on), 9 write2st64_b64 (qword 0 here and kLdsUpper on). The lane's chunk and
// the one kLdsUpper on hold background phase 1 + 10 map + f; 4 words are read back, 8 (both chunks) of the st64 forms.
NANOGPU_HD constexpr int lds_write_words(int f) { return f < 8 ? 4 : 8; }
constexpr int kLdsWriteMapWords = 48;
NANOGPU_HD inline int lds_write_sub(int lane, int f) {
  return f == 0 ? (lane + 7) & 15 : f == 1 ? 2 * ((lane + 1) & 7) : f == 2 ? 4 * ((lane + 2) & 3) : f == 3 ? 8 * ((lane >> 1) & 1) : 0;
}
NANOGPU_HD inline int lds_write_bytes(int f) { return f == 0 ? 1 : f == 1 ? 2 : f == 2 ? 4 : f == 3 ? 8 : f == 4 ? 12 : 16; }
NANOGPU_HD inline uint32_t lds_write_expected(int wave, int lane, int map, int f, int j) {
  const int phase = 1 + 10 * map + f, upper = j >> 2, jj = j & 3;
  const uint32_t bg = lds_bg(wave, phase, (lds_chunk(map, lane) + kLdsUpper * static_cast<uint32_t>(upper)) / 4 + static_cast<uint32_t>(jj));
  auto src = [=](int i) { return lds_val(wave, lane, map, f, i); };
  if (f < 6) return overlay(bg, jj, lds_write_sub(lane, f), lds_write_bytes(f), src);
  if (f == 6) return jj == 0 ? src(0) : jj == 2 ? src(1) : bg;       // data0 at dword 0, data1 at dword 2
  if (f == 7) return src(jj);                                           // data0 = registers 0, 1 at qword 0, data1 = 2, 3 at qword 1
  if (f == 8) return jj == 0 ? src(upper) : bg;                        // data0 here, data1 in the upper chunk
  return jj < 2 ? src(2 * upper + jj) : bg;
}
constexpr int kLdsReadWords = kLdsMaps * kLdsReadMapWords;
NANOGPU_HD inline int lds_write_k(int map, int f, int j) { return kLdsReadWords + map * kLdsWriteMapWords + (f < 8 ? 4 * f : 32 + 8 * (f - 8)) + j; }

// ---- ldstr ------------------------------------------------------------------------------
// Step s: a 16 x 16 image of 16-bit elements with rows of 32 + 16 s bytes. Lane 4q + p of 16-lane group g writes
// (ds_write_b64) and then addresses row 4g + q, columns 4p .. 4p + 3; lane i of the group receives column i of rows
// 4g .. 4g + 3, row 4g + q in element q.
constexpr int kLdstrSteps = 2;
constexpr uint32_t kTagLdstr = 0x7b160000u;
NANOGPU_HD inline uint32_t ldstr_stride(int s) { return 32u + 16u * static_cast<uint32_t>(s); }
NANOGPU_HD inline uint32_t ldstr_elem(int wave, int s, int row, int col) { return val(kTagLdstr, wave, 0, 16 * s + row, col) & 0xffffu; }
NANOGPU_HD inline uint32_t ldstr_addr(int s, int lane) {
  return static_cast<uint32_t>(4 * (lane >> 4) + ((lane >> 2) & 3)) * ldstr_stride(s) + 8u * static_cast<uint32_t>(lane & 3);
}
NANOGPU_HD inline uint32_t ldstr_written(int wave, int s, int lane, int j) {   // register j of the lane's ds_write_b64
  const int row = 4 * (lane >> 4) + ((lane >> 2) & 3), col = 4 * (lane & 3) + 2 * j;
  return ldstr_elem(wave, s, row, col) | (ldstr_elem(wave, s, row, col + 1) << 16);
}
NANOGPU_HD inline uint32_t ldstr_expected(int wave, int s, int lane, int j) {
  const int row = 4 * (lane >> 4) + 2 * j, col = lane & 15;
  return ldstr_elem(wave, s, row, col) | (ldstr_elem(wave, s, row + 1, col) << 16);
}
NANOGPU_HD constexpr int ldstr_k(int s, int j) { return 2 * s + j; }

// ---- ldsdma -----------------------------------------------------------------------------
// Form f: 0 global_load_lds_dword, 1 _dwordx4, 2 buffer_load_dword ... lds. The lane's source is a
// 16-byte chunk of the table (permuted); the destination is the wave's region + dma_dst(f) + lane * size.
constexpr int kDmaForms = 3;
NANOGPU_HD constexpr int dma_bytes(int f) { return f == 1 ? 16 : 4; }
NANOGPU_HD inline uint32_t dma_dst(int f) { return 1024u * static_cast<uint32_t>(f); }
NANOGPU_HD inline uint32_t dma_src(int wave, int lane, int f) { return 16u * static_cast<uint32_t>((lane * 29 + wave * 512 + f * 64 + 3) & 2047); }
NANOGPU_HD constexpr int dma_first(int f) { return f == 0 ? 0 : f == 1 ? 1 : 5; }
NANOGPU_HD inline uint32_t dma_expected(int wave, int lane, int f, int j) { return table_word(dma_src(wave, lane, f) / 4 + static_cast<uint32_t>(j)); }
NANOGPU_HD constexpr int dma_k(int f, int j) { return dma_first(f) + j; }
constexpr uint32_t kDmaBg = 0xdeadd0d0u;   // what the destinations hold before

// ---- atomic -----------------------------------------------------------------------------
// Memory m: 0 the slice (agent scope), 1 LDS. Lane l's word (pair of words) is at byte 8 l of the wave's region; the
// contended word at byte kAtomContended. Per operation the lane's location first holds a, the instruction's operand is
// v (cmpswap: compare c, new v); the results are the value returned (a) and the value held after.
enum AtomOp : int { kAdd, kSub, kSmin, kUmin, kSmax, kUmax, kAnd, kOr, kXor, kInc, kDec, kSwap, kCmpswap, kNumOps32,
                    kAdd64 = kNumOps32, kUmax64, kSwap64, kCmpswap64, kNumOps };
constexpr uint32_t kTagAtom = 0x00a70300u, kAtomContended = 1024;
constexpr int kAtomMemWords = 2 * kNumOps32 + 4 * (kNumOps - kNumOps32) + 4;   // 46
NANOGPU_HD inline uint64_t atom_raw(int m, int wave, int lane, int op, int which) {
  const uint32_t lo = val(kTagAtom, wave, lane, 64 * m + op, 4 * which), hi = val(kTagAtom, wave, lane, 64 * m + op, 4 * which + 1);
  return op < kNumOps32 ? lo : (static_cast<uint64_t>(hi) << 32) | lo;
}
NANOGPU_HD inline uint64_t atom_v(int m, int wave, int lane, int op) {
  const uint64_t v = atom_raw(m, wave, lane, op, 1);
  return op == kInc || op == kDec ? (v & 0x7fffffffu) | 2u : v;        // 2 <= v < 2^31: v + 1 and v >> 1 are what they seem
}
NANOGPU_HD inline uint64_t atom_a(int m, int wave, int lane, int op) {
  const uint64_t v = atom_v(m, wave, lane, op);
  if (op == kInc) return (lane & 1) ? v >> 1 : v;                      // even lanes wrap to 0
  if (op == kDec) return (lane & 3) == 0 ? 0u : (lane & 3) == 1 ? v + 1 : v >> 1;   // 0 and values above v wrap to v
  return atom_raw(m, wave, lane, op, 0);
}
NANOGPU_HD inline uint64_t atom_cmp(int m, int wave, int lane, int op) {   // even lanes succeed
  return atom_a(m, wave, lane, op) ^ ((lane & 1) ? 0x10u : 0u);
}
NANOGPU_HD inline uint64_t atom_after(int m, int wave, int lane, int op) {
  const uint64_t a = atom_a(m, wave, lane, op), v = atom_v(m, wave, lane, op);
  const uint32_t a32 = static_cast<uint32_t>(a), v32 = static_cast<uint32_t>(v);
  switch (op) {
    case kAdd: return a32 + v32;
    case kSub: return a32 - v32;
    case kSmin: return static_cast<int32_t>(a32) < static_cast<int32_t>(v32) ? a32 : v32;
    case kUmin: return a32 < v32 ? a32 : v32;
    case kSmax: return static_cast<int32_t>(a32) > static_cast<int32_t>(v32) ? a32 : v32;
    case kUmax: return a32 > v32 ? a32 : v32;
    case kAnd: return a32 & v32;
    case kOr: return a32 | v32;
    case kXor: return a32 ^ v32;
    case kInc: return a32 >= v32 ? 0u : a32 + 1u;
    case kDec: return a32 == 0u || a32 > v32 ? v32 : a32 - 1u;
    case kSwap: case kSwap64: return v;
    case kCmpswap: case kCmpswap64: return atom_cmp(m, wave, lane, op) == a ? v : a;
    case kAdd64: return a + v;
    default: return a > v ? a : v;   // kUmax64
  }
}
NANOGPU_HD constexpr int atom_first(int op) { return op < kNumOps32 ? 2 * op : 2 * kNumOps32 + 4 * (op - kNumOps32); }
// j: the returned value's words, then the words held after.
NANOGPU_HD inline uint32_t atom_expected(int m, int wave, int lane, int op, int j) {
  const int n = op < kNumOps32 ? 1 : 2;
  const uint64_t x = j < n ? atom_a(m, wave, lane, op) : atom_after(m, wave, lane, op);
  return static_cast<uint32_t>(x >> (32 * (j % n)));
}
NANOGPU_HD constexpr int atom_k(int m, int op, int j) { return m * kAtomMemWords + atom_first(op) + j; }
// The contended word begins as b and every lane adds c: both below 2^24, so nothing wraps. Result words: 1 when the
// lane's returned value is b + q c with q < 64; the OR over the lanes of 1 << q, low and high word; the value after.
NANOGPU_HD inline uint32_t atom_cont_b(int m, int wave) { return val(kTagAtom, wave, 0, 64 * m + 32, 0) & 0xffffffu; }
NANOGPU_HD inline uint32_t atom_cont_c(int m, int wave) { return (val(kTagAtom, wave, 0, 64 * m + 32, 1) & 0xffffffu) | 1u; }
NANOGPU_HD inline uint32_t atom_cont_q(int m, int wave, uint32_t returned) {   // kNoBad: no such q
  const uint32_t d = returned - atom_cont_b(m, wave), c = atom_cont_c(m, wave);
  return returned >= atom_cont_b(m, wave) && d % c == 0 && d / c < 64u ? d / c : kNoBad;
}
NANOGPU_HD inline uint32_t atom_cont_expected(int m, int wave, int j) {
  return j == 0 ? 1u : j < 3 ? 0xffffffffu : atom_cont_b(m, wave) + 64u * atom_cont_c(m, wave);
}
NANOGPU_HD constexpr int atom_cont_k(int m, int j) { return m * kAtomMemWords + kAtomMemWords - 4 + j; }

// ---- the groups' result words -----------------------------------------------------------
NANOGPU_HD constexpr int group_words(int g) {
  return g == kGload    ? kGloadMaps * kGloadMapWords
         : g == kL1     ? kL1Passes * kL1Steps * 4
         : g == kGstore ? 4 * kGstoreForms
         : g == kBuffer ? kBufLoadWords + 4 * kBufWidths * kBufModes
         : g == kLds    ? kLdsReadWords + kLdsMaps * kLdsWriteMapWords
         : g == kLdstr  ? 2 * kLdstrSteps
         : g == kLdsdma ? 6
                        : 2 * kAtomMemWords;
}
// The size of the space the record's index is in.
NANOGPU_HD constexpr int group_indices(int g) { return g == kL1 ? kTableWords : group_words(g) * kLanes; }
constexpr int kMaxGroupWords = 256;
// Groups whose compared values come from the table: corrupt_expected takes them.
constexpr uint32_t kTableGroups = 1u << kGload | 1u << kL1 | 1u << kLdsdma;

// f(k, index, expected) for every result word of (g, wave, lane), in no particular order.
template <class F>
inline void for_each_result(int g, int wave, int lane, F&& f) {
  auto put = [&](int k, uint32_t v) { f(k, static_cast<uint32_t>(k * kLanes + lane), v); };
  switch (g) {
    case kGload:
      for (int m = 0; m < kGloadMaps; ++m)
        for (int fo = 0; fo < kGloadForms; ++fo)
          for (int j = 0; j < gload_words(fo); ++j) put(gload_k(m, fo, j), gload_expected(m, wave, lane, fo, j));
      break;
    case kL1:
      for (int p = 0; p < kL1Passes; ++p)
        for (int s = 0; s < kL1Steps; ++s)
          for (int j = 0; j < 4; ++j) {
            const uint32_t word = 4 * l1_chunk(p, s, lane) + static_cast<uint32_t>(j);
            f(l1_k(p, s, j), word, table_word(word));
          }
      break;
    case kGstore:
      for (int fo = 0; fo < kGstoreForms; ++fo)
        for (int j = 0; j < 4; ++j) put(gstore_k(fo, j), gstore_expected(wave, lane, fo, j));
      break;
    case kBuffer:
      for (int w = 0; w < kBufWidths; ++w)
        for (int m = 0; m < kBufModes; ++m) {
          for (int j = 0; j < buf_words(w); ++j) put(buf_load_k(w, m, j), buf_load_expected(wave, lane, w, m, j));
          for (int j = 0; j < 4; ++j) put(buf_store_k(w, m, j), buf_store_expected(wave, lane, w, m, j));
        }
      break;
    case kLds:
      for (int m = 0; m < kLdsMaps; ++m) {
        for (int fo = 0; fo < kLdsReadForms; ++fo)
          for (int j = 0; j < lds_read_words(fo); ++j) put(lds_read_k(m, fo, j), lds_read_expected(wave, lane, m, fo, j));
        for (int fo = 0; fo < kLdsWriteForms; ++fo)
          for (int j = 0; j < lds_write_words(fo); ++j) put(lds_write_k(m, fo, j), lds_write_expected(wave, lane, m, fo, j));
      }
      break;
    case kLdstr:
      for (int s = 0; s < kLdstrSteps; ++s)
        for (int j = 0; j < 2; ++j) put(ldstr_k(s, j), ldstr_expected(wave, s, lane, j));
      break;
    case kLdsdma:
      for (int fo = 0; fo < kDmaForms; ++fo)
        for (int j = 0; j < dma_bytes(fo) / 4; ++j) put(dma_k(fo, j), dma_expected(wave, lane, fo, j));
      break;
    default:
      for (int m = 0; m < 2; ++m) {
        for (int op = 0; op < kNumOps; ++op)
          for (int j = 0; j < (op < kNumOps32 ? 2 : 4); ++j) put(atom_k(m, op, j), atom_expected(m, wave, lane, op, j));
        for (int j = 0; j < 4; ++j) put(atom_cont_k(m, j), atom_cont_expected(m, wave, j));
      }
  }
}

// Group g's result words as mem_lanes returns them: [wave][k][lane].
inline std::vector<uint32_t> group_expected(int g) {
  std::vector<uint32_t> out(static_cast<size_t>(kWaves) * group_words(g) * kLanes, 0u);
  for (int wave = 0; wave < kWaves; ++wave)
    for (int lane = 0; lane < kLanes; ++lane)
      for_each_result(g, wave, lane, [&](int k, uint32_t, uint32_t v) {
        out[(static_cast<size_t>(wave) * group_words(g) + k) * kLanes + lane] = v;
      });
  return out;
}

// ---- every access, for the host's checks ------------------------------------------------
enum Space : int { kTable, kSlice, kLdsSpace };
struct Access {
  int space;        // kTable: bytes of the table; kSlice, kLdsSpace: bytes of the wave's region
  uint32_t at, bytes, align;
  bool store;
};

// f(Access) for every access of (g, wave, lane) whose address the header's maps give.
template <class F>
inline void for_each_access(int g, int wave, int lane, F&& f) {
  const uint32_t l = static_cast<uint32_t>(lane);
  switch (g) {
    case kGload:
      for (int m = 0; m < kGloadMaps; ++m)
        for (int fo = 0; fo < kGloadForms; ++fo) {
          const int kind = gload_kind(fo);
          const uint32_t n = kind == kDwords ? 4u * gload_words(fo) : kind == kUbyte || kind == kSbyte || (kind >= kUbyteD16 && kind <= kSbyteD16Hi) ? 1u : 2u;
          f(Access{kTable, gload_addr(m, wave, lane, fo), n, n == 12 ? 16u : n, false});
        }
      break;
    case kL1:
      for (int p = 0; p < kL1Passes; ++p)
        for (int s = 0; s < kL1Steps; ++s) f(Access{kTable, 16u * l1_chunk(p, s, lane), 16, 16, false});
      break;
    case kGstore:
      for (int fo = 0; fo < kGstoreForms; ++fo) {
        const uint32_t n = static_cast<uint32_t>(gstore_bytes(fo));
        f(Access{kSlice, 16u * l, 16, 16, true});                                   // the background
        f(Access{kSlice, gstore_chunk(wave, lane, fo) + static_cast<uint32_t>(gstore_sub(lane, fo)), n, n == 12 ? 16u : n, true});
        f(Access{kSlice, gstore_chunk(wave, lane, fo), 16, 16, false});
      }
      break;
    case kBuffer:
      for (uint32_t i = 0; i < kWaveBytes / (16 * kLanes); ++i) f(Access{kSlice, 16u * (l + 64u * i), 16, 16, true});   // the background
      for (int w = 0; w < kBufWidths; ++w)
        for (int m = 0; m < kBufModes; ++m) {
          const uint32_t n = static_cast<uint32_t>(buf_bytes(w));
          f(Access{kSlice, buf_addr(w, m, lane), n, n == 12 ? 16u : n, true});       // where it would land were the range not checked
          f(Access{kSlice, buf_addr(w, m, lane) & ~15u, 16, 16, false});
        }
      break;
    case kLds:
      for (int m = 0; m < kLdsMaps; ++m) {
        const uint32_t c = lds_chunk(m, lane);
        for (uint32_t up = 0; up < 2; ++up) f(Access{kLdsSpace, c + up * kLdsUpper, 16, 16, true});   // the background, the read back
        for (int fo = 0; fo < 8; ++fo) {                                           // the one-address reads
          const uint32_t n = fo < 2 ? 1u : fo < 4 ? 2u : fo == 4 ? 4u : fo == 5 ? 8u : fo == 6 ? 12u : 16u;
          f(Access{kLdsSpace, c + static_cast<uint32_t>(lds_read_sub(lane, fo)), n, n == 12 ? 16u : n, false});
        }
        for (int fo = 0; fo < 6; ++fo) {                                           // the one-address writes
          const uint32_t n = static_cast<uint32_t>(lds_write_bytes(fo));
          f(Access{kLdsSpace, c + static_cast<uint32_t>(lds_write_sub(lane, fo)), n, n == 12 ? 16u : n, true});
        }
        for (uint32_t n : {4u, 8u}) {                                              // read2 / write2 and their st64 forms
          f(Access{kLdsSpace, c, n, n, true});
          f(Access{kLdsSpace, c + 8, n, n, true});                            // offset1 2 of 4 bytes, 1 of 8
          f(Access{kLdsSpace, c + kLdsUpper, n, n, true});
        }
      }
      break;
    case kLdstr:
      for (int s = 0; s < kLdstrSteps; ++s) f(Access{kLdsSpace, ldstr_addr(s, lane), 8, 8, true});
      break;
    case kLdsdma:
      for (int fo = 0; fo < kDmaForms; ++fo) {
        const uint32_t n = static_cast<uint32_t>(dma_bytes(fo));
        f(Access{kTable, dma_src(wave, lane, fo), n, n, false});
        f(Access{kLdsSpace, dma_dst(fo) + l * n, n, n, true});
        f(Access{kLdsSpace, dma_dst(fo) + l * 16u, 16, 16, true});                   // the background
      }
      break;
    default:
      for (int m = 0; m < 2; ++m) {
        f(Access{m == 0 ? kSlice : kLdsSpace, 8u * l, 8, 8, true});
        f(Access{m == 0 ? kSlice : kLdsSpace, kAtomContended, 4, 4, true});
      }
      f(Access{kLdsSpace, kAtomContended + 8, 8, 4, true});                          // the flags of the contended case
  }
}

// ---- record -----------------------------------------------------------------------------
constexpr int kMemRecordWords = 8;   // xcc, hw_id, fail (bit w: wave w saw a failure), SIMDs seen, failed-group bits,
                                     // first bad group, its lowest bad index, that index's wave (kNoBad: none)
NANOGPU_HD inline uint32_t pack_bad(uint32_t group, uint32_t index, uint32_t wave) { return (group << 20) | (index << 2) | wave; }
static_assert(kMaxGroupWords * kLanes <= (1 << 18) && kNumNames <= (1 << 11), "pack_bad holds every index, below kNoBad");

struct MemRecord {
  uint32_t xcc, hw_id, fail, simds, groups, bad_group, bad_index, bad_wave;
};

inline MemRecord decode_mem_record(const uint32_t* words, size_t block) {
  const uint32_t* w = words + block * kMemRecordWords;
  return MemRecord{w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]};
}

inline std::vector<uint32_t> mem_table() {
  std::vector<uint32_t> t(kTableWords);
  for (int i = 0; i < kTableWords; ++i) t[i] = table_word(static_cast<uint32_t>(i));
  return t;
}

// Bits that are the same in every word.
inline uint32_t uncovered_bits(const std::vector<uint32_t>& words) {
  uint32_t ones = 0, zeros = 0;
  for (uint32_t w : words) ones |= w, zeros |= ~w;
  return ~(ones & zeros);
}

}  // namespace mem
}  // namespace selftest
}  // namespace nanogpu
