// ---------------------------------------------------------------------------- memory part
// The CU's memory pipeline (nanogpu/selftest_mem_host.h): global and buffer loads and stores of every
// width, the per-CU L1, LDS instruction forms, the transposed LDS read, LDS-DMA and atomics with
// return. Every instruction form is one asm statement that ends in its own wait, or a builtin the
// compiler counts itself. The statements take per-lane addresses in VGPRs; the only scalar operand
// of an asm statement is the buffer descriptor, and that statement opens with the wait states a
// fresh SGPR needs.
namespace sm = nanogpu::selftest::mem;
using u32x3v = __attribute__((ext_vector_type(3))) uint32_t;

#define NANOGPU_MEM_LOAD(name, text, T)                                                                           \
  __device__ __forceinline__ T name(const void* p) {                                                              \
    T r;                                                                                                          \
    asm volatile(text "\n\ts_waitcnt vmcnt(0)" : "=&v"(r) : "v"(p) : "memory");                                   \
    return r;                                                                                                     \
  }
// A d16 load writes one half of its register; that half is returned.
#define NANOGPU_MEM_LOAD_D16(name, text, hi)                                                                      \
  __device__ __forceinline__ uint32_t name(const void* p) {                                                       \
    uint32_t r = sm::kD16Init;                                                                                    \
    asm volatile(text "\n\ts_waitcnt vmcnt(0)" : "+v"(r) : "v"(p) : "memory");                                    \
    return sm::gload_d16_half(r, hi);                                                                             \
  }
#define NANOGPU_MEM_STORE(name, text, T)                                                                          \
  __device__ __forceinline__ void name(void* p, T v) { asm volatile(text "\n\ts_waitcnt vmcnt(0)" : : "v"(p), "v"(v) : "memory"); }
NANOGPU_MEM_LOAD(gl_ubyte, "global_load_ubyte %0, %1, off", uint32_t)
NANOGPU_MEM_LOAD(gl_sbyte, "global_load_sbyte %0, %1, off", uint32_t)
NANOGPU_MEM_LOAD(gl_ushort, "global_load_ushort %0, %1, off", uint32_t)
NANOGPU_MEM_LOAD(gl_sshort, "global_load_sshort %0, %1, off", uint32_t)
NANOGPU_MEM_LOAD_D16(gl_ubyte_d16, "global_load_ubyte_d16 %0, %1, off", false)
NANOGPU_MEM_LOAD_D16(gl_ubyte_d16_hi, "global_load_ubyte_d16_hi %0, %1, off", true)
NANOGPU_MEM_LOAD_D16(gl_sbyte_d16, "global_load_sbyte_d16 %0, %1, off", false)
NANOGPU_MEM_LOAD_D16(gl_sbyte_d16_hi, "global_load_sbyte_d16_hi %0, %1, off", true)
NANOGPU_MEM_LOAD_D16(gl_short_d16, "global_load_short_d16 %0, %1, off", false)
NANOGPU_MEM_LOAD_D16(gl_short_d16_hi, "global_load_short_d16_hi %0, %1, off", true)
NANOGPU_MEM_LOAD(gl_x1, "global_load_dword %0, %1, off", uint32_t)
NANOGPU_MEM_LOAD(gl_x2, "global_load_dwordx2 %0, %1, off", u32x2v)
NANOGPU_MEM_LOAD(gl_x3, "global_load_dwordx3 %0, %1, off", u32x3v)
NANOGPU_MEM_LOAD(gl_x4, "global_load_dwordx4 %0, %1, off", u32x4v)
NANOGPU_MEM_LOAD(gl_x4_nt, "global_load_dwordx4 %0, %1, off nt", u32x4v)
NANOGPU_MEM_LOAD(gl_x4_sc0, "global_load_dwordx4 %0, %1, off sc0", u32x4v)
NANOGPU_MEM_LOAD(gl_x4_sc1, "global_load_dwordx4 %0, %1, off sc1", u32x4v)
NANOGPU_MEM_LOAD(gl_x4_sc0sc1, "global_load_dwordx4 %0, %1, off sc0 sc1", u32x4v)
NANOGPU_MEM_STORE(gs_byte, "global_store_byte %0, %1, off", uint32_t)
NANOGPU_MEM_STORE(gs_short, "global_store_short %0, %1, off", uint32_t)
NANOGPU_MEM_STORE(gs_short_d16_hi, "global_store_short_d16_hi %0, %1, off", uint32_t)
NANOGPU_MEM_STORE(gs_x1, "global_store_dword %0, %1, off", uint32_t)
NANOGPU_MEM_STORE(gs_x2, "global_store_dwordx2 %0, %1, off", u32x2v)
NANOGPU_MEM_STORE(gs_x3, "global_store_dwordx3 %0, %1, off", u32x3v)
NANOGPU_MEM_STORE(gs_x4, "global_store_dwordx4 %0, %1, off", u32x4v)
#undef NANOGPU_MEM_LOAD
#undef NANOGPU_MEM_LOAD_D16
#undef NANOGPU_MEM_STORE

// LDS statements take the byte address in the LDS aperture.
#define NANOGPU_DS_READ(name, text, T)                                                                            \
  __device__ __forceinline__ T name(uint32_t a) {                                                                 \
    T r;                                                                                                          \
    asm volatile(text "\n\ts_waitcnt lgkmcnt(0)" : "=&v"(r) : "v"(a) : "memory");                                 \
    return r;                                                                                                     \
  }
#define NANOGPU_DS_WRITE(name, text, T)                                                                           \
  __device__ __forceinline__ void name(uint32_t a, T v) { asm volatile(text "\n\ts_waitcnt lgkmcnt(0)" : : "v"(a), "v"(v) : "memory"); }
#define NANOGPU_DS_WRITE2(name, text, T)                                                                          \
  __device__ __forceinline__ void name(uint32_t a, T v, T w) {                                                    \
    asm volatile(text "\n\ts_waitcnt lgkmcnt(0)" : : "v"(a), "v"(v), "v"(w) : "memory");                          \
  }
NANOGPU_DS_READ(ds_r_u8, "ds_read_u8 %0, %1", uint32_t)
NANOGPU_DS_READ(ds_r_i8, "ds_read_i8 %0, %1", uint32_t)
NANOGPU_DS_READ(ds_r_u16, "ds_read_u16 %0, %1", uint32_t)
NANOGPU_DS_READ(ds_r_i16, "ds_read_i16 %0, %1", uint32_t)
NANOGPU_DS_READ(ds_r_b32, "ds_read_b32 %0, %1", uint32_t)
NANOGPU_DS_READ(ds_r_b64, "ds_read_b64 %0, %1", u32x2v)
NANOGPU_DS_READ(ds_r_b96, "ds_read_b96 %0, %1", u32x3v)
NANOGPU_DS_READ(ds_r_b128, "ds_read_b128 %0, %1", u32x4v)
NANOGPU_DS_READ(ds_r2_b32, "ds_read2_b32 %0, %1 offset0:0 offset1:2", u32x2v)
NANOGPU_DS_READ(ds_r2_b64, "ds_read2_b64 %0, %1 offset0:0 offset1:1", u32x4v)
NANOGPU_DS_READ(ds_r2st64_b32, "ds_read2st64_b32 %0, %1 offset0:0 offset1:16", u32x2v)
NANOGPU_DS_READ(ds_r2st64_b64, "ds_read2st64_b64 %0, %1 offset0:0 offset1:8", u32x4v)
NANOGPU_DS_READ(ds_r_tr_b16, "ds_read_b64_tr_b16 %0, %1", u32x2v)
NANOGPU_DS_WRITE(ds_w_b8, "ds_write_b8 %0, %1", uint32_t)
NANOGPU_DS_WRITE(ds_w_b16, "ds_write_b16 %0, %1", uint32_t)
NANOGPU_DS_WRITE(ds_w_b32, "ds_write_b32 %0, %1", uint32_t)
NANOGPU_DS_WRITE(ds_w_b64, "ds_write_b64 %0, %1", u32x2v)
NANOGPU_DS_WRITE(ds_w_b96, "ds_write_b96 %0, %1", u32x3v)
NANOGPU_DS_WRITE(ds_w_b128, "ds_write_b128 %0, %1", u32x4v)
NANOGPU_DS_WRITE2(ds_w2_b32, "ds_write2_b32 %0, %1, %2 offset0:0 offset1:2", uint32_t)
NANOGPU_DS_WRITE2(ds_w2_b64, "ds_write2_b64 %0, %1, %2 offset0:0 offset1:1", u32x2v)
NANOGPU_DS_WRITE2(ds_w2st64_b32, "ds_write2st64_b32 %0, %1, %2 offset0:0 offset1:16", uint32_t)
NANOGPU_DS_WRITE2(ds_w2st64_b64, "ds_write2st64_b64 %0, %1, %2 offset0:0 offset1:8", u32x2v)
#undef NANOGPU_DS_READ
#undef NANOGPU_DS_WRITE
#undef NANOGPU_DS_WRITE2
static_assert(sm::kLdsUpper == 16 * 64 * 4 && sm::kLdsUpper == 8 * 64 * 8, "offset1 of the st64 statements");

// Everything this wave has in flight, whoever issued it.
__device__ __forceinline__ void mem_drain() { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); }

// Raw buffer statements, M: 0 offen, 1 offen with soffset 64, 2 offen with the immediate offset 48. The descriptor is four
// SGPRs fresh from readfirstlane, so every statement opens with the wait states such an operand needs.
#define NANOGPU_BUF_ASM(mnemonic, tail, outs, ...) \
  asm volatile("s_nop 4\n\t" mnemonic " %0, %1, %2, " tail "\n\ts_waitcnt vmcnt(0)" : outs : __VA_ARGS__ : "memory")
#define NANOGPU_BUF_LOAD(name, mnemonic, T)                                                                       \
  template <int M>                                                                                                \
  __device__ __forceinline__ T name(u32x4v rs, uint32_t voffset) {                                                \
    T r;                                                                                                          \
    if constexpr (M == 0) NANOGPU_BUF_ASM(mnemonic, "0 offen", "=&v"(r), "v"(voffset), "s"(rs));                  \
    if constexpr (M == 1) NANOGPU_BUF_ASM(mnemonic, "64 offen", "=&v"(r), "v"(voffset), "s"(rs));                 \
    if constexpr (M == 2) NANOGPU_BUF_ASM(mnemonic, "0 offen offset:48", "=&v"(r), "v"(voffset), "s"(rs));        \
    return r;                                                                                                     \
  }
#define NANOGPU_BUF_STORE(name, mnemonic, T)                                                                      \
  template <int M>                                                                                                \
  __device__ __forceinline__ void name(u32x4v rs, uint32_t voffset, T v) {                                        \
    if constexpr (M == 0) NANOGPU_BUF_ASM(mnemonic, "0 offen", , "v"(v), "v"(voffset), "s"(rs));                  \
    if constexpr (M == 1) NANOGPU_BUF_ASM(mnemonic, "64 offen", , "v"(v), "v"(voffset), "s"(rs));                 \
    if constexpr (M == 2) NANOGPU_BUF_ASM(mnemonic, "0 offen offset:48", , "v"(v), "v"(voffset), "s"(rs));        \
  }
NANOGPU_BUF_LOAD(bl_b8, "buffer_load_ubyte", uint32_t)
NANOGPU_BUF_LOAD(bl_b16, "buffer_load_ushort", uint32_t)
NANOGPU_BUF_LOAD(bl_b32, "buffer_load_dword", uint32_t)
NANOGPU_BUF_LOAD(bl_b64, "buffer_load_dwordx2", u32x2v)
NANOGPU_BUF_LOAD(bl_b96, "buffer_load_dwordx3", u32x3v)
NANOGPU_BUF_LOAD(bl_b128, "buffer_load_dwordx4", u32x4v)
NANOGPU_BUF_STORE(bs_b8, "buffer_store_byte", uint32_t)
NANOGPU_BUF_STORE(bs_b16, "buffer_store_short", uint32_t)
NANOGPU_BUF_STORE(bs_b32, "buffer_store_dword", uint32_t)
NANOGPU_BUF_STORE(bs_b64, "buffer_store_dwordx2", u32x2v)
NANOGPU_BUF_STORE(bs_b96, "buffer_store_dwordx3", u32x3v)
NANOGPU_BUF_STORE(bs_b128, "buffer_store_dwordx4", u32x4v)
#undef NANOGPU_BUF_LOAD
#undef NANOGPU_BUF_STORE
#undef NANOGPU_BUF_ASM
static_assert(sm::kBufSoffset == 64 && sm::kBufImm == 48, "the soffset and the immediate of the statements above");

// What a group works on: the table, the wave's region of the slice and of the LDS array (as a pointer
// and as the byte address the ds_ statements take). `wave` is wave-uniform to the compiler.
struct MemCtx {
  const uint32_t* table;
  char* slice;
  uint32_t* lds;
  uint32_t lds_at;
  int wave, lane;
};

// The sweep's sink: the lowest index whose word is not what the header computes. `inject` (kNoBad:
// none) is the index whose expected value has bit 0 flipped.
struct MemCheck {
  int lane;
  uint32_t inject, bad;
  __device__ __forceinline__ void at(int, uint32_t index, uint32_t got, uint32_t want) {
    if (got != (want ^ (index == inject ? 1u : 0u)) && index < bad) bad = index;
  }
  __device__ __forceinline__ void word(int k, uint32_t got, uint32_t want) { at(k, static_cast<uint32_t>(k * sm::kLanes + lane), got, want); }
};

// mem_lanes' sink: the raw words, [wave][k][lane].
struct MemKeep {
  uint32_t* out;
  int words, wave, lane;
  __device__ __forceinline__ void at(int k, uint32_t, uint32_t got, uint32_t) { out[(wave * words + k) * sm::kLanes + lane] = got; }
  __device__ __forceinline__ void word(int k, uint32_t got, uint32_t want) { at(k, 0u, got, want); }
};

template <int N, class V, class Sink, class Want>
__device__ __forceinline__ void mem_words(Sink& sink, int first, const V& got, Want&& want) {
#pragma unroll
  for (int j = 0; j < N; ++j) {
    uint32_t g;
    if constexpr (std::is_same_v<V, uint32_t>) g = got;
    else g = got[j];
    sink.word(first + j, g, want(j));
  }
}

template <class Sink>
__device__ __forceinline__ void mem_gload(const MemCtx& c, Sink& sink) {
#pragma nounroll
  for (int map = 0; map < sm::kGloadMaps; ++map) {
    auto p = [&](int f) { return reinterpret_cast<const char*>(c.table) + sm::gload_addr(map, c.wave, c.lane, f); };
    auto one = [&](int f, uint32_t got) { sink.word(sm::gload_k(map, f, 0), got, sm::gload_expected(map, c.wave, c.lane, f, 0)); };
    auto want = [&](int f) { return [&c, map, f](int j) { return sm::gload_expected(map, c.wave, c.lane, f, j); }; };
    one(0, gl_ubyte(p(0)));
    one(1, gl_ubyte(p(1)));
    one(2, gl_ubyte(p(2)));
    one(3, gl_ubyte(p(3)));
    one(4, gl_sbyte(p(4)));
    one(5, gl_sbyte(p(5)));
    one(6, gl_sbyte(p(6)));
    one(7, gl_sbyte(p(7)));
    one(8, gl_ushort(p(8)));
    one(9, gl_ushort(p(9)));
    one(10, gl_sshort(p(10)));
    one(11, gl_sshort(p(11)));
    one(12, gl_ubyte_d16(p(12)));
    one(13, gl_ubyte_d16_hi(p(13)));
    one(14, gl_sbyte_d16(p(14)));
    one(15, gl_sbyte_d16_hi(p(15)));
    one(16, gl_short_d16(p(16)));
    one(17, gl_short_d16_hi(p(17)));
    one(18, gl_x1(p(18)));
    mem_words<2>(sink, sm::gload_k(map, 19, 0), gl_x2(p(19)), want(19));
    mem_words<3>(sink, sm::gload_k(map, 20, 0), gl_x3(p(20)), want(20));
    mem_words<4>(sink, sm::gload_k(map, 21, 0), gl_x4(p(21)), want(21));
    mem_words<4>(sink, sm::gload_k(map, 22, 0), gl_x4_nt(p(22)), want(22));
    mem_words<4>(sink, sm::gload_k(map, 23, 0), gl_x4_sc0(p(23)), want(23));
    mem_words<4>(sink, sm::gload_k(map, 24, 0), gl_x4_sc1(p(24)), want(24));
    mem_words<4>(sink, sm::gload_k(map, 25, 0), gl_x4_sc0sc1(p(25)), want(25));
  }
}
static_assert(sm::kGloadForms == 26 && sm::gload_kind(17) == sm::kShortD16Hi && sm::gload_kind(18) == sm::kDwords, "the statements above, in the header's order");

// Four loads, then one wait, a statement: every wave reads every line of the table, twice.
template <class Sink>
__device__ __forceinline__ void mem_l1(const MemCtx& c, Sink& sink) {
#pragma nounroll
  for (int pass = 0; pass < sm::kL1Passes; ++pass) {
#pragma nounroll
    for (int step = 0; step < sm::kL1Steps; step += 4) {
      const u32x4v* t = reinterpret_cast<const u32x4v*>(c.table);
      uint32_t chunk[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) chunk[i] = sm::l1_chunk(pass, step + i, c.lane);
      u32x4v v0, v1, v2, v3;
      asm volatile("global_load_dwordx4 %0, %4, off\n\tglobal_load_dwordx4 %1, %5, off\n\tglobal_load_dwordx4 %2, %6, off\n\t"
                   "global_load_dwordx4 %3, %7, off\n\ts_waitcnt vmcnt(0)"
                   : "=&v"(v0), "=&v"(v1), "=&v"(v2), "=&v"(v3)
                   : "v"(t + chunk[0]), "v"(t + chunk[1]), "v"(t + chunk[2]), "v"(t + chunk[3])
                   : "memory");
      const u32x4v v[4] = {v0, v1, v2, v3};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint32_t word = 4 * chunk[i] + j;
          sink.at(sm::l1_k(pass, step + i, j), word, v[i][j], sm::table_word(word));
        }
    }
  }
}
static_assert(sm::kL1Steps % 4 == 0, "four loads a statement");

template <class Sink>
__device__ __forceinline__ void mem_gstore(const MemCtx& c, Sink& sink) {
  auto form = [&](auto fc) {
    constexpr int f = decltype(fc)::value;
    u32x4v bg;
#pragma unroll
    for (int j = 0; j < 4; ++j) bg[j] = sm::gstore_bg(c.wave, f, 4 * c.lane + j);
    gs_x4(c.slice + 16 * c.lane, bg);
    const uint32_t chunk = sm::gstore_chunk(c.wave, c.lane, f);
    char* p = c.slice + chunk + sm::gstore_sub(c.lane, f);
    auto v = [&](int j) { return sm::gstore_val(c.wave, c.lane, f, j); };
    if constexpr (f == 0) gs_byte(p, v(0));
    if constexpr (f == 1) gs_short(p, v(0));
    if constexpr (f == 2) gs_short_d16_hi(p, v(0));
    if constexpr (f == 3) gs_x1(p, v(0));
    if constexpr (f == 4) gs_x2(p, u32x2v{v(0), v(1)});
    if constexpr (f == 5) gs_x3(p, u32x3v{v(0), v(1), v(2)});
    if constexpr (f == 6) gs_x4(p, u32x4v{v(0), v(1), v(2), v(3)});
    mem_words<4>(sink, sm::gstore_k(f, 0), gl_x4(c.slice + chunk), [&](int j) { return sm::gstore_expected(c.wave, c.lane, f, j); });
  };
  form(std::integral_constant<int, 0>{});
  form(std::integral_constant<int, 1>{});
  form(std::integral_constant<int, 2>{});
  form(std::integral_constant<int, 3>{});
  form(std::integral_constant<int, 4>{});
  form(std::integral_constant<int, 5>{});
  form(std::integral_constant<int, 6>{});
}
static_assert(sm::kGstoreForms == 7, "the forms above");

// W: the header's width index (1, 2, 4, 8, 12, 16 bytes); M: 0 offen, 1 soffset, 2 immediate. The result is padded to four words.
template <int W, int M>
__device__ __forceinline__ u32x4v mem_buf_load(u32x4v rs, uint32_t voffset) {
  u32x4v r = {0u, 0u, 0u, 0u};
  if constexpr (W == 0) r[0] = bl_b8<M>(rs, voffset);
  if constexpr (W == 1) r[0] = bl_b16<M>(rs, voffset);
  if constexpr (W == 2) r[0] = bl_b32<M>(rs, voffset);
  if constexpr (W == 3) { const u32x2v v = bl_b64<M>(rs, voffset); r[0] = v[0], r[1] = v[1]; }
  if constexpr (W == 4) { const u32x3v v = bl_b96<M>(rs, voffset); r[0] = v[0], r[1] = v[1], r[2] = v[2]; }
  if constexpr (W == 5) r = bl_b128<M>(rs, voffset);
  return r;
}

template <int W, int M>
__device__ __forceinline__ void mem_buf_store(u32x4v rs, uint32_t voffset, u32x4v v) {
  if constexpr (W == 0) bs_b8<M>(rs, voffset, v[0]);
  if constexpr (W == 1) bs_b16<M>(rs, voffset, v[0]);
  if constexpr (W == 2) bs_b32<M>(rs, voffset, v[0]);
  if constexpr (W == 3) bs_b64<M>(rs, voffset, u32x2v{v[0], v[1]});
  if constexpr (W == 4) bs_b96<M>(rs, voffset, u32x3v{v[0], v[1], v[2]});
  if constexpr (W == 5) bs_b128<M>(rs, voffset, v);
}

// The wave's whole region, background `phase`.
__device__ __forceinline__ void mem_buf_background(const MemCtx& c, int phase) {
#pragma unroll
  for (uint32_t i = 0; i < sm::kWaveBytes / (16 * sm::kLanes); ++i) {
    const uint32_t chunk = c.lane + 64 * i;
    u32x4v bg;
#pragma unroll
    for (int j = 0; j < 4; ++j) bg[j] = sm::buf_bg(c.wave, phase, 4 * chunk + j);
    gs_x4(c.slice + 16 * chunk, bg);
  }
}

template <class Sink>
__device__ __forceinline__ void mem_buffer(const MemCtx& c, Sink& sink) {
  // the descriptor from wave-uniform values only: the halves of the region's address through readfirstlane
  const uint64_t base = reinterpret_cast<uint64_t>(c.slice);
  const uint32_t lo = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(base)));
  const uint32_t hi = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(base >> 32)));
  const u32x4v rs = {lo, hi & 0xffffu, sm::kBufRecords, 0x00020000u};   // stride 0, raw
  mem_buf_background(c, 0);
  auto load = [&](auto wc, auto mc) {
    constexpr int w = decltype(wc)::value, m = decltype(mc)::value;
    const u32x4v r = mem_buf_load<w, m>(rs, sm::buf_voffset(w, m, c.lane));
    mem_words<sm::buf_words(w)>(sink, sm::buf_load_k(w, m, 0), r, [&](int j) { return sm::buf_load_expected(c.wave, c.lane, w, m, j); });
  };
  auto store = [&](auto wc, auto mc) {
    constexpr int w = decltype(wc)::value, m = decltype(mc)::value;
    mem_buf_background(c, 1 + 3 * w + m);
    u32x4v v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = sm::buf_val(c.wave, c.lane, w, m, j);
    mem_buf_store<w, m>(rs, sm::buf_voffset(w, m, c.lane), v);
    mem_words<4>(sink, sm::buf_store_k(w, m, 0), gl_x4(c.slice + (sm::buf_addr(w, m, c.lane) & ~15u)),
                 [&](int j) { return sm::buf_store_expected(c.wave, c.lane, w, m, j); });
  };
  auto widths = [&](auto&& op, auto mc) {
    op(std::integral_constant<int, 0>{}, mc);
    op(std::integral_constant<int, 1>{}, mc);
    op(std::integral_constant<int, 2>{}, mc);
    op(std::integral_constant<int, 3>{}, mc);
    op(std::integral_constant<int, 4>{}, mc);
    op(std::integral_constant<int, 5>{}, mc);
  };
  widths(load, std::integral_constant<int, 0>{});
  widths(load, std::integral_constant<int, 1>{});
  widths(load, std::integral_constant<int, 2>{});
  widths(store, std::integral_constant<int, 0>{});
  widths(store, std::integral_constant<int, 1>{});
  widths(store, std::integral_constant<int, 2>{});
}
static_assert(sm::kBufWidths == 6 && sm::kBufModes == 3, "the forms above");

__device__ __forceinline__ u32x4v mem_lds_bg4(int wave, int phase, uint32_t at) {   // the chunk at byte `at` of the wave's region
  u32x4v bg;
#pragma unroll
  for (int j = 0; j < 4; ++j) bg[j] = sm::lds_bg(wave, phase, at / 4 + j);
  return bg;
}

template <class Sink>
__device__ __forceinline__ void mem_lds(const MemCtx& c, Sink& sink) {
#pragma nounroll
  for (int map = 0; map < sm::kLdsMaps; ++map) {
    const uint32_t chunk = sm::lds_chunk(map, c.lane), a = c.lds_at + chunk;
    auto background = [&](int phase) {
      ds_w_b128(a, mem_lds_bg4(c.wave, phase, chunk));
      ds_w_b128(a + sm::kLdsUpper, mem_lds_bg4(c.wave, phase, chunk + sm::kLdsUpper));
    };
    background(0);
    auto sub = [&](int f) { return a + sm::lds_read_sub(c.lane, f); };
    auto want = [&](int f) { return [&c, map, f](int j) { return sm::lds_read_expected(c.wave, c.lane, map, f, j); }; };
    auto first = [&](int f) { return sm::lds_read_k(map, f, 0); };
    mem_words<1>(sink, first(0), ds_r_u8(sub(0)), want(0));
    mem_words<1>(sink, first(1), ds_r_i8(sub(1)), want(1));
    mem_words<1>(sink, first(2), ds_r_u16(sub(2)), want(2));
    mem_words<1>(sink, first(3), ds_r_i16(sub(3)), want(3));
    mem_words<1>(sink, first(4), ds_r_b32(sub(4)), want(4));
    mem_words<2>(sink, first(5), ds_r_b64(sub(5)), want(5));
    mem_words<3>(sink, first(6), ds_r_b96(sub(6)), want(6));
    mem_words<4>(sink, first(7), ds_r_b128(sub(7)), want(7));
    mem_words<2>(sink, first(8), ds_r2_b32(a), want(8));
    mem_words<4>(sink, first(9), ds_r2_b64(a), want(9));
    mem_words<2>(sink, first(10), ds_r2st64_b32(a), want(10));
    mem_words<4>(sink, first(11), ds_r2st64_b64(a), want(11));
    auto write = [&](auto fc) {
      constexpr int f = decltype(fc)::value;
      background(1 + 10 * map + f);
      auto v = [&](int j) { return sm::lds_val(c.wave, c.lane, map, f, j); };
      const uint32_t at = a + sm::lds_write_sub(c.lane, f);
      if constexpr (f == 0) ds_w_b8(at, v(0));
      if constexpr (f == 1) ds_w_b16(at, v(0));
      if constexpr (f == 2) ds_w_b32(at, v(0));
      if constexpr (f == 3) ds_w_b64(at, u32x2v{v(0), v(1)});
      if constexpr (f == 4) ds_w_b96(at, u32x3v{v(0), v(1), v(2)});
      if constexpr (f == 5) ds_w_b128(at, u32x4v{v(0), v(1), v(2), v(3)});
      if constexpr (f == 6) ds_w2_b32(at, v(0), v(1));
      if constexpr (f == 7) ds_w2_b64(at, u32x2v{v(0), v(1)}, u32x2v{v(2), v(3)});
      if constexpr (f == 8) ds_w2st64_b32(at, v(0), v(1));
      if constexpr (f == 9) ds_w2st64_b64(at, u32x2v{v(0), v(1)}, u32x2v{v(2), v(3)});
      auto wantw = [&](int up) { return [&c, map, up](int j) { return sm::lds_write_expected(c.wave, c.lane, map, f, 4 * up + j); }; };
      mem_words<4>(sink, sm::lds_write_k(map, f, 0), ds_r_b128(a), wantw(0));
      if constexpr (f >= 8) mem_words<4>(sink, sm::lds_write_k(map, f, 4), ds_r_b128(a + sm::kLdsUpper), wantw(1));
    };
    write(std::integral_constant<int, 0>{});
    write(std::integral_constant<int, 1>{});
    write(std::integral_constant<int, 2>{});
    write(std::integral_constant<int, 3>{});
    write(std::integral_constant<int, 4>{});
    write(std::integral_constant<int, 5>{});
    write(std::integral_constant<int, 6>{});
    write(std::integral_constant<int, 7>{});
    write(std::integral_constant<int, 8>{});
    write(std::integral_constant<int, 9>{});
  }
}
static_assert(sm::kLdsReadForms == 12 && sm::kLdsWriteForms == 10, "the forms above");

// All 64 lanes are active: the caller's branch around the group is wave-uniform and nothing here diverges.
template <class Sink>
__device__ __forceinline__ void mem_ldstr(const MemCtx& c, Sink& sink) {
#pragma unroll
  for (int s = 0; s < sm::kLdstrSteps; ++s) {
    const uint32_t a = c.lds_at + sm::ldstr_addr(s, c.lane);
    ds_w_b64(a, u32x2v{sm::ldstr_written(c.wave, s, c.lane, 0), sm::ldstr_written(c.wave, s, c.lane, 1)});
    mem_words<2>(sink, sm::ldstr_k(s, 0), ds_r_tr_b16(a), [&](int j) { return sm::ldstr_expected(c.wave, s, c.lane, j); });
  }
}

using lds_u32_ptr = __attribute__((address_space(3))) uint32_t*;

template <class Sink>
__device__ __forceinline__ void mem_ldsdma(const MemCtx& c, Sink& sink) {
#pragma unroll
  for (int f = 0; f < sm::kDmaForms; ++f) ds_w_b128(c.lds_at + sm::dma_dst(f) + 16 * c.lane, u32x4v{sm::kDmaBg, sm::kDmaBg, sm::kDmaBg, sm::kDmaBg});
  auto src = [&](int f) { return reinterpret_cast<const uint32_t*>(reinterpret_cast<const char*>(c.table) + sm::dma_src(c.wave, c.lane, f)); };
  auto dst = [&](int f) { return (lds_u32_ptr)(c.lds + sm::dma_dst(f) / 4); };   // wave-uniform: the hardware adds lane x size
  __builtin_amdgcn_global_load_lds(src(0), dst(0), 4, 0, 0);
  __builtin_amdgcn_global_load_lds(src(1), dst(1), 16, 0, 0);
  const __amdgpu_buffer_rsrc_t table = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(c.table), 0, sm::kTableBytes, 0x00020000);
  __builtin_amdgcn_raw_ptr_buffer_load_lds(table, dst(2), 4, sm::dma_src(c.wave, c.lane, 2), 0, 0, 0);
  mem_drain();   // LDS-DMA is counted by vmcnt; the reads below are this wave's own
#pragma unroll
  for (int f = 0; f < sm::kDmaForms; ++f)
#pragma unroll
    for (int j = 0; j < sm::dma_bytes(f) / 4; ++j)
      sink.word(sm::dma_k(f, j), ds_r_b32(c.lds_at + sm::dma_dst(f) + sm::dma_bytes(f) * c.lane + 4 * j), sm::dma_expected(c.wave, c.lane, f, j));
}

// One atomic with return on *p, which holds a: agent scope on the slice, workgroup scope on LDS.
template <int OP, int SCOPE, class T>
__device__ __forceinline__ T mem_atomic(T* p, T v, T cmp) {
  if constexpr (OP == sm::kAdd || OP == sm::kAdd64) return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, SCOPE);
  if constexpr (OP == sm::kSub) return __hip_atomic_fetch_sub(p, v, __ATOMIC_RELAXED, SCOPE);
  if constexpr (OP == sm::kSmin) return static_cast<T>(__hip_atomic_fetch_min(reinterpret_cast<int32_t*>(p), static_cast<int32_t>(v), __ATOMIC_RELAXED, SCOPE));
  if constexpr (OP == sm::kUmin) return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, SCOPE);
  if constexpr (OP == sm::kSmax) return static_cast<T>(__hip_atomic_fetch_max(reinterpret_cast<int32_t*>(p), static_cast<int32_t>(v), __ATOMIC_RELAXED, SCOPE));
  if constexpr (OP == sm::kUmax || OP == sm::kUmax64) return __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, SCOPE);
  if constexpr (OP == sm::kAnd) return __hip_atomic_fetch_and(p, v, __ATOMIC_RELAXED, SCOPE);
  if constexpr (OP == sm::kOr) return __hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, SCOPE);
  if constexpr (OP == sm::kXor) return __hip_atomic_fetch_xor(p, v, __ATOMIC_RELAXED, SCOPE);
  if constexpr (OP == sm::kInc && SCOPE == __HIP_MEMORY_SCOPE_AGENT) return __builtin_amdgcn_atomic_inc32(p, v, __ATOMIC_RELAXED, "agent");
  if constexpr (OP == sm::kInc && SCOPE != __HIP_MEMORY_SCOPE_AGENT) return __builtin_amdgcn_atomic_inc32(p, v, __ATOMIC_RELAXED, "workgroup");
  if constexpr (OP == sm::kDec && SCOPE == __HIP_MEMORY_SCOPE_AGENT) return __builtin_amdgcn_atomic_dec32(p, v, __ATOMIC_RELAXED, "agent");
  if constexpr (OP == sm::kDec && SCOPE != __HIP_MEMORY_SCOPE_AGENT) return __builtin_amdgcn_atomic_dec32(p, v, __ATOMIC_RELAXED, "workgroup");
  if constexpr (OP == sm::kSwap || OP == sm::kSwap64) return __hip_atomic_exchange(p, v, __ATOMIC_RELAXED, SCOPE);
  if constexpr (OP == sm::kCmpswap || OP == sm::kCmpswap64) {
    __hip_atomic_compare_exchange_strong(p, &cmp, v, __ATOMIC_RELAXED, __ATOMIC_RELAXED, SCOPE);
    return cmp;   // what the location held
  }
  __builtin_unreachable();
}

template <int M, class Sink>
__device__ __forceinline__ void mem_atomic_memory(const MemCtx& c, Sink& sink) {
  constexpr int scope = M == 0 ? __HIP_MEMORY_SCOPE_AGENT : __HIP_MEMORY_SCOPE_WORKGROUP;
  char* region = M == 0 ? c.slice : reinterpret_cast<char*>(c.lds);
  auto op = [&](auto oc) {
    constexpr int o = decltype(oc)::value;
    using T = std::conditional_t<(o < sm::kNumOps32), uint32_t, uint64_t>;
    T* p = reinterpret_cast<T*>(region + 8 * c.lane);
    __hip_atomic_store(p, static_cast<T>(sm::atom_a(M, c.wave, c.lane, o)), __ATOMIC_RELAXED, scope);
    const T got = mem_atomic<o, scope, T>(p, static_cast<T>(sm::atom_v(M, c.wave, c.lane, o)), static_cast<T>(sm::atom_cmp(M, c.wave, c.lane, o)));
    const T after = __hip_atomic_load(p, __ATOMIC_RELAXED, scope);
    constexpr int n = sizeof(T) / 4;
#pragma unroll
    for (int j = 0; j < 2 * n; ++j)
      sink.word(sm::atom_k(M, o, j), static_cast<uint32_t>((j < n ? got : after) >> (32 * (j % n))), sm::atom_expected(M, c.wave, c.lane, o, j));
  };
  op(std::integral_constant<int, sm::kAdd>{});
  op(std::integral_constant<int, sm::kSub>{});
  op(std::integral_constant<int, sm::kSmin>{});
  op(std::integral_constant<int, sm::kUmin>{});
  op(std::integral_constant<int, sm::kSmax>{});
  op(std::integral_constant<int, sm::kUmax>{});
  op(std::integral_constant<int, sm::kAnd>{});
  op(std::integral_constant<int, sm::kOr>{});
  op(std::integral_constant<int, sm::kXor>{});
  op(std::integral_constant<int, sm::kInc>{});
  op(std::integral_constant<int, sm::kDec>{});
  op(std::integral_constant<int, sm::kSwap>{});
  op(std::integral_constant<int, sm::kCmpswap>{});
  op(std::integral_constant<int, sm::kAdd64>{});
  op(std::integral_constant<int, sm::kUmax64>{});
  op(std::integral_constant<int, sm::kSwap64>{});
  op(std::integral_constant<int, sm::kCmpswap64>{});
  // contended: every lane adds c to one word; the flags of the returned values are gathered in LDS
  uint32_t* word = reinterpret_cast<uint32_t*>(region + sm::kAtomContended);
  uint32_t* flags = c.lds + (sm::kAtomContended + 8) / 4;
  __hip_atomic_store(word, sm::atom_cont_b(M, c.wave), __ATOMIC_RELAXED, scope);
  __hip_atomic_store(flags + (c.lane & 1), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  mem_drain();   // another lane's store, before this lane's add
  // one statement, address and operand in VGPRs: 64 lanes' adds reach the atomic unit (the builtin is folded by the
  // compiler into one add of 64 c by one lane when address and operand are wave-uniform)
  uint32_t got;
  const uint32_t add = sm::atom_cont_c(M, c.wave);
  if constexpr (M == 0)
    asm volatile("global_atomic_add %0, %1, %2, off sc0\n\ts_waitcnt vmcnt(0)" : "=&v"(got) : "v"(word), "v"(add) : "memory");
  else
    asm volatile("ds_add_rtn_u32 %0, %1, %2\n\ts_waitcnt lgkmcnt(0)" : "=&v"(got) : "v"(c.lds_at + sm::kAtomContended), "v"(add) : "memory");
  const uint32_t q = sm::atom_cont_q(M, c.wave, got);
  __hip_atomic_fetch_or(flags + (q == sm::kNoBad ? 0u : q >> 5), q == sm::kNoBad ? 0u : 1u << (q & 31u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  mem_drain();
  sink.word(sm::atom_cont_k(M, 0), q == sm::kNoBad ? 0u : 1u, sm::atom_cont_expected(M, c.wave, 0));
  sink.word(sm::atom_cont_k(M, 1), __hip_atomic_load(flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP), sm::atom_cont_expected(M, c.wave, 1));
  sink.word(sm::atom_cont_k(M, 2), __hip_atomic_load(flags + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP), sm::atom_cont_expected(M, c.wave, 2));
  sink.word(sm::atom_cont_k(M, 3), __hip_atomic_load(word, __ATOMIC_RELAXED, scope), sm::atom_cont_expected(M, c.wave, 3));
}
static_assert(sm::kNumOps == 17, "the operations above");
static_assert(sm::kDmaForms == 3 && sm::dma_bytes(1) == 16, "mem_ldsdma's three loads");

template <class Sink>
__device__ __forceinline__ void mem_atomic_group(const MemCtx& c, Sink& sink) {
  mem_atomic_memory<0>(c, sink);
  mem_atomic_memory<1>(c, sink);
}

template <int G, class Sink>
__device__ __forceinline__ void mem_group(const MemCtx& c, Sink& sink) {
  if constexpr (G == sm::kGload) mem_gload(c, sink);
  if constexpr (G == sm::kL1) mem_l1(c, sink);
  if constexpr (G == sm::kGstore) mem_gstore(c, sink);
  if constexpr (G == sm::kBuffer) mem_buffer(c, sink);
  if constexpr (G == sm::kLds) mem_lds(c, sink);
  if constexpr (G == sm::kLdstr) mem_ldstr(c, sink);
  if constexpr (G == sm::kLdsdma) mem_ldsdma(c, sink);
  if constexpr (G == sm::kAtomic) mem_atomic_group(c, sink);
}
using MemGroups = std::make_integer_sequence<int, sm::kNumNames>;

// Test hook: on CU (xcc, cu_key), bit 0 flips of the value index `index` of group `group` is compared
// with, on wave index % 4. No held data is touched.
struct MemInject {
  int xcc = -1, cu_key = -1, group = -1, index = -1;
};

// More than half of the CU's 160 KiB, as kScalarLdsDwords: one workgroup a CU.
constexpr uint32_t kMemLdsDwords = sm::kLdsArrayBytes / 4;   // 84 KiB
constexpr uint32_t kMemRed = sm::kWaves * sm::kLdsWaveBytes / 4;
static_assert(kMemLdsDwords * 2 > kLdsDwordsFull && kMemLdsDwords >= kMemRed + 4, "alone on its CU; the waves' regions and the reduction fit");

__device__ __forceinline__ MemCtx mem_ctx(const uint32_t* table, uint8_t* slice, uint32_t* lds, int wave, int lane) {
  return MemCtx{table, reinterpret_cast<char*>(slice) + static_cast<uint32_t>(wave) * sm::kWaveBytes,
                lds + static_cast<uint32_t>(wave) * (sm::kLdsWaveBytes / 4),
                static_cast<uint32_t>(reinterpret_cast<uintptr_t>(lds)) + static_cast<uint32_t>(wave) * sm::kLdsWaveBytes, wave, lane};
}

template <int... G>
__device__ __forceinline__ void mem_groups_checked(std::integer_sequence<int, G...>, const MemCtx& c, uint32_t groups, int inj_group,
                                                   uint32_t inj_index, uint32_t* red) {
  auto one = [&](auto gc) {
    constexpr int g = decltype(gc)::value;
    if (!(groups >> g & 1u)) return;   // wave-uniform: a kernel argument
    MemCheck sink{c.lane, inj_group == g ? inj_index : sm::kNoBad, sm::kNoBad};
    mem_group<g>(c, sink);
    if (sink.bad != sm::kNoBad) {
      atomicOr(&red[0], 1u << c.wave);
      atomicOr(&red[2], 1u << g);
      atomicMin(&red[3], sm::pack_bad(g, sink.bad, static_cast<uint32_t>(c.wave)));
    }
  };
  (one(std::integral_constant<int, G>{}), ...);
}

// One visit of one CU, on the grid and the stream of cu_sweep_kernel: all four waves (one per SIMD)
// run every selected group on the table, on their region of workgroup blockIdx.x's slice of
// `scratch` and on their region of the LDS array. One record per workgroup. It never writes EXEC;
// M0 is written only by the compiler, for LDS-DMA. No spin, no inter-workgroup traffic, every loop
// bounded by a constant; every branch around a group is wave-uniform.
__global__ __launch_bounds__(kSweepBlock) void cu_mem_kernel(const uint32_t* __restrict__ table, uint8_t* __restrict__ scratch,
                                                             uint32_t* __restrict__ out, MemInject inj, uint32_t groups) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kMemLdsDwords];
  uint32_t* red = lds + kMemRed;   // 0 fail, 1 simds, 2 groups, 3 first bad (pack_bad)
  const uint32_t tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(tid >> 6));
  uint32_t xcc, hwid;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
  const bool mine = inj.group >= 0 && xcc == static_cast<uint32_t>(inj.xcc) && st::hw_cu_key(hwid) == static_cast<uint32_t>(inj.cu_key) &&
                    (inj.index & 3) == wave;
  if (tid < 4) red[tid] = tid == 3 ? sm::kNoBad : 0u;
  __syncthreads();
  const MemCtx c = mem_ctx(table, scratch + static_cast<size_t>(blockIdx.x) * sm::kSliceBytes, lds, wave, static_cast<int>(lane));
  mem_groups_checked(MemGroups{}, c, groups, mine ? inj.group : -1, static_cast<uint32_t>(inj.index), red);
  if (lane == 0) atomicOr(&red[1], 1u << st::hw_simd(hwid));
  __syncthreads();
  if (tid == 0) {
    uint32_t* o = out + static_cast<size_t>(blockIdx.x) * sm::kMemRecordWords;
    const uint32_t b = red[3];
    o[0] = xcc;
    o[1] = hwid;
    o[2] = red[0];
    o[3] = red[1];
    o[4] = red[2];
    o[5] = b == sm::kNoBad ? sm::kNoBad : b >> 20;
    o[6] = b == sm::kNoBad ? sm::kNoBad : (b >> 2) & 0x3ffffu;
    o[7] = b == sm::kNoBad ? sm::kNoBad : b & 3u;
  }
}

// One workgroup of four waves, one group: every lane's raw result words at out[wave][k][lane]. It
// establishes on the device that the kernel's instructions give what the twin computes.
template <int G>
__global__ __launch_bounds__(kSweepBlock) void mem_lanes_kernel(const uint32_t* __restrict__ table, uint8_t* __restrict__ scratch,
                                                                uint32_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kMemLdsDwords];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x >> 6));
  const MemCtx c = mem_ctx(table, scratch, lds, wave, lane);
  MemKeep sink{out, sm::group_words(G), wave, lane};
  mem_group<G>(c, sink);
}

// ---- memory sweep (host) ----

const std::vector<uint32_t>& mem_table_words() {
  static const std::vector<uint32_t> table = sm::mem_table();
  return table;
}

using MemLanesKernel = void (*)(const uint32_t*, uint8_t*, uint32_t*);
static_assert(sm::kNoBad == st::kNoBadOffset, "or_minus1's 'none' word");

// The memory part (PartSession): the table, and one slice of scratch memory per workgroup of the grid.
struct MemPart {
  static constexpr const char* who = "cu_sweep_mem";
  static constexpr const char* sensitivity_who = "mem_sensitivity";
  static constexpr NameTable names{sm::kNumNames, sm::group_name, "memory group"};
  static constexpr uint32_t kAllGroups = sm::kAllGroups;
  static constexpr int kRecordWords = sm::kMemRecordWords;
  static constexpr auto kernel = cu_mem_kernel;
  static constexpr size_t kSliceBytes = sm::kSliceBytes;
  template <int G>
  static constexpr MemLanesKernel group_kernel = mem_lanes_kernel<G>;

  // inject of cu_sweep_mem: (xcc, cu_key, group, index).
  using Inject = MemInject;
  static Inject parse_inject(const py::object& inject) {
    Inject inj;
    const py::tuple t = inject_head(inject, 4, 4, "cu_sweep_mem: inject = (xcc, cu_key, group, index)", inj);
    if (t.empty()) return inj;
    inj.group = names.index(t[2].cast<std::string>());
    inj.index = t[3].cast<int>();
    if (inj.index < 0 || inj.index >= sm::group_indices(inj.group)) throw std::invalid_argument("cu_sweep_mem: inject index beyond the group's");
    return inj;
  }

  static std::vector<const std::vector<uint32_t>*> tables() { return {&mem_table_words()}; }
  static constexpr const char* flip_usage = "cu_sweep_mem: corrupt_expected = ('gload' | 'l1' | 'ldsdma', word, xor)";
  static FlipTarget flip_target(int table) {
    if (!(sm::kTableGroups >> table & 1u)) throw std::invalid_argument("corrupt_expected: a group that reads the table: gload, l1 or ldsdma");
    return {0, 0, sm::kTableWords};
  }
  static void check(uint32_t, const hipFuncAttributes&) { require_block_fits(who, kernel); }

  static void launch(hipStream_t stream, int blocks, const Uploads& up, uint8_t* slices, uint32_t* out,
                     uint32_t /*seed: the part's data are fixed*/, const Inject& j, uint32_t groups) {
    hipLaunchKernelGGL(cu_mem_kernel, dim3(blocks), dim3(kSweepBlock), 0, stream, up[0]->p(), slices, out, j, groups);
  }

  static py::tuple record_tuple(const uint32_t* words, int b) {
    const sm::MemRecord rec = sm::decode_mem_record(words, b);
    return py::make_tuple(rec.xcc, rec.hw_id, rec.fail, rec.simds, rec.groups, or_minus1(rec.bad_group), or_minus1(rec.bad_index),
                          or_minus1(rec.bad_wave));
  }
  static void extras(py::dict& d, const hipFuncAttributes& attr) {
    d["table_words"] = sm::kTableWords;
    d["slice_bytes"] = sm::kSliceBytes;
    d["num_regs"] = attr.numRegs;
  }

  // Per word the fields fail, failed-group bits, first bad group and its lowest bad index, of a sweep of group g alone.
  static uint32_t sensitivity_groups(int g) { return 1u << g; }
  static constexpr uint32_t kSensitivityMinus1 = 1u << 2 | 1u << 3;
  static std::array<uint32_t, 4> sensitivity_fields(const uint32_t* words, int b) {
    const sm::MemRecord rec = sm::decode_mem_record(words, b);
    return {rec.fail, rec.groups, rec.bad_group, rec.bad_index};
  }
};

// Group g on one workgroup of four waves: every lane's raw result words [wave][k][lane].
std::vector<uint32_t> mem_lanes(int g) {
  DevBuf<uint32_t> table(sm::kTableWords);
  DevBuf<uint8_t> slice(sm::kSliceBytes);
  HIP_OK(hipMemcpy(table.p, mem_table_words().data(), sm::kTableBytes, hipMemcpyHostToDevice));
  HIP_OK(hipMemset(slice.p, 0, sm::kSliceBytes));
  return one_workgroup_words(static_cast<size_t>(sm::kWaves) * sm::group_words(g) * sm::kLanes, [&](uint32_t* out) {
    hipLaunchKernelGGL(kernel_of<MemPart>(MemGroups{}, g), dim3(1), dim3(kSweepBlock), 0, 0, table.p, slice.p, out);
  });
}

