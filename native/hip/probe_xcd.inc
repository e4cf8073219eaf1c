// ---------------------------------------------------------------------------- XCD check
// Data that one XCD wrote, read on another (nanogpu/selftest_xcd_host.h). The eight L2s are not coherent with
// each other, a CU's L1 is never refreshed by another CU's stores, and atomics execute at the memory side, so
// three groups, on cu_sweep's grid and stream:
//   handoff  xcd_write_kernel fills a slice a workgroup with plain stores and enters it in its XCD's list;
//            xcd_read_kernel, the next launch, verifies from every XCD one slice of every XCD's list;
//   ticket   xcd_ticket_kernel: plain stores, agent-scope release, one relaxed ticket; the workgroup that
//            draws the last ticket acquires and verifies the slices of the others, which it had read before;
//   atomic   xcd_atomic_kernel: adds, or, xor, min, max and a counter from every workgroup onto the same words.
// No kernel waits for another workgroup: no spin, no poll, no sleep, every loop bounded by a constant or by the
// grid's size, and the workgroups need not be resident together. Every index read from memory goes through a
// range check of the header before it is part of an address; out of range is kind `dir` in the record. The
// directory is read through agent-scope atomic loads and the slices through per-lane 16-byte loads: nothing
// another workgroup wrote comes through the scalar cache.
namespace sx = nanogpu::selftest::xcd;

// Test hook. group kHandoff: readers on XCD b compare word 0 of XCD a's slices with bit 0 flipped; group
// kTicket: the last arriver of ticket group a does so for its first partner. -1: none.
struct XcdInject {
  int group = -1, a = -1, b = -1;
};

// More than half of the CU's 160 KiB: one workgroup a CU, so the grid spreads over every enabled CU.
constexpr uint32_t kXcdLdsDwords = 84 * 1024 / 4;
constexpr uint32_t kXcdRed = kXcdLdsDwords - 16;
static_assert(kXcdLdsDwords * 2 > kLdsDwordsFull, "alone on its CU");
static_assert(sx::kThreads == kSweepBlock, "a thread moves 16 bytes a step");

__device__ __forceinline__ uint32_t xcd_dir_load(uint32_t* dir, uint32_t at) {
  return __hip_atomic_load(dir + at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void xcd_ids(uint32_t& xcc, uint32_t& hwid) {
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hwid));
}

// The four steps of a hand-off slice: four plain 16-byte loads in flight, then one wait.
__device__ __forceinline__ void xcd_load4(const uint8_t* slices, uint32_t block, uint32_t tid, u32x4v (&v)[4]) {
  asm volatile("global_load_dwordx4 %0, %4, off\n\tglobal_load_dwordx4 %1, %5, off\n\tglobal_load_dwordx4 %2, %6, off\n\t"
               "global_load_dwordx4 %3, %7, off\n\ts_waitcnt vmcnt(0)"
               : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3])
               : "v"(slices + sx::slice_byte(block, tid, 0)), "v"(slices + sx::slice_byte(block, tid, 1)),
                 "v"(slices + sx::slice_byte(block, tid, 2)), "v"(slices + sx::slice_byte(block, tid, 3))
               : "memory");
}

// The lowest (block, word) this thread saw fail, with what it compared.
struct XcdFirst {
  uint32_t pack = sx::kNone, wxcc = sx::kNone, whwid = sx::kNone, expected = 0, observed = 0;
  __device__ __forceinline__ void see(uint32_t block, uint32_t word, uint32_t wx, uint32_t wh, uint32_t exp, uint32_t obs) {
    const uint32_t p = sx::pack_first(block, word);
    if (p < pack) pack = p, wxcc = wx, whwid = wh, expected = exp, observed = obs;
  }
  // red[0] holds the workgroup's lowest pack; the thread that saw it fills red[1..4]
  __device__ __forceinline__ void publish(uint32_t* red) const {
    if (pack != sx::kNone && pack == red[0]) red[1] = wxcc, red[2] = whwid, red[3] = expected, red[4] = observed;
  }
};

__device__ __forceinline__ void xcd_first_out(uint32_t* o, const uint32_t* red) {   // the six words of First
  const uint32_t p = red[0];
  o[0] = p == sx::kNone ? sx::kNone : p >> 12;
  o[1] = red[1];
  o[2] = red[2];
  o[3] = p == sx::kNone ? sx::kNone : p & 0xfffu;
  o[4] = red[3];
  o[5] = red[4];
}

// Workgroup b enters itself in its XCD's list and fills its hand-off slice and, with the before pattern, its
// ticket slice. Plain stores: they stay in the writing XCD's L2 until the kernel's end writes them back.
__global__ __launch_bounds__(kSweepBlock) void xcd_write_kernel(uint32_t* dir, uint8_t* slices, uint8_t* tslices, uint32_t* out,
                                                                uint32_t n, uint32_t seed) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kXcdLdsDwords];
  uint32_t* red = lds + kXcdRed;
  const uint32_t tid = threadIdx.x, b = blockIdx.x;
  uint32_t xcc, hwid;
  xcd_ids(xcc, hwid);
  if (tid == 0) red[0] = 0u, red[1] = sx::kNone;
  __syncthreads();
  if (tid == 0) {
    uint32_t kinds = 0, position = sx::kNone;
    if (sx::xcc_ok(xcc)) {
      position = __hip_atomic_fetch_add(dir + sx::count_at(xcc), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (position < n) gs_x1(dir + sx::list_at(xcc, position), b);
      else kinds |= sx::kKindDir;
    } else {
      kinds |= sx::kKindDir;
    }
    gs_x1(dir + sx::writer_at(b), xcc);
    gs_x1(dir + sx::writer_at(b) + 1, hwid);
    atomicOr(&red[0], kinds);   // LDS atomics, as in the other kernels: the array keeps its whole size
    atomicMin(&red[1], position);
  }
#pragma unroll
  for (uint32_t step = 0; step < sx::kSliceWords / (4 * sx::kThreads); ++step) {
    const uint32_t first = 4 * (step * sx::kThreads + tid);
    gs_x4(slices + sx::slice_byte(b, tid, step), u32x4v{sx::hand_word(seed, b, first), sx::hand_word(seed, b, first + 1),
                                                         sx::hand_word(seed, b, first + 2), sx::hand_word(seed, b, first + 3)});
  }
  gs_x4(tslices + sx::ticket_byte(b, tid), u32x4v{sx::ticket_word(seed, b, 4 * tid, 0), sx::ticket_word(seed, b, 4 * tid + 1, 0),
                                                  sx::ticket_word(seed, b, 4 * tid + 2, 0), sx::ticket_word(seed, b, 4 * tid + 3, 0)});
  __syncthreads();
  if (tid == 0) {
    uint32_t* o = out + static_cast<size_t>(b) * sx::kRecordWords + sx::kWriteAt;
    o[0] = xcc, o[1] = hwid, o[2] = red[0], o[3] = red[1];
  }
}

// Workgroup c, reader number q of its XCD, verifies for every XCD i with writers the slice of block
// list[i][q % count[i]], all 4,096 words, after checking that writer[] names XCD i for that block.
__global__ __launch_bounds__(kSweepBlock) void xcd_read_kernel(uint32_t* dir, const uint8_t* slices, uint32_t* out, uint32_t n,
                                                               uint32_t seed, XcdInject inj) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kXcdLdsDwords];
  uint32_t* red = lds + kXcdRed;   // 0..4 first, 5 kinds, 6 failed XCDs, 7 ordinal
  const uint32_t tid = threadIdx.x;
  uint32_t xcc, hwid;
  xcd_ids(xcc, hwid);
  if (tid == 0) {
    red[0] = red[1] = red[2] = sx::kNone;
    red[3] = red[4] = red[5] = red[6] = 0u;
    red[7] = sx::xcc_ok(xcc) ? __hip_atomic_fetch_add(dir + sx::readers_at(xcc), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : sx::kNone;
  }
  __syncthreads();
  const uint32_t q = red[7];
  uint32_t kinds = q == sx::kNone ? sx::kKindDir : 0u, checked = 0, failed = 0;
  XcdFirst first;
  for (uint32_t i = 0; i < sx::kXcds && q != sx::kNone; ++i) {
    const uint32_t count = xcd_dir_load(dir, sx::count_at(i));
    const uint32_t position = sx::pick_position(n, count, q);
    if (position == sx::kNone) {
      if (count != 0) kinds |= sx::kKindDir;
      continue;
    }
    const uint32_t block = xcd_dir_load(dir, sx::list_at(i, position));
    if (!sx::block_ok(n, block)) {
      kinds |= sx::kKindDir;
      continue;
    }
    const uint32_t wxcc = xcd_dir_load(dir, sx::writer_at(block)), whwid = xcd_dir_load(dir, sx::writer_at(block) + 1);
    checked |= 1u << i;
    if (wxcc != i) kinds |= sx::kKindWriter, failed |= 1u << i;
    const bool flip = inj.group == sx::kHandoff && inj.a == static_cast<int>(i) && inj.b == static_cast<int>(xcc);
    u32x4v v[4];
    xcd_load4(slices, block, tid, v);
#pragma unroll
    for (uint32_t step = 0; step < 4; ++step)
#pragma unroll
      for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t word = 4 * (step * sx::kThreads + tid) + k;
        const uint32_t expected = sx::hand_word(seed, block, word) ^ (flip && word == 0 ? 1u : 0u);
        if (v[step][k] != expected) {
          kinds |= sx::kKindData, failed |= 1u << i;
          first.see(block, word, wxcc, whwid, expected, v[step][k]);
        }
      }
  }
  if (kinds) atomicOr(&red[5], kinds);
  if (failed) atomicOr(&red[6], failed);
  if (first.pack != sx::kNone) atomicMin(&red[0], first.pack);
  __syncthreads();
  first.publish(red);
  __syncthreads();
  if (tid == 0) {
    uint32_t* o = out + static_cast<size_t>(blockIdx.x) * sx::kRecordWords + sx::kReadAt;
    o[0] = xcc, o[1] = hwid, o[2] = red[5], o[3] = checked & ~red[6], o[4] = red[6], o[5] = q;
    xcd_first_out(o + 6, red);
  }
}
static_assert(sx::kSliceWords == 16 * sx::kThreads, "xcd_load4's four steps are the slice");

// Workgroups 8g .. 8g+7 share ticket[g]. Each reads the others' slices (so that its L1 holds them), overwrites
// its own with the after pattern, releases and draws a ticket; the one that draws the last acquires and reads the
// others' slices again, which must now hold the after pattern, word for word. Nobody waits.
__global__ __launch_bounds__(kSweepBlock) void xcd_ticket_kernel(uint32_t* dir, uint8_t* tslices, uint32_t* out, uint32_t n, uint32_t seed,
                                                                 XcdInject inj) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kXcdLdsDwords];
  uint32_t* red = lds + kXcdRed;   // 0..4 first, 5 kinds, 6 failed XCDs, 7 ticket, 8 fold, 9 failed members
  const uint32_t tid = threadIdx.x, b = blockIdx.x;
  const uint32_t g = b / sx::kGroupSize, me = b % sx::kGroupSize, size = sx::group_size(n, g);
  uint32_t xcc, hwid;
  xcd_ids(xcc, hwid);
  if (tid == 0) {
    red[0] = red[1] = red[2] = sx::kNone;
    red[3] = red[4] = red[5] = red[6] = red[8] = red[9] = 0u;
    red[7] = sx::kNone;
  }
  __syncthreads();
  uint32_t kinds = 0, fold = 0;
  // 1: the others' slices by plain loads, before or after their owners' stores
  for (uint32_t j = 0; j < size; ++j) {
    if (j == me) continue;
    const uint32_t block = g * sx::kGroupSize + j;
    const u32x4v v = gl_x4(tslices + sx::ticket_byte(block, tid));
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
      const uint32_t before = sx::ticket_word(seed, block, 4 * tid + k, 0);
      if (v[k] != before && v[k] != ~before) kinds |= sx::kKindPreread;
      fold ^= v[k] ^ before;   // 0 or all ones a word
    }
  }
  if (fold) atomicXor(&red[8], fold);
  // 2: the after pattern over this workgroup's own slice, and who it is, by plain stores
  {
    const uint32_t first = 4 * tid;
    const u32x4v after = {sx::ticket_word(seed, b, first, 1), sx::ticket_word(seed, b, first + 1, 1), sx::ticket_word(seed, b, first + 2, 1),
                          sx::ticket_word(seed, b, first + 3, 1)};
    asm volatile("global_store_dwordx4 %0, %1, off" : : "v"(tslices + sx::ticket_byte(b, tid)), "v"(after) : "memory");
    if (tid == 0) {
      asm volatile("global_store_dword %0, %1, off" : : "v"(dir + sx::member_at(b)), "v"(xcc + 1u) : "memory");
      asm volatile("global_store_dword %0, %1, off" : : "v"(dir + sx::member_at(b) + 1), "v"(hwid) : "memory");
    }
  }
  // 3: every storing wave drains, then one lane releases at agent scope and draws the ticket
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    red[7] = __hip_atomic_fetch_add(dir + sx::ticket_at(g), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  const uint32_t ticket = red[7];
  const bool last = ticket == size - 1;   // the same in every thread: read from LDS after the barrier
  if (ticket >= size) kinds |= sx::kKindDir;
  uint32_t compared = 0, writers = 0, failed = 0, failed_members = 0;
  XcdFirst first;
  if (last) {
    // 4: one lane's acquire, its wait, the barrier, then every wave's plain loads
    if (tid == 0) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    const uint32_t partner = me == 0 ? 1u : 0u;
    for (uint32_t j = 0; j < size; ++j) {
      if (j == me) continue;
      const uint32_t block = g * sx::kGroupSize + j;
      const uint32_t id = gl_x1(dir + sx::member_at(block)), whwid = gl_x1(dir + sx::member_at(block) + 1);
      const bool known = id >= 1 && sx::xcc_ok(id - 1);
      const uint32_t wxcc = known ? id - 1 : sx::kNone, wbit = known ? 1u << (id - 1) : 0u;
      compared |= 1u << j, writers |= wbit;
      if (!known) kinds |= sx::kKindDir, failed_members |= 1u << j;
      const bool flip = inj.group == sx::kTicket && inj.a == static_cast<int>(g) && j == partner;
      const u32x4v v = gl_x4(tslices + sx::ticket_byte(block, tid));
#pragma unroll
      for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t word = 4 * tid + k;
        const uint32_t expected = sx::ticket_word(seed, block, word, 1) ^ (flip && word == 0 ? 1u : 0u);
        if (v[k] != expected) {
          kinds |= sx::kKindData, failed |= wbit, failed_members |= 1u << j;
          first.see(block, word, wxcc, whwid, expected, v[k]);
        }
      }
    }
  }
  if (kinds) atomicOr(&red[5], kinds);
  if (failed) atomicOr(&red[6], failed);
  if (failed_members) atomicOr(&red[9], failed_members);
  if (first.pack != sx::kNone) atomicMin(&red[0], first.pack);
  __syncthreads();
  first.publish(red);
  __syncthreads();
  if (tid == 0) {
    uint32_t* o = out + static_cast<size_t>(b) * sx::kRecordWords + sx::kTickAt;
    o[0] = xcc, o[1] = hwid, o[2] = red[5], o[3] = last ? 1u : 0u, o[4] = ticket;
    o[5] = static_cast<uint32_t>(__builtin_popcount(compared & ~red[9]));
    o[6] = writers & ~red[6], o[7] = red[6];
    xcd_first_out(o + 8, red);
    o[14] = red[8];
  }
}

// Every workgroup, from whichever XCD it runs on, updates the same words at the memory side: thread 0 the sums,
// the folds and its bit of the `or` bitmap, lane 0 of every wave the counter, whose returned value t sets bit t
// of the second bitmap. A bit found set was set twice.
__global__ __launch_bounds__(kSweepBlock) void xcd_atomic_kernel(uint32_t* dir, uint32_t* out, uint32_t n, uint32_t seed) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kXcdLdsDwords];
  uint32_t* red = lds + kXcdRed;   // 0 kinds, 1 duplicates
  const uint32_t tid = threadIdx.x, b = blockIdx.x;
  uint32_t xcc, hwid;
  xcd_ids(xcc, hwid);
  if (tid == 0) red[0] = red[1] = 0u;
  __syncthreads();
  constexpr int agent = __HIP_MEMORY_SCOPE_AGENT;
  if (tid == 0) {
    __hip_atomic_fetch_add(dir + sx::atom_at(sx::kAdd32), sx::atom_const(seed, b, 0), __ATOMIC_RELAXED, agent);
    __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(dir + sx::atom_at(sx::kAdd64)),
                           static_cast<unsigned long long>(sx::atom_add64(seed, b)), __ATOMIC_RELAXED, agent);
    __hip_atomic_fetch_xor(dir + sx::atom_at(sx::kXor), sx::atom_const(seed, b, 3), __ATOMIC_RELAXED, agent);
    __hip_atomic_fetch_max(dir + sx::atom_at(sx::kUmax), sx::atom_const(seed, b, 4), __ATOMIC_RELAXED, agent);
    __hip_atomic_fetch_max(reinterpret_cast<int32_t*>(dir + sx::atom_at(sx::kSmax)), static_cast<int32_t>(sx::atom_const(seed, b, 5)),
                           __ATOMIC_RELAXED, agent);
    __hip_atomic_fetch_min(dir + sx::atom_at(sx::kUmin), sx::atom_const(seed, b, 6), __ATOMIC_RELAXED, agent);
    __hip_atomic_fetch_min(reinterpret_cast<int32_t*>(dir + sx::atom_at(sx::kSmin)), static_cast<int32_t>(sx::atom_const(seed, b, 7)),
                           __ATOMIC_RELAXED, agent);
    const uint32_t bit = 1u << (b % 32);   // b < n <= kMaxBlocks: the grid's own index, not read from memory
    if (__hip_atomic_fetch_or(dir + sx::atom_at(sx::kOrMap + b / 32), bit, __ATOMIC_RELAXED, agent) & bit) {
      atomicOr(&red[0], sx::kKindDup);
      atomicAdd(&red[1], 1u);
    }
  }
  if ((tid & 63u) == 0) {
    const uint32_t t = __hip_atomic_fetch_add(dir + sx::atom_at(sx::kCounter), 1u, __ATOMIC_RELAXED, agent);
    if (t < 4 * n) {
      const uint32_t bit = 1u << (t % 32);
      if (__hip_atomic_fetch_or(dir + sx::atom_at(sx::kSeenMap + t / 32), bit, __ATOMIC_RELAXED, agent) & bit) {
        atomicOr(&red[0], sx::kKindDup);
        atomicAdd(&red[1], 1u);
      }
    } else {
      atomicOr(&red[0], sx::kKindDir);
    }
  }
  __syncthreads();
  if (tid == 0) {
    uint32_t* o = out + static_cast<size_t>(b) * sx::kRecordWords + sx::kAtomRecAt;
    o[0] = xcc, o[1] = hwid, o[2] = red[0], o[3] = red[1];
  }
}

// ---- XCD check (host) ----

constexpr NameTable kXcdNames{sx::kNumNames, sx::group_name, "XCD group"};

// Test hook: word `word` of block `block`'s hand-off slice is XORed by the host between the write and the read
// kernel. The write kernel of the next run stores the slice anew, so no flip outlives its run.
struct XcdCorrupt {
  int block = -1;
  uint32_t word = 0, mask = 0;
};

struct XcdRun {
  CuRun run;
  std::vector<uint32_t> dir;
  float ms[4] = {0.f, 0.f, 0.f, 0.f};   // write, read, ticket, atomic
};

struct XcdAttributes {
  int regs[4] = {0, 0, 0, 0};
  size_t scratch = 0;   // the largest of the four
};

// The CuSession of the four kernels: the directory with its initial image, and the two slices a workgroup. A
// run is one sequence on the session's stream with no host synchronisation in it, unless a slice is to be corrupted.
class XcdSession : public CuSession {
 public:
  static constexpr const char* who = "xcd_check";

  XcdSession(int dev, const std::vector<uint32_t>& mask, int rounds, uint32_t groups)
      : CuSession(who, dev, mask, checked_rounds(rounds), sx::kRecordWords), groups_(groups), dir_(sx::kDirWords), init_(sx::kDirWords),
        slices_(static_cast<size_t>(checked_blocks(blocks())) * sx::kSliceBytes), tslices_(static_cast<size_t>(blocks()) * sx::kTicketBytes) {
    if (!groups || (groups & ~sx::kAllGroups)) throw std::invalid_argument(std::string(who) + ": no group, or an unknown one");
    const void* kernels[4] = {reinterpret_cast<const void*>(xcd_write_kernel), reinterpret_cast<const void*>(xcd_read_kernel),
                              reinterpret_cast<const void*>(xcd_ticket_kernel), reinterpret_cast<const void*>(xcd_atomic_kernel)};
    for (int k = 0; k < 4; ++k) {
      hipFuncAttributes a{};
      HIP_OK(hipFuncGetAttributes(&a, kernels[k]));
      attr_.regs[k] = a.numRegs;
      attr_.scratch = std::max(attr_.scratch, static_cast<size_t>(a.localSizeBytes));
      if (a.sharedSizeBytes * 2 <= kLdsDwordsFull * sizeof(uint32_t))   // an array the compiler shrank would let two workgroups share a CU
        throw std::runtime_error(std::string(who) + ": a kernel holds " + std::to_string(a.sharedSizeBytes) + " bytes of LDS, not more than half a CU's");
    }
    require_block_fits(who, xcd_write_kernel);
    require_block_fits(who, xcd_read_kernel);
    require_block_fits(who, xcd_ticket_kernel);
    require_block_fits(who, xcd_atomic_kernel);
    const std::vector<uint32_t> initial = sx::dir_initial();
    HIP_OK(hipMemcpy(init_.p, initial.data(), sx::kDirWords * sizeof(uint32_t), hipMemcpyHostToDevice));
    warm_up([this](int blocks) { launch(blocks, 0u, XcdInject{}, false); });
  }

  void set_corrupt(const XcdCorrupt& c) {
    if (c.block >= 0 && (c.block >= blocks() || c.word >= sx::kSliceWords || !(groups_ >> sx::kHandoff & 1u)))
      throw std::invalid_argument(std::string(who) + ": corrupt = (block of the grid, byte offset in its 16 KiB slice, xor byte), with handoff selected");
    corrupt_ = c;
  }

  XcdRun run(uint32_t seed, const XcdInject& inj) {
    XcdRun r;
    r.run = CuSession::run([&](int blocks) { launch(blocks, seed, inj, true); });   // synchronises the stream
    hipEvent_t at[5] = {e01_.a, e01_.b, e23_.a, e23_.b, e4_.a};
    for (int k = 0; k < 4; ++k) HIP_OK(hipEventElapsedTime(&r.ms[k], at[k], at[k + 1]));
    r.dir.resize(sx::kDirWords);
    HIP_OK(hipMemcpy(r.dir.data(), dir_.p, sx::kDirWords * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return r;
  }

  const XcdAttributes& attributes() const { return attr_; }
  size_t bytes() const { return static_cast<size_t>(blocks()) * (sx::kSliceBytes + sx::kTicketBytes) + 2 * sx::kDirWords * sizeof(uint32_t); }
  using CuSession::blocks;

 private:
  static int checked_rounds(int rounds) {
    if (rounds < 1 || rounds > static_cast<int>(sx::kMaxRounds))
      throw std::invalid_argument(std::string(who) + ": rounds in 1..4, so that what an XCD writes stays under its L2");
    return rounds;
  }
  static int checked_blocks(int blocks) {
    if (blocks > static_cast<int>(sx::kMaxBlocks)) throw std::invalid_argument(std::string(who) + ": more than 1024 workgroups");
    return blocks;
  }

  void launch(int blocks, uint32_t seed, const XcdInject& inj, bool hooks) {
    const uint32_t n = static_cast<uint32_t>(blocks);
    const dim3 grid(n), block(kSweepBlock);
    hipStream_t s = stream();
    HIP_OK(hipMemcpyAsync(dir_.p, init_.p, sx::kDirWords * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
    HIP_OK(hipEventRecord(e01_.a, s));
    hipLaunchKernelGGL(xcd_write_kernel, grid, block, 0, s, dir_.p, slices_.p, tslices_.p, out(), n, seed);
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(e01_.b, s));
    if (hooks && corrupt_.block >= 0) {   // the one synchronisation inside a run
      HIP_OK(hipStreamSynchronize(s));
      uint32_t* at = reinterpret_cast<uint32_t*>(slices_.p + static_cast<size_t>(corrupt_.block) * sx::kSliceBytes) + corrupt_.word;
      uint32_t w = 0;
      HIP_OK(hipMemcpy(&w, at, 4, hipMemcpyDeviceToHost));
      w ^= corrupt_.mask;
      HIP_OK(hipMemcpy(at, &w, 4, hipMemcpyHostToDevice));
    }
    if (groups_ >> sx::kHandoff & 1u) hipLaunchKernelGGL(xcd_read_kernel, grid, block, 0, s, dir_.p, slices_.p, out(), n, seed, inj);
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(e23_.a, s));
    if (groups_ >> sx::kTicket & 1u) hipLaunchKernelGGL(xcd_ticket_kernel, grid, block, 0, s, dir_.p, tslices_.p, out(), n, seed, inj);
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(e23_.b, s));
    if (groups_ >> sx::kAtomic & 1u) hipLaunchKernelGGL(xcd_atomic_kernel, grid, block, 0, s, dir_.p, out(), n, seed);
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(e4_.a, s));
  }

  uint32_t groups_;
  XcdAttributes attr_;
  XcdCorrupt corrupt_;
  Events e01_, e23_, e4_;
  DevBuf<uint32_t> dir_, init_;
  DevBuf<uint8_t> slices_, tslices_;
};

// A section of record b as a tuple, None where its kernel did not run; a kernel that ran and left none is an error.
// Field `none` prints kNone as None (a position, an ordinal or a ticket not drawn); the six fields of the first
// failure from `first` (-1: the section has none) are None together, when it names no block.
py::object xcd_section(const uint32_t* words, int b, int at, int count, bool ran, int none, int first) {
  const uint32_t* w = words + static_cast<size_t>(b) * sx::kRecordWords;
  if (!ran) return py::none();
  if (!sx::section_written(w, at)) throw std::runtime_error(std::string(XcdSession::who) + ": workgroup " + std::to_string(b) + " left no record");
  py::tuple t(count);
  for (int i = 0; i < count; ++i) {
    const bool in_first = first >= 0 && i >= first && i < first + sx::kFirstWords;
    if (in_first ? w[at + first] == sx::kNone : i == none && w[at + i] == sx::kNone) t[i] = py::none();
    else t[i] = py::int_(w[at + i]);
  }
  return t;
}

py::list xcd_pairs(uint64_t pairs) {   // bit 8 writer + reader
  py::list out;
  for (int i = 0; i < 64; ++i)
    if (pairs >> i & 1u) out.append(py::make_tuple(i / 8, i % 8));
  return out;
}

XcdInject xcd_parse_inject(const py::object& inject, int& atomic_word) {
  XcdInject inj;
  atomic_word = -1;
  if (inject.is_none()) return inj;
  const py::tuple t = inject.cast<py::tuple>();
  const char* usage = "xcd_check: inject = ('handoff', writer xcc, reader xcc) | ('ticket', group) | ('atomic', word)";
  if (t.size() < 2) throw std::invalid_argument(usage);
  const int g = kXcdNames.index(t[0].cast<std::string>());
  if (t.size() != (g == sx::kHandoff ? 3u : 2u)) throw std::invalid_argument(usage);
  const int a = t[1].cast<int>();
  if (g == sx::kAtomic) {
    if (a < 0 || a >= static_cast<int>(sx::kAtomWords)) throw std::invalid_argument("xcd_check: inject word beyond the atomic words");
    atomic_word = a;
    return inj;
  }
  inj.group = g, inj.a = a, inj.b = g == sx::kHandoff ? t[2].cast<int>() : -1;
  if (a < 0 || (g == sx::kHandoff && (a >= 8 || inj.b < 0 || inj.b >= 8))) throw std::invalid_argument(usage);
  return inj;
}

py::dict xcd_check(int dev, const std::vector<uint32_t>& mask, int rounds, uint32_t seed, const std::vector<std::string>& groups,
                   const py::object& inject, const py::object& corrupt) {
  const uint32_t bits = kXcdNames.bits(groups);
  int atomic_word = -1;
  const XcdInject inj = xcd_parse_inject(inject, atomic_word);
  XcdCorrupt c;
  if (!corrupt.is_none()) {
    const py::tuple t = corrupt.cast<py::tuple>();
    if (t.size() != 3) throw std::invalid_argument("xcd_check: corrupt = (block, byte offset, xor byte)");
    const uint32_t offset = t[1].cast<uint32_t>(), x = t[2].cast<uint32_t>();
    if (x > 0xff || offset >= sx::kSliceBytes) throw std::invalid_argument("xcd_check: corrupt = (block, byte offset < 16384, xor byte)");
    c.block = t[0].cast<int>();
    if (c.block < 0) throw std::invalid_argument("xcd_check: corrupt = (block, byte offset, xor byte)");
    c.word = offset / 4, c.mask = x << (8 * (offset % 4));
  }
  XcdRun r;
  XcdAttributes attr;
  size_t bytes = 0;
  {
    py::gil_scoped_release nogil;
    HIP_OK(hipSetDevice(dev));
    XcdSession session(dev, mask, rounds, bits);
    session.set_corrupt(c);
    r = session.run(seed, inj);
    attr = session.attributes();
    bytes = session.bytes();
  }
  const bool handoff = bits >> sx::kHandoff & 1u, ticket = bits >> sx::kTicket & 1u, atomic = bits >> sx::kAtomic & 1u;
  const uint32_t n = static_cast<uint32_t>(r.run.blocks);
  py::list recs;
  uint64_t hand_pairs = 0, ticket_pairs = 0;
  for (int b = 0; b < r.run.blocks; ++b) {
    const uint32_t* w = r.run.words.data() + static_cast<size_t>(b) * sx::kRecordWords;
    const uint32_t* all = r.run.words.data();
    recs.append(py::make_tuple(xcd_section(all, b, sx::kWriteAt, 4, true, 3, -1), xcd_section(all, b, sx::kReadAt, 12, handoff, 5, 6),
                               xcd_section(all, b, sx::kTickAt, 15, ticket, 4, 8), xcd_section(all, b, sx::kAtomRecAt, 4, atomic, -1, -1)));
    if (handoff && sx::xcc_ok(w[sx::kReadAt]))
      for (uint32_t i = 0; i < sx::kXcds; ++i)
        if (w[sx::kReadAt + 3] >> i & 1u) hand_pairs |= uint64_t(1) << (8 * i + w[sx::kReadAt]);
    if (ticket && sx::xcc_ok(w[sx::kTickAt]))
      for (uint32_t i = 0; i < sx::kXcds; ++i)
        if (w[sx::kTickAt + 6] >> i & 1u) ticket_pairs |= uint64_t(1) << (8 * i + w[sx::kTickAt]);
  }
  py::dict d;
  d["records"] = recs;
  const auto [names, checked] = kXcdNames.names_and_checked(bits);
  d["groups"] = names;
  d["checked"] = checked;
  py::list words, expected, bad;
  if (atomic) {
    std::vector<uint64_t> want = sx::atomic_expected(seed, n);
    if (atomic_word >= 0) want[atomic_word] ^= 1u;
    for (uint32_t i = 0; i < sx::kAtomWords; ++i) {
      const uint64_t got = sx::atom_read(r.dir.data(), i);
      words.append(got);
      expected.append(want[i]);
      if (got != want[i]) bad.append(i);
    }
  }
  d["atomic_words"] = words;
  d["atomic_expected"] = expected;
  d["atomic_bad"] = bad;
  py::dict pairs;
  pairs["handoff"] = xcd_pairs(hand_pairs);
  pairs["ticket"] = xcd_pairs(ticket_pairs);
  pairs["atomic"] = py::list();
  d["pairs"] = pairs;
  d["blocks"] = r.run.blocks;
  d["bytes"] = bytes;
  py::list regs;
  for (int k = 0; k < 4; ++k) regs.append(attr.regs[k]);
  d["num_regs"] = regs;
  d["scratch_bytes"] = attr.scratch;
  py::dict ms;
  ms["write"] = r.ms[0], ms["read"] = r.ms[1], ms["ticket"] = r.ms[2], ms["atomic"] = r.ms[3];
  d["ms_kernels"] = ms;
  d["ms"] = r.run.ms;
  return d;
}

// xcd_sensitivity: per (word, xor) one run of the hand-off with that word of block 0's slice flipped after the write kernel.
py::dict xcd_sensitivity(int dev, const std::vector<std::pair<uint32_t, uint32_t>>& flips, const std::vector<uint32_t>& mask, int rounds,
                         uint32_t seed) {
  constexpr size_t N = 4;
  if (flips.size() > 4096) throw std::invalid_argument("xcd_sensitivity: at most 4096 words a call");
  Sensitivity r;
  {
    py::gil_scoped_release nogil;
    HIP_OK(hipSetDevice(dev));
    XcdSession session(dev, mask, rounds, 1u << sx::kHandoff);
    struct Runs {   // sensitivity<N> wants a CuRun
      XcdSession& s;
      CuRun run(uint32_t seed, const XcdInject& inj) { return s.run(seed, inj).run; }
    } runs{session};
    r = sensitivity<N>(
        runs, seed, flips, [&](const std::pair<uint32_t, uint32_t>& f) { session.set_corrupt(XcdCorrupt{0, f.first, f.second}); },
        [](const CuRun& run, int b) {
          const uint32_t* w = run.words.data() + static_cast<size_t>(b) * sx::kRecordWords + sx::kReadAt;
          return std::array<uint32_t, N>{w[2], w[4], w[6], w[9]};   // kinds, failed writer XCDs, first block, first word
        });
  }
  return sensitivity_dict(r, flips.size(), N, [](const uint32_t* f) {
    return py::make_tuple(f[0], f[1], or_minus1(f[2]), or_minus1(f[3]));
  });
}
