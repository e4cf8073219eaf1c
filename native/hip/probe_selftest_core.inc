// ---------------------------------------------------------------------------- deep self-test

constexpr int kSweepBlock = 256;               // 4 waves: one per SIMD's MFMA pipe

// ---------------------------------------------------------------------------- deep self-test (host)

// The names behind the bits of a sweep's selection: the matrix paths, the vector-ALU, scalar and memory groups.
struct NameTable {
  int count;
  const char* (*name)(int);
  const char* noun;

  int index(const std::string& n) const {
    for (int i = 0; i < count; ++i)
      if (n == name(i)) return i;
    throw std::invalid_argument(std::string("unknown ") + noun + " '" + n + "'");
  }
  uint32_t bits(const std::vector<std::string>& names) const {
    uint32_t b = 0;
    for (const std::string& n : names) b |= 1u << index(n);
    return b;
  }
  std::pair<py::list, py::list> names_and_checked(uint32_t bits) const {   // every name in bit order; those of `bits`
    py::list all, checked;
    for (int i = 0; i < count; ++i) {
      all.append(name(i));
      if (bits >> i & 1u) checked.append(name(i));
    }
    return {all, checked};
  }
};

// Test hook: a device copy of `count` host words of which one at a time is XORed. flip() first
// puts the word flipped before back as the host has it; the host array is never written. The
// stream is idle between runs (CuSession::run synchronises), so plain copies are ordered with it.
class FlippableUpload {
 public:
  FlippableUpload(const uint32_t* host, size_t count) : host_(host), dev_(count) {
    HIP_OK(hipMemcpy(dev_.p, host, count * sizeof(uint32_t), hipMemcpyHostToDevice));
  }
  const uint32_t* p() const { return dev_.p; }
  void flip(std::optional<size_t> at, uint32_t mask) {
    if (flipped_) write(*flipped_, 0u);
    flipped_ = at;
    if (at) write(*at, mask);
  }

 private:
  void write(size_t at, uint32_t mask) {
    const uint32_t w = host_[at] ^ mask;
    HIP_OK(hipMemcpy(dev_.p + at, &w, 4, hipMemcpyHostToDevice));
  }
  const uint32_t* host_;
  DevBuf<uint32_t> dev_;
  std::optional<size_t> flipped_;
};

// corrupt_expected as a session takes it: word `word` of table `table` XORed with `mask`; -1: none.
// The sweep's tables are 0 (the bf16 chain's tile) and 1 + p (path p's tile); the vector-ALU
// sweep's are its exact groups; the scalar sweep's are its exact groups and, as table ss::kSmem, the load table;
// the memory sweep's are the groups that read its one table (sm::kTableGroups), all naming that table.
struct WordFlip {
  int table = -1;
  uint32_t word = 0, mask = 0;
};

struct CuRun {
  std::vector<uint32_t> words;   // record_words per workgroup
  int record_words = 0, blocks = 0;
  double ms = 0.0;
};

// What every per-CU check shares: rounds x (enabled CUs) workgroups on a stream masked to `mask`,
// 0xff-filled records of which every workgroup must write its own, and a first launch outside the
// timed span. `who` begins the messages. A session derived from this holds its kernel's inputs,
// which are destroyed before the stream they were used on; `launch(blocks)` is its kernel's launch.
// Two derive from it: SweepSession (cu_sweep and cu_sweep_paths) and PartSession<P> (cu_sweep_valu,
// cu_sweep_scalar and cu_sweep_mem).
class CuSession {
 protected:
  CuSession(const char* who, int dev, const std::vector<uint32_t>& mask, int rounds, int record_words)
      : who_(who), stream_(mask), blocks_(grid(who_, dev, mask, rounds)), record_words_(record_words),
        out_(static_cast<size_t>(blocks_) * record_words) {}

  template <class Launch>
  void warm_up(Launch&& launch) {   // loads the code object
    launch(1);
    HIP_OK(hipStreamSynchronize(stream_.s));
  }

  template <class Launch>
  CuRun run(Launch&& launch) {
    CuRun res;
    res.blocks = blocks_;
    res.record_words = record_words_;
    const size_t words = static_cast<size_t>(blocks_) * record_words_;
    HIP_OK(hipMemsetAsync(out_.p, 0xff, words * sizeof(uint32_t), stream_.s));
    HIP_OK(hipEventRecord(ev_.a, stream_.s));
    launch(blocks_);
    HIP_OK(hipEventRecord(ev_.b, stream_.s));
    res.ms = ev_.ms();
    HIP_OK(hipStreamSynchronize(stream_.s));
    res.words.resize(words);
    HIP_OK(hipMemcpy(res.words.data(), out_.p, words * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (int b = 0; b < blocks_; ++b)
      if (!st::record_written(res.words.data() + static_cast<size_t>(b) * record_words_))
        throw std::runtime_error(who_ + ": workgroup " + std::to_string(b) + " left no record");
    return res;
  }

  hipStream_t stream() const { return stream_.s; }
  uint32_t* out() const { return out_.p; }
  int blocks() const { return blocks_; }

 private:
  static int grid(const std::string& who, int dev, const std::vector<uint32_t>& mask, int rounds) {
    if (rounds < 1 || rounds > 64) throw std::invalid_argument(who + ": rounds in 1..64");
    int cus = 0;
    if (mask.empty())
      cus = cu_count(dev);
    else
      for (uint32_t w : mask) cus += __builtin_popcount(w);
    if (cus <= 0 || cus > 4096) throw std::invalid_argument(who + ": the mask enables no CU");
    return rounds * cus;
  }

  std::string who_;
  Stream stream_;
  Events ev_;
  int blocks_, record_words_;
  DevBuf<uint32_t> out_;
};

// Test hook behind tests/test_gpu_selftest_sensitivity.py and test_gpu_selftest_valu.py: for every
// flip one run of `session` with `set_flip(flip)` applied. `fields(run, b)` picks N words of record
// b; per flip the AND of each over all records, then the OR of each: 2N words.
struct Sensitivity {
  std::vector<uint32_t> fields;
  int records = 0;                // per sweep
  double seconds = 0.0;           // wall time of the loop
};

template <size_t N, class Session, class Flip, class SetFlip, class Fields>
Sensitivity sensitivity(Session& session, uint32_t seed, const std::vector<Flip>& flips, SetFlip&& set_flip, Fields&& fields) {
  Sensitivity out;
  out.fields.reserve(flips.size() * 2 * N);
  const Clock::time_point t0 = Clock::now();
  for (const Flip& f : flips) {
    set_flip(f);
    const CuRun r = session.run(seed, {});
    out.records = r.blocks;
    std::array<uint32_t, N> a, o;
    a.fill(~0u);
    o.fill(0u);
    for (int b = 0; b < r.blocks; ++b) {
      const std::array<uint32_t, N> v = fields(r, b);
      for (size_t i = 0; i < N; ++i) a[i] &= v[i], o[i] |= v[i];
    }
    out.fields.insert(out.fields.end(), a.begin(), a.end());
    out.fields.insert(out.fields.end(), o.begin(), o.end());
  }
  out.seconds = std::chrono::duration<double>(Clock::now() - t0).count();
  return out;
}

// corrupt_expected = (table name, word, xor), or (word, xor) of table 0 where `names` is null. With `table0`
// that name is table 0 and `names`' are the tables from 1 (WordFlip). `usage` is the message.
int table_index(const NameTable& names, const char* table0, const std::string& name) {
  if (!table0) return names.index(name);
  return name == table0 ? 0 : 1 + names.index(name);
}

WordFlip parse_flip(const py::object& corrupt, const NameTable* names, const char* table0, const char* usage) {
  WordFlip f;
  if (corrupt.is_none()) return f;
  const py::tuple t = corrupt.cast<py::tuple>();
  const size_t named = names ? 1 : 0;
  if (t.size() != 2 + named) throw std::invalid_argument(usage);
  f.table = names ? table_index(*names, table0, t[0].cast<std::string>()) : 0;
  f.word = t[named].cast<uint32_t>();
  f.mask = t[named + 1].cast<uint32_t>();
  return f;
}

// One 'none' word in every record: each part asserts that its own is this one.
int64_t or_minus1(uint32_t v) { return v == st::kNoBadOffset ? int64_t(-1) : int64_t(v); }

// {words: [(AND tuple, OR tuple)] per flip, records, seconds}; `tuple` packs one half's n words.
template <class Tuple>
py::dict sensitivity_dict(const Sensitivity& r, size_t flips, size_t n, Tuple&& tuple) {
  py::list words;
  for (size_t i = 0; i < flips; ++i) {
    const uint32_t* f = r.fields.data() + 2 * n * i;
    words.append(py::make_tuple(tuple(f), tuple(f + n)));
  }
  py::dict d;
  d["words"] = words;
  d["records"] = r.records;
  d["seconds"] = r.seconds;
  return d;
}

// ---- the parts launched after the sweep: valu, scalar, mem ----
//
// A part is a struct P of static members, next to its kernels in its own file, that holds only what
// differs between the parts:
//   who, sensitivity_who     the bindings' names, which begin the messages
//   names, kAllGroups        the groups' NameTable and the mask of the legal ones
//   kRecordWords, kernel     of the part's __global__ function
//   Inject, parse_inject(o)  the kernel's test hook and its Python form (inject_head unpacks the common head)
//   tables()                 the host words to upload, one FlippableUpload each
//   kSliceBytes              device memory a workgroup of the grid gets for itself, allocated once per session
//   flip_target(table), flip_usage
//                            which words of which upload corrupt_expected's table names (throws when it names
//                            none), and the message for a corrupt_expected of another shape
//   check(groups, attr)      the part's refusals once the kernel's attributes are known (refuse_scratch,
//                            require_block_fits)
//   launch(...)              the kernel's launch: the three signatures differ
//   record_tuple(words, b)   record b as the binding returns it
//   extras(d, attr)          the result's keys between `checked` and `scratch_bytes`
//   sensitivity_groups(g)    the groups P_sensitivity runs when it corrupts group g's words
//   sensitivity_fields(words, b), kSensitivityMinus1
//                            the words of record b it reports; bit i set: field i prints kNoBad as -1
//   group_kernel<G>          the one-workgroup kernel of group G (kernel_of)
// Everything else is written once, below.

using Uploads = std::vector<std::unique_ptr<FlippableUpload>>;

// Words first.. of upload `upload`, `words` of them.
struct FlipTarget {
  size_t upload, first, words;
};

// The (xcc, cu_key, ...) head of every part's inject tuple into `inj`. Returns the tuple, of `min`..`max`
// items (else `usage` is thrown), or an empty one when there is no inject.
template <class Inject>
py::tuple inject_head(const py::object& inject, size_t min, size_t max, const char* usage, Inject& inj) {
  if (inject.is_none()) return py::tuple();
  const py::tuple t = inject.cast<py::tuple>();
  if (t.size() < min || t.size() > max) throw std::invalid_argument(usage);
  inj.xcc = t[0].cast<int>();
  inj.cu_key = t[1].cast<int>();
  return t;
}

// A pattern test of registers that was compiled with scratch would test memory: `group` is refused then.
void refuse_scratch(const char* who, const NameTable& names, int group, uint32_t groups, const hipFuncAttributes& attr) {
  if ((groups >> group & 1u) && attr.localSizeBytes != 0)
    throw std::runtime_error(std::string(who) + ": the kernel was compiled with " + std::to_string(attr.localSizeBytes) +
                             " bytes of scratch a lane, so '" + names.name(group) +
                             "' would test memory, not registers: it is refused");
}

// A kernel that holds more than half a CU's LDS to be alone on its CU: asked of the occupancy API, never found
// out by a failing launch.
template <class Kernel>
void require_block_fits(const char* who, Kernel kernel) {
  int fit = 0;
  HIP_OK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&fit, kernel, kSweepBlock, 0));
  if (fit < 1) throw std::runtime_error(std::string(who) + ": no workgroup of this part fits a CU of this device");
}

// The CuSession of part P's kernel: its tables, its slices, and the kernel's attributes, read once.
// P's binding is one session and one run, P's sensitivity a run per word.
template <class P>
class PartSession : public CuSession {
 public:
  PartSession(int dev, const std::vector<uint32_t>& mask, int rounds, uint32_t groups)
      : CuSession(P::who, dev, mask, rounds, P::kRecordWords), groups_(groups) {
    if (!groups || (groups & ~P::kAllGroups)) throw std::invalid_argument(std::string(P::who) + ": no group, or an unknown one");
    HIP_OK(hipFuncGetAttributes(&attr_, reinterpret_cast<const void*>(P::kernel)));
    P::check(groups, attr_);
    if (P::kSliceBytes) slices_.emplace(static_cast<size_t>(blocks()) * P::kSliceBytes);
    for (const std::vector<uint32_t>* t : P::tables()) uploads_.emplace_back(new FlippableUpload(t->data(), t->size()));
    warm_up([this](int blocks) { launch(blocks, 0u, typename P::Inject{}); });
  }

  void set_flip(const WordFlip& f) {
    for (auto& u : uploads_) u->flip(std::nullopt, 0u);   // every upload clean before the checks: a refused flip leaves none behind
    if (f.table < 0) return;
    const FlipTarget t = P::flip_target(f.table);
    if (!(groups_ >> f.table & 1u))
      throw std::invalid_argument(std::string("corrupt_expected: group ") + P::names.name(f.table) + " is not selected");
    if (f.word >= t.words) throw std::invalid_argument("corrupt_expected: word beyond the table");
    uploads_[t.upload]->flip(t.first + f.word, f.mask);
  }

  CuRun run(uint32_t seed, const typename P::Inject& inj) {
    return CuSession::run([&](int blocks) { launch(blocks, seed, inj); });
  }

  const hipFuncAttributes& attributes() const { return attr_; }

 private:
  void launch(int blocks, uint32_t seed, const typename P::Inject& j) {
    P::launch(stream(), blocks, uploads_, slices_ ? slices_->p : nullptr, out(), seed, j, groups_);
    HIP_OK(hipGetLastError());
  }

  uint32_t groups_;
  hipFuncAttributes attr_{};
  std::optional<DevBuf<uint8_t>> slices_;
  Uploads uploads_;
};

// cu_sweep_valu, cu_sweep_scalar and cu_sweep_mem.
template <class P>
py::dict part_binding(int dev, const std::vector<uint32_t>& mask, int rounds, uint32_t seed, const std::vector<std::string>& groups,
                      const py::object& inject, const py::object& corrupt_expected) {
  const uint32_t bits = P::names.bits(groups);
  const typename P::Inject inj = P::parse_inject(inject);
  const WordFlip flip = parse_flip(corrupt_expected, &P::names, nullptr, P::flip_usage);
  CuRun r;
  hipFuncAttributes attr{};
  {
    py::gil_scoped_release nogil;
    HIP_OK(hipSetDevice(dev));
    PartSession<P> session(dev, mask, rounds, bits);
    session.set_flip(flip);
    r = session.run(seed, inj);
    attr = session.attributes();
  }
  py::list recs;
  for (int b = 0; b < r.blocks; ++b) recs.append(P::record_tuple(r.words.data(), b));
  py::dict d;
  d["records"] = recs;
  const auto [names, checked] = P::names.names_and_checked(bits);
  d["groups"] = names;
  d["checked"] = checked;
  P::extras(d, attr);
  d["scratch_bytes"] = attr.localSizeBytes;
  d["ms"] = r.ms;
  return d;
}

// valu_sensitivity, scalar_sensitivity and mem_sensitivity.
template <class P>
py::dict part_sensitivity(int dev, const std::string& group, const std::vector<std::pair<uint32_t, uint32_t>>& flips,
                          const std::vector<uint32_t>& mask, int rounds, uint32_t seed) {
  constexpr size_t N = std::tuple_size<decltype(P::sensitivity_fields(nullptr, 0))>::value;
  const int g = P::names.index(group);
  if (flips.size() > 4096) throw std::invalid_argument(std::string(P::sensitivity_who) + ": at most 4096 words a call");
  Sensitivity r;
  {
    py::gil_scoped_release nogil;
    HIP_OK(hipSetDevice(dev));
    PartSession<P> session(dev, mask, rounds, P::sensitivity_groups(g));
    r = sensitivity<N>(
        session, seed, flips,
        [&](const std::pair<uint32_t, uint32_t>& f) { session.set_flip(WordFlip{g, f.first, f.second}); },
        [](const CuRun& run, int b) { return P::sensitivity_fields(run.words.data(), b); });
  }
  return sensitivity_dict(r, flips.size(), N, [](const uint32_t* f) {
    py::tuple t(N);
    for (size_t i = 0; i < N; ++i) t[i] = P::kSensitivityMinus1 >> i & 1u ? py::int_(or_minus1(f[i])) : py::int_(f[i]);
    return t;
  });
}

// The instantiation of P::group_kernel for group g of the sequence.
template <class P, int... G>
auto kernel_of(std::integer_sequence<int, G...>, int g) {
  static constexpr decltype(P::template group_kernel<0>) table[] = {P::template group_kernel<G>...};
  return table[g];
}

// One workgroup's raw words: `n` zeroed words that `launch(out)` has a kernel fill.
template <class Launch>
std::vector<uint32_t> one_workgroup_words(size_t n, Launch&& launch) {
  DevBuf<uint32_t> d(n);
  HIP_OK(hipMemset(d.p, 0, n * 4));
  launch(d.p);
  HIP_OK(hipGetLastError());
  std::vector<uint32_t> h(n);
  HIP_OK(hipMemcpy(h.data(), d.p, n * 4, hipMemcpyDeviceToHost));
  return h;
}

// Registers P's two bindings; the three parts share the argument lists.
template <class P>
void def_part(py::module_& m, const char* sweep_doc, const char* sensitivity_doc) {
  m.def(P::who, &part_binding<P>, py::arg("device") = 0, py::arg("cu_mask") = std::vector<uint32_t>{}, py::arg("rounds") = 4,
        py::arg("seed") = 0x5eed5eedu, py::arg("groups") = std::vector<std::string>{}, py::arg("inject") = py::none(),
        py::arg("corrupt_expected") = py::none(), sweep_doc);
  m.def(P::sensitivity_who, &part_sensitivity<P>, py::arg("device"), py::arg("group"), py::arg("flips"),
        py::arg("cu_mask") = std::vector<uint32_t>{}, py::arg("rounds") = 1, py::arg("seed") = 0x5eed5eedu, sensitivity_doc);
}

