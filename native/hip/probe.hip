// nanogpu._probe — MI355X (gfx950) calibration kernels for the node agent.
//
// The reference scheduler never touches a GPU; it trusts an external NVIDIA device plugin
// to realise "gpu-percent" (reference README.md:9, 30-34). On MI355X the agent realises a
// fractional grant spatially: a container with p% of a device gets a CU mask covering
// ceil(p/100 * CUs) compute units, XCD-aligned where possible (each XCD has its own 4 MiB
// L2, so a grant that owns whole XCDs keeps its L2 to itself). These kernels measure the
// facts that mapping needs, on the real device:
//   * cu_census   — which XCD / SE / CU each CU-mask bit enables (s_getreg XCC_ID, HW_ID);
//   * mfma_burn   — bf16 MFMA throughput of a masked stream (isolation check: TFLOP/s
//                   must scale with the CUs granted);
//   * hbm_copy    — streaming HBM3E bandwidth (16 B/lane, grid >> 256 WGs);
//                   these two rates, alone or co-located, are lists of Tenant behind one run_tenants;
//   * peer_bandwidth — per-pair xGMI rate: copy kernel pulling over peer access, and SDMA
//   * cu_sweep_kernel, hbm_fill / hbm_verify — the agent's deep self-test: every CU's MFMA
//                   pipes and LDS (`cu_sweep`), and free HBM against an address-derived pattern.
//   * matrix_tile_kernel, cu_sweep_kernel<kPaths> — the same sweep over the rest of the matrix
//                   unit (`cu_sweep_paths`): f16, fp8 / bf8, i8, block-scaled fp8 / fp6 / fp4,
//                   f32 and f64 MFMA.
//   * cu_valu_kernel, cu_scalar_kernel — the sweep's further parts on the same grid and stream: the
//                   vector ALU with the VGPR file (`cu_sweep_valu`), and the scalar ALU, scalar loads
//                   and the SGPR file (`cu_sweep_scalar`).
//   * cu_mem_kernel — and the CU's memory pipeline (`cu_sweep_mem`): global and buffer loads and
//                   stores, the L1, LDS instruction forms, the transposed read, LDS-DMA, atomics.
//   * xcd_write / read / ticket / atomic_kernel — a check of the device, not of a CU (`xcd_check`): what one
//                   XCD wrote, read on another, across a kernel boundary, by release, ticket and acquire
//                   inside one kernel, and by memory-side atomics from every XCD onto the same words.
#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cstdint>
#include <cstring>
#include <memory>
#include <new>
#include <optional>
#include <stdexcept>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "nanogpu/selftest_host.h"
#include "nanogpu/selftest_mem_host.h"
#include "nanogpu/selftest_paths_host.h"
#include "nanogpu/selftest_scalar_host.h"
#include "nanogpu/selftest_valu_host.h"
#include "nanogpu/selftest_xcd_host.h"

namespace py = pybind11;

#define HIP_OK(expr)                                                                    \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess)                                                               \
      throw std::runtime_error(std::string(#expr) + ": " + hipGetErrorString(e_));      \
  } while (0)

namespace {

namespace st = nanogpu::selftest;

// One translation unit, one file per part, each file its kernels and then its host code. The order
// is the order of dependency; the matrix_tile runner comes last because kernel templates are
// instantiated in the order in which host code first names them, and that is the order of the
// kernels in the code object.
#include "probe_calibration.inc"    // hbm_copy, cu_census, mfma_burn, mfma_tile; DevBuf, Stream, Events; Tenant
#include "probe_selftest_core.inc"  // NameTable, CuSession, PartSession and the part bindings, Sensitivity
#include "probe_sweep.inc"          // cu_sweep and cu_sweep_paths: the matrix unit and LDS
#include "probe_valu.inc"           // cu_sweep_valu
#include "probe_scalar.inc"         // cu_sweep_scalar
#include "probe_mem.inc"            // cu_sweep_mem
#include "probe_hbm.inc"            // hbm_fill, hbm_verify, hbm_pattern_check
#include "probe_xcd.inc"            // xcd_check: what one XCD wrote, read on another
#include "probe_matrix_tile.inc"    // matrix_tile: one instruction of a matrix path on the caller's codes

}  // namespace

PYBIND11_MODULE(_probe, m) {
  m.doc() = "MI355X calibration kernels (gfx950): CU census, MFMA burn, HBM and xGMI bandwidth";
  m.def("device_count", []() {
    int n = 0;
    HIP_OK(hipGetDeviceCount(&n));
    return n;
  });
  m.def("device_props", &device_props, py::arg("device") = 0);
  m.def("hbm_bandwidth", &hbm_bandwidth, py::arg("device") = 0, py::arg("bytes") = size_t(1) << 30,
        py::arg("iters") = 10, py::call_guard<py::gil_scoped_release>(),
        "Streaming copy bandwidth in GB/s (read + write bytes).");
  m.def("cu_census", &census, py::arg("device") = 0, py::arg("cu_mask") = std::vector<uint32_t>{},
        py::arg("blocks") = 2048, py::arg("sleep_iters") = 64,
        "Per-workgroup (xcc_id, hw_id) for a launch on a CU-masked stream.");
  m.def("mfma_throughput", &mfma_throughput, py::arg("device") = 0,
        py::arg("cu_mask") = std::vector<uint32_t>{}, py::arg("blocks") = 2048, py::arg("iters") = 2048,
        "bf16 MFMA TFLOP/s on a CU-masked stream.");
  m.def("gemm_tile", &gemm_tile, py::arg("a"), py::arg("b"),
        "C[32x32] = bf16(A[32x16]) @ bf16(B[16x32]) with one v_mfma_f32_32x32x16_bf16 (fp32 accumulate). The operands "
        "are lists of float32: a Python float that is no float32 value is rounded twice, double -> float32 -> bf16 "
        "(bf16_bits rounds the same way).");
  m.def(
      "bf16_bits",
      [](const py::object& x) {
        std::vector<uint16_t> out;
        if (py::isinstance<py::buffer>(x)) {   // float32 words as they lie in memory: no Python float in between
          const py::buffer_info info = x.cast<py::buffer>().request();
          if (info.itemsize != 4 || info.format != py::format_descriptor<float>::format() || info.ndim != 1 ||
              info.strides[0] != 4)
            throw std::invalid_argument("bf16_bits: a buffer must be one contiguous dimension of float32");
          out.resize(static_cast<size_t>(info.shape[0]));
          const char* p = static_cast<const char*>(info.ptr);
          for (size_t i = 0; i < out.size(); ++i) {
            float f;
            std::memcpy(&f, p + 4 * i, 4);
            out[i] = st::f32_to_bf16_bits(f);
          }
        } else {
          const std::vector<float> v = x.cast<std::vector<float>>();
          out.resize(v.size());
          for (size_t i = 0; i < v.size(); ++i) out[i] = st::f32_to_bf16_bits(v[i]);
        }
        return out;
      },
      py::arg("x"),
      "The bf16 codes gemm_tile gives its operands: float32 -> bf16, round to nearest even, NaN to a NaN of its sign. "
      "No GPU involved. x is a list of floats, or a one-dimensional contiguous float32 buffer (a numpy array), whose "
      "words are read as they are. In a list, a Python float that is no float32 value is rounded twice, double -> "
      "float32 -> bf16, and the conversion makes a signalling NaN quiet; pass a buffer for exact bit patterns.");
  m.def("mfma_burn_sums", &mfma_burn_sums, py::arg("device") = 0, py::arg("blocks") = 2, py::arg("iters") = 8,
        "Test hook: one launch of mfma_throughput's kernel in its checking form, which stores every thread's sum of its "
        "64 accumulators; [block][thread], 256 threads a block. blocks in 1..8 and iters in 1..1024, else ValueError.");
  m.def(
      "copy_check",
      [](int dev, size_t n_floats, size_t guard_bytes) -> py::object {
        CopyCheck r;
        {
          py::gil_scoped_release nogil;
          r = copy_check(dev, n_floats, guard_bytes);
        }
        if (guard_bytes == 0) return py::bool_(r.ok);
        py::dict d;
        d["ok"] = r.ok;
        d["guards_ok"] = r.guard_changed == 0;
        d["guard_bytes_changed"] = r.guard_changed;
        return d;
      },
      py::arg("device") = 0, py::arg("n_floats") = size_t(1) << 24, py::arg("guard_bytes") = size_t(0),
      "hbm_copy kernel result == source, bit for bit. Test hook: guard_bytes > 0 (a multiple of 16) puts the "
      "destination between two guard regions of that size and returns {ok, guards_ok, guard_bytes_changed} "
      "instead of the bool: guards_ok is false when the kernel wrote outside the destination.");
  m.def("mixed_colocated", &mixed_colocated, py::arg("device"), py::arg("hbm_mask"), py::arg("mfma_mask"),
        py::arg("bytes") = size_t(1) << 30, py::arg("iters") = 10, py::arg("mfma_blocks") = 1536,
        py::arg("mfma_iters") = 4096, py::call_guard<py::gil_scoped_release>(),
        "{copy GB/s, MFMA TFLOP/s} for a streaming tenant beside a compute-bound one.");
  m.def("hbm_colocated", &hbm_colocated, py::arg("device"), py::arg("cu_masks"), py::arg("bytes") = size_t(1) << 30,
        py::arg("iters") = 10, py::arg("iters_each") = std::vector<int>{}, py::call_guard<py::gil_scoped_release>(),
        "Per-tenant HBM copy GB/s for concurrent tenants on CU-masked streams.");
  m.def("mfma_colocated", &mfma_colocated, py::arg("device"), py::arg("cu_masks"), py::arg("blocks"),
        py::arg("iters") = 2048, py::call_guard<py::gil_scoped_release>(),
        "Concurrent MFMA burns on CU-masked streams; per-stream TFLOP/s.");
  m.def(
      "peer_bandwidth",
      [](int src, int dst, size_t bytes, int iters, double deadline_s) {
        PeerRate r;
        {
          py::gil_scoped_release nogil;
          r = peer_bandwidth(src, dst, bytes, iters, deadline_s);
        }
        py::dict d;
        d["pull_gbs"] = r.pull_gbs;
        d["dma_gbs"] = r.dma_gbs;
        d["peer_access"] = r.peer_access;
        d["gbs"] = std::max(r.pull_gbs, r.dma_gbs);
        return d;
      },
      py::arg("src"), py::arg("dst"), py::arg("bytes") = size_t(256) << 20, py::arg("iters") = 10,
      py::arg("deadline_s") = 30.0,
      "One-direction xGMI rate src -> dst in GB/s: copy kernel pulling over peer access, and SDMA. "
      "Raises TimeoutError when the transfers do not finish within deadline_s (the work is abandoned).");
  py::register_exception<PeerTimeout>(m, "PeerTimeout", PyExc_TimeoutError);
  m.def(
      "cu_sweep",
      [](int dev, const std::vector<uint32_t>& mask, int rounds, uint32_t seed, const py::object& inject,
         const py::object& corrupt_expected, std::optional<size_t> lds_bytes) {
        return sweep_binding(dev, mask, rounds, seed, nullptr, inject, corrupt_expected, lds_bytes);
      },
      py::arg("device") = 0, py::arg("cu_mask") = std::vector<uint32_t>{}, py::arg("rounds") = 4,
      py::arg("seed") = 0x5eed5eedu, py::arg("inject") = py::none(), py::arg("corrupt_expected") = py::none(),
      py::arg("lds_bytes") = py::none(),
      "Deep CU check on a CU-masked stream: rounds x CUs workgroups, each holding a CU's whole LDS, run an "
      "exact bf16 MFMA chain on all 4 waves and a pattern test of the LDS. Records are (xcc, hw_id, fail bits, "
      "SIMD ids seen, first bad LDS dword or -1). inject = (xcc, cu_key, 'mfma' | 'lds'[, lds dword]) flips one "
      "bit of that CU's own data (tests). Test hook: corrupt_expected = (word, xor) XORs word 0..1023 of the host's "
      "expected bf16 tile in the upload, so every wave of every visit must report the MFMA check failed. Test hook: "
      "lds_bytes (a multiple of 16, 16..65536) runs the dynamic-LDS kernel with that much LDS instead of the one a "
      "device without room for a whole-LDS block would get; several such workgroups share a CU, so a visit of "
      "every CU is not promised in this mode.");
  m.def(
      "matrix_tile",
      [](const std::string& path, const std::vector<uint64_t>& a, const std::vector<uint64_t>& b,
         const std::vector<uint32_t>& scale_a, const std::vector<uint32_t>& scale_b, std::pair<int, int> opsel) {
        const int p = kPathNames.index(path);
        const std::vector<uint32_t> w = matrix_tile(p, a, b, scale_a, scale_b, opsel.first, opsel.second);
        py::list c;
        const size_t n = static_cast<size_t>(sp::path_dim(p)) * sp::path_dim(p);
        for (size_t i = 0; i < n; ++i) {
          if (p == sp::kI8) {
            c.append(static_cast<int32_t>(w[i]));
          } else if (p == sp::kF64) {
            const uint64_t bits = (static_cast<uint64_t>(w[2 * i + 1]) << 32) | w[2 * i];
            double v;
            std::memcpy(&v, &bits, 8);
            c.append(v);
          } else {
            float v;
            std::memcpy(&v, &w[i], 4);
            c.append(v);
          }
        }
        return c;
      },
      py::arg("path"), py::arg("a_codes"), py::arg("b_codes"), py::arg("scale_a") = std::vector<uint32_t>{},
      py::arg("scale_b") = std::vector<uint32_t>{}, py::arg("opsel") = std::pair<int, int>{0, 0},
      "One MFMA instruction of `path` (f16, fp8, bf8, i8, mxfp8, mxfp6, mxfp4, f32, f64) on operand codes: "
      "a_codes = A[row][k] and b_codes = B[k][col] bit patterns, row-major; on the scaled paths scale_a = "
      "[row][k block] and scale_b = [k block][col] E8M0 codes, carried in byte opsel = (a, b) of the scale "
      "register. Returns C row-major: floats, ints for i8, doubles (16x16) for f64.");
  m.def(
      "cu_sweep_paths",
      [](int dev, const std::vector<uint32_t>& mask, int rounds, uint32_t seed, const std::vector<std::string>& paths,
         const py::object& inject, const py::object& corrupt_expected, std::optional<size_t> lds_bytes) {
        return sweep_binding(dev, mask, rounds, seed, &paths, inject, corrupt_expected, lds_bytes);
      },
      py::arg("device") = 0, py::arg("cu_mask") = std::vector<uint32_t>{}, py::arg("rounds") = 4,
      py::arg("seed") = 0x5eed5eedu, py::arg("paths") = std::vector<std::string>{}, py::arg("inject") = py::none(),
      py::arg("corrupt_expected") = py::none(), py::arg("lds_bytes") = py::none(),
      "cu_sweep whose visits also run, on all 4 waves, an exact chain of 8 MFMA instructions of every path in "
      "`paths` and compare every accumulator bit with the host's tile. Records are cu_sweep's 5 fields plus "
      "(failed-path bits, waves that saw a path fail); `paths` in the result names the bits in order, `checked` "
      "the paths that ran. inject = (xcc, cu_key, path name) flips one accumulator bit of that path on that CU (tests). "
      "Test hook: corrupt_expected = ('bf16' | path name, word, xor) XORs one word of that expected tile (1024 "
      "words, f64 512) in this call's upload, never in the host's cached tiles; the path must be selected. Test hook: "
      "lds_bytes as in cu_sweep, 36864 (the nine staged tiles)..65536; a visit of every CU is not promised then.");
  m.def(
      "sweep_sensitivity",
      &sweep_sensitivity,
      py::arg("device"), py::arg("tile"), py::arg("flips"), py::arg("paths") = std::vector<std::string>{},
      py::arg("cu_mask") = std::vector<uint32_t>{}, py::arg("rounds") = 1, py::arg("seed") = 0x5eed5eedu,
      "Test hook: for every (word, xor) of `flips` one sweep (cu_sweep_paths over `paths`, or cu_sweep when "
      "`paths` is empty) with that word of expected tile `tile` ('bf16' or a path name) corrupted as by "
      "corrupt_expected, all on one set of buffers. words[i] = (AND, OR) over that sweep's records of (fail bits, "
      "lds_bad or -1, failed-path bits, path waves); records = workgroups per sweep, seconds = the loop's wall time.");
  m.def(
      "hbm_pattern_check",
      [](int dev, size_t bytes, uint32_t seed, int passes, const std::vector<std::pair<uint64_t, uint32_t>>& corrupt,
         const py::object& verify_seed, size_t guard_bytes, long long fill_launch_blocks,
         long long verify_launch_blocks, const std::vector<uint32_t>& cu_mask) {
        const int64_t vseed = verify_seed.is_none() ? int64_t(-1) : int64_t(verify_seed.cast<uint32_t>());
        PatternResult r;
        {
          py::gil_scoped_release nogil;
          r = hbm_pattern_check(dev, bytes, seed, passes, corrupt, vseed, guard_bytes, fill_launch_blocks,
                                verify_launch_blocks, cu_mask);
        }
        py::list first;
        for (const st::Mismatch& mm : r.first)
          first.append(py::make_tuple(st::mismatch_byte_offset(mm), mm.expected, mm.got));
        py::dict d;
        d["bytes"] = r.bytes;
        d["errors"] = r.errors;
        d["first"] = first;
        d["fill_gbs"] = r.fill_gbs;
        d["verify_gbs"] = r.verify_gbs;
        d["fill_launches"] = r.fill_launches;
        d["verify_launches"] = r.verify_launches;
        if (guard_bytes) d["guard_ok"] = r.guard_changed == 0;
        return d;
      },
      py::arg("device") = 0, py::arg("bytes") = size_t(256) << 20, py::arg("seed") = 0x5eed5eedu,
      py::arg("passes") = 2, py::arg("corrupt") = std::vector<std::pair<uint64_t, uint32_t>>{},
      py::arg("verify_seed") = py::none(), py::arg("guard_bytes") = size_t(0), py::arg("fill_launch_blocks") = 0LL,
      py::arg("verify_launch_blocks") = 0LL, py::arg("cu_mask") = std::vector<uint32_t>{},
      "Fills `bytes` of device memory with an address-derived pattern and verifies it (odd passes: the "
      "complement). errors counts mismatching 16-byte elements over all passes; first = up to 16 of "
      "(byte offset of the first differing byte, expected word, got word). corrupt = [(byte offset, xor byte)] "
      "is applied by the host between fill and verify. Test hook: guard_bytes > 0 (a multiple of 16) puts the "
      "buffer between two guard regions of that size and adds guard_ok, false when a guard byte changed: a kernel "
      "wrote outside the buffer, or `corrupt` named an offset in the guard behind it (bytes <= offset < bytes + guard_bytes). A pass is one launch after another of at most 2^22 blocks (64 GiB), "
      "each below the 2^32 work-items HIP supports; fill_launches / verify_launches count them per pass. Test hook: "
      "fill_launch_blocks / verify_launch_blocks = blocks of 1,024 elements a launch of the fill / of the verify "
      "(0: 2^22; 1..2^22; anything else raises ValueError). cu_mask = 32-bit words of a CU mask (as cu_sweep's): the fill, "
      "the verify and the clearing of their result run on a stream masked to those CUs; empty: an unmasked stream, "
      "every CU. Raises MemoryError when the buffer cannot be allocated.");
  def_part<ValuPart>(
      m,
      "Vector-ALU part of the deep CU check, on cu_sweep's grid and stream: all 4 waves of every visit run the exact "
      "chains of the selected groups (fma32, fma64, pkfma16, pkfma32, addmul32, int32, int64, bits, dot, cvt, xlane) "
      "against the host's table, 'approx' (exp2, log2, rcp, rsq, sqrt within 8 ulp of libm, and one hash per wave) and "
      "'regs' (a pattern test of reg_slots vector registers a lane, twice). Records are (xcc, hw_id, fail bits: 0..3 exact "
      "groups, 4..7 registers, 8..11 approx bound, 12..15 approx hash unlike wave 0's, by wave; SIMD ids seen; failed-group "
      "bits; first bad slot or -1; its thread (wave << 6 | lane) or -1; wave 0's approx hash). `groups` in the result names "
      "the bits, `checked` what ran; regs_per_lane and scratch_bytes are the kernel's attributes as the runtime reports "
      "them ('regs' raises when scratch_bytes is not 0). inject = (xcc, cu_key, 'valu', group) | (xcc, cu_key, 'regs', slot) "
      "| (xcc, cu_key, 'approx') flips one bit of that CU's wave 0, lane 0 (tests): of the group's result, of one approx "
      "output, or of the value held slot `slot` is compared with (the held register is not written: that would cost "
      "the registers under test; the reported slot, wave and lane are the same). Test hook: corrupt_expected = (group, "
      "word 0..127, xor) XORs one word of that group's expected words in this call's upload only.",
      "Test hook: for every (word, xor) of `flips` one cu_sweep_valu over every exact group with that word of `group`'s "
      "expected words corrupted, all on one session. words[i] = (AND, OR) over that sweep's records of (fail bits, "
      "failed-group bits); records = workgroups per sweep, seconds = the loop's wall time.");
  m.def(
      "valu_lanes",
      [](const std::string& group) -> py::object {
        const int g = ValuPart::names.index(group);
        const std::vector<uint32_t> w = valu_lanes(g);
        py::list out;
        for (uint32_t v : w) {
          if (g == sv::kApprox) out.append(sv::bits_float(v));
          else out.append(v);
        }
        return out;
      },
      py::arg("group"),
      "One wave runs group `group`: the 128 words [lane][2] of an exact group, or for 'approx' the 320 floats [op][lane] "
      "of exp2, log2, rcp, rsq, sqrt.");
  def_part<ScalarPart>(
      m,
      "Scalar part of the deep CU check, on cu_sweep's grid and stream: all 4 waves of every visit run the exact chains "
      "of the selected groups (add, mul, shift, logic, bits, cmp: one asm statement per scalar-ALU instruction; vcc: the "
      "vector / scalar boundary) against the host's table of 224 words, 'smem' (scalar loads of every width from a "
      "read-only table of 4096 words, wave w its quarter) and 'sregs' (a pattern test of sreg_slots named scalar "
      "registers a wave, twice). Records are (xcc, hw_id, fail bits: 0..3 exact groups, 4..7 smem, 8..11 sregs, by wave; "
      "SIMD ids seen; failed-group bits; first bad register slot, else first bad table word, or -1; its wave or -1; 0 for "
      "a slot, 1 for a word, or -1). `groups` in the result names the bits, `checked` what ran; num_regs and scratch_bytes "
      "are the kernel's attributes as the runtime reports them (it has no count of scalar registers; 'sregs' raises when scratch_bytes is not 0). inject = "
      "(xcc, cu_key, 'scalar', group) | (xcc, cu_key, 'smem', word) | (xcc, cu_key, 'sregs', slot) flips bit 0 on that CU "
      "(tests): of the group's first result word on wave 0, of the value table word `word` is compared with (on the wave "
      "that reads it: word // 1024), or of the value slot `slot` is compared with in pass 0 on wave 0 (the held "
      "register is not written). Test hook: corrupt_expected = (group, word 0..31, xor) | ('smem', word 0..4095, xor) "
      "XORs one word of that table in this call's upload only.",
      "Test hook: for every (word, xor) of `flips` one cu_sweep_scalar over every exact group and 'smem' with that word "
      "of `group`'s expected words (or, for 'smem', of the load table) corrupted, all on one session. words[i] = (AND, "
      "OR) over that sweep's records of (fail bits, failed-group bits, first bad index or -1); records = workgroups per "
      "sweep, seconds = the loop's wall time.");
  m.def(
      "scalar_words",
      [](const std::string& group) { return scalar_words(ScalarPart::names.index(group)); },
      py::arg("group"), "One workgroup of four waves runs exact scalar group `group`: its 32 words [wave][8].");
  def_part<MemPart>(
      m,
      "Memory part of the deep CU check, on cu_sweep's grid and stream: all 4 waves of every visit run the selected groups "
      "(gload, l1, gstore, buffer, lds, ldstr, ldsdma, atomic: nanogpu/selftest_mem_host.h lists each one's instructions) on a "
      "read-only table of table_words words, on their quarter of the workgroup's slice_bytes of scratch memory and on LDS, and "
      "compare every result word with the value computed from its index. `seed` is accepted and not used: the part's data are "
      "fixed. Records are (xcc, hw_id, fail bits: bit w is wave w; SIMD ids seen; failed-group bits; first bad group, its lowest "
      "bad index and that index's wave, or -1). The index of a result word is k * 64 + lane, in l1 the table word. `groups` in "
      "the result names the bits, `checked` what ran; num_regs and scratch_bytes are the kernel's attributes as the runtime "
      "reports them. inject = (xcc, cu_key, group, index) flips bit 0 of the value that index is compared with on that CU, on "
      "wave index % 4 (tests; no held data is touched). Test hook: corrupt_expected = ('gload' | 'l1' | 'ldsdma', word 0..8191, "
      "xor) XORs one word of the table in this call's upload only.",
      "Test hook: for every (word, xor) of `flips` one cu_sweep_mem of `group` (gload, l1 or ldsdma) alone with that word of the "
      "table corrupted, all on one session. words[i] = (AND, OR) over that sweep's records of (fail bits, failed-group bits, "
      "first bad group or -1, its lowest bad index or -1); records = workgroups per sweep, seconds = the loop's wall time.");
  m.def(
      "mem_lanes",
      [](const std::string& group) { return mem_lanes(MemPart::names.index(group)); },
      py::arg("group"), py::call_guard<py::gil_scoped_release>(),
      "One workgroup of four waves runs memory group `group`: every lane's raw result words [wave][k][lane].");
  m.def("xcd_check", &xcd_check, py::arg("device") = 0, py::arg("cu_mask") = std::vector<uint32_t>{}, py::arg("rounds") = 4,
        py::arg("seed") = 0x5eed5eedu, py::arg("groups") = std::vector<std::string>{"handoff", "ticket", "atomic"},
        py::arg("inject") = py::none(), py::arg("corrupt") = py::none(),
        "Check of the device on cu_sweep's grid and stream (rounds 1..4 x CUs workgroups, N of them): data one XCD wrote, read on "
        "another. Groups: 'handoff' (a write kernel fills 16 KiB a workgroup with plain stores and enters it in its XCD's list; the "
        "next launch verifies from every XCD one slice of every XCD), 'ticket' (workgroups 8g..8g+7: plain stores, agent-scope "
        "release, one ticket; the last arriver acquires and verifies the others' 4 KiB slices, which it had read before) and "
        "'atomic' (adds, or, xor, min, max and a counter from every workgroup onto the same words). No kernel waits for another "
        "workgroup. records[b] = (write, read, ticket, atomic) sections of workgroup b of each kernel, None where the kernel did not "
        "run: write (xcc, hw_id, kinds, list position); read (xcc, hw_id, kinds, writer XCDs verified, writer XCDs failed, reader "
        "ordinal, then the first failure: writer block, its xcc, its hw_id, word, expected, observed, each None without one); ticket "
        "(xcc, hw_id, kinds, last arriver, ticket, slices verified, writer XCDs verified, failed, the first failure, fold of the words "
        "read before the ticket); atomic (xcc, hw_id, kinds, duplicates). kinds: bit 0 data, 1 dir (an index read from memory was out "
        "of range: never used as an address), 2 writer, 3 preread, 4 dup. atomic_words / atomic_expected are the 168 final words and "
        "the host's, atomic_bad the indices that differ; pairs[group] the ordered (writer xcc, reader xcc) verified; bytes the device "
        "memory held; ms_kernels and ms the time per kernel and of the sequence; num_regs per kernel and the largest scratch_bytes. "
        "Test hooks: inject = ('handoff', writer xcc, reader xcc) | ('ticket', group) flips bit 0 of the value word 0 is compared with "
        "(of that XCD's slices on that XCD's readers; of the first partner's slice on that group's last arriver), ('atomic', word) "
        "flips bit 0 of the host's expected word; corrupt = (block, byte offset, xor byte): the host XORs one byte of that block's "
        "hand-off slice between the write and the read kernel, the one synchronisation inside a run.");
  m.def("xcd_sensitivity", &xcd_sensitivity, py::arg("device"), py::arg("flips"), py::arg("cu_mask") = std::vector<uint32_t>{},
        py::arg("rounds") = 1, py::arg("seed") = 0x5eed5eedu,
        "Test hook: for every (word, xor) of `flips` one hand-off on one session with that word of block 0's slice XORed between the "
        "write and the read kernel. words[i] = (AND, OR) over that run's read sections of (kinds, writer XCDs failed, first bad "
        "block or -1, its word or -1); records = workgroups per run, seconds = the loop's wall time.");
  m.def(
      "mem_info",
      [](int dev) {
        size_t free_b = 0, total_b = 0;
        HIP_OK(hipSetDevice(dev));
        HIP_OK(hipMemGetInfo(&free_b, &total_b));
        return py::make_tuple(free_b, total_b);
      },
      py::arg("device") = 0, "(free bytes, total bytes) of the device's memory.");
}
