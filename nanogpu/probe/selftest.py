"""Deep GPU self-test: every CU's MFMA pipes and LDS, and free HBM with an address pattern.

The basic self-test (agent.node.gpu_selftest) runs one wave on one CU and copies 16 MiB. This
one drives the probe's `cu_sweep` and `hbm_pattern_check` (native/hip/probe.hip):

* `cu_sweep` launches rounds x CUs workgroups that each hold a CU's whole LDS (so at most one
  is resident per CU and the dispatcher spreads them), run an exact bf16 MFMA chain on all 4
  waves and pattern-test the LDS. `fold_sweep` folds the per-workgroup records by CU identity
  `(xcc, (hw_id >> 8) & 0xFF)`. A CU that no workgroup reached is a coverage shortfall, not a
  failure: `deep_selftest` re-launches with doubled rounds (3 launches at most), then reports
  how many CUs it could not reach.
* `hbm_pattern_check` fills a buffer with words that are a function of their address and
  verifies it, then does the same with the complement. `pattern_word` / `pattern_at` are the
  host twin of that pattern, so a report (or a test) can state the expected value anywhere.

* `cu_sweep_paths` is `cu_sweep` with, in every visit, an exact chain of 8 instructions of each
  selected matrix path (`PATHS`: f16, fp8, bf8, i8, block-scaled mxfp8 / mxfp6 / mxfp4, f32,
  f64) on all 4 waves, every accumulator compared bit for bit with a host tile. The operand
  data is generated as codes and decoded on the host; the decoders, generators and expected
  tiles below are the Python twin of native/include/nanogpu/selftest_paths_host.h, which
  states the exactness argument. `fold_paths` reports per CU which paths failed.

* `cu_sweep_valu` and `cu_sweep_scalar` are further launches on the same mask after each sweep launch: the
  vector ALU, transcendentals and VGPR file (`selftest_valu.py`), and the scalar ALU, the vector / scalar boundary,
  scalar loads and the SGPR file (`selftest_scalar.py`). Each has its own records, folded by CU like the sweep's.

What it does not cover: HBM pages and CUs held by tenants (the agent sweeps only free units
and checks HBM only on devices without a grant), the contents of L2 / Infinity Cache, and of
the matrix unit the 16x16 shapes, the sparse (smfmac) forms, bf6 operands, mixed A / B formats
and Inf and NaN operands. Zero, subnormal and largest-normal operands and E8M0 scales other than
127 and 128 are outside the sweep's generators: `edge_tiles` puts them through `matrix_tile`, one
wave on one CU, in the GPU tests only.

`localise_failure` turns a failing sweep into CU-mask units (agent.cumask: one CU per XCD): it
runs `deep_selftest` once per candidate unit, masked to it, and says which units fail again and
which failing CUs no such unit explains. The agent fences those units (`--selftest-fence`)
instead of failing the device when `fenceable` allows it.

`python -m nanogpu.probe.selftest [--device N] [--hbm-mib M] [--paths all|LIST] [--valu all|LIST] [--scalar all|LIST] [--json]`
prints one report;
with `--fence N` it also prints the units (at most N) an agent would fence, and changes nothing.
"""
from __future__ import annotations

import logging
import time
from dataclasses import asdict, dataclass, field
from functools import reduce
from operator import or_

log = logging.getLogger(__name__)

M32 = 0xFFFFFFFF
HI_MUL = 0x9E3779B1
FAIL_LDS = 1 << 4            # fail bits 0..3: the MFMA check of wave 0..3
HBM_HEADROOM = 2 << 30       # left free by the "all free HBM" check
MAX_LAUNCHES = 3


def mix32(x: int) -> int:
    """The fixed 32-bit finaliser both kernels use (murmur3's)."""
    x &= M32
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    x ^= x >> 16
    return x


def pattern_word(index: int, k: int, seed: int, pass_: int = 0) -> int:
    """Word k (0..3) of 16-byte element `index` in pass `pass_`: with w = 4 index + k the
    64-bit word index, mix32(lo32(w) ^ seed) ^ hi32(w) * HI_MUL; odd passes hold the complement."""
    w = 4 * index + k
    v = mix32((w & M32) ^ (seed & M32)) ^ (((w >> 32) * HI_MUL) & M32)
    return v ^ M32 if pass_ & 1 else v


def pattern_at(byte_offset: int, seed: int, pass_: int = 0) -> int:
    """The 32-bit word that holds `byte_offset` (little-endian: byte b is bits 8b..8b+7)."""
    return pattern_word(byte_offset // 16, (byte_offset % 16) // 4, seed, pass_)


def cu_key(hw_id: int) -> int:
    """CU / SH / SE bits of HW_ID: with the XCC id, a CU's identity on the chip."""
    return (hw_id >> 8) & 0xFF


def fail_kinds(fail_bits: int) -> list[str]:
    kinds = []
    if fail_bits & 0xF:
        kinds.append("mfma")
    if fail_bits & FAIL_LDS:
        kinds.append("lds")
    if fail_bits & ~0x1F:
        kinds.append("record")
    return kinds


def _coverage(seen, expected_cus) -> tuple[int, list, int]:
    """(n_expected, uncovered, n_uncovered) of the CU keys in `seen` against `expected_cus`: a set
    of `(xcc, cu_key)`, or only their number (then `uncovered` cannot be listed and is empty)."""
    if isinstance(expected_cus, int):
        return expected_cus, [], max(0, expected_cus - len(seen))
    expected = {tuple(k) for k in expected_cus}
    uncovered = sorted(expected - set(seen))
    return len(expected), uncovered, len(uncovered)


def _by_cu(records) -> dict[tuple[int, int], list[list]]:
    """Records that begin `(xcc, hw_id, ...)`, grouped: `{(xcc, cu_key): [a visit's other fields, ...]}`."""
    by_cu: dict[tuple[int, int], list[list]] = {}
    for xcc, hw_id, *rest in records:
        by_cu.setdefault((xcc, cu_key(hw_id)), []).append(rest)
    return by_cu


def _or(values) -> int:
    return reduce(or_, values, 0)


def _simds_seen_min(by_cu, field: int) -> int:
    return min((bin(_or(v[field] for v in visits)).count("1") for visits in by_cu.values()), default=0)


def _named_failures(by_cu, expected_cus, failures) -> dict:
    """The report of a fold whose failures have names. `failures` holds, per failed CU in key
    order, `(key, the names it failed, what its entry of "cus" adds to xcc and cu_key)`."""
    n_expected, uncovered, n_uncovered = _coverage(by_cu, expected_cus)
    failed: dict[str, list[list[int]]] = {}
    cus = []
    for (xcc, key), names, entry in failures:
        cus.append({"xcc": xcc, "cu_key": key, **entry})
        for n in names:
            failed.setdefault(n, []).append([xcc, key])
    return {"cus_seen": len(by_cu), "cus_expected": n_expected, "failed": failed, "cus": cus,
            "uncovered": [list(k) for k in uncovered], "cus_uncovered": n_uncovered}


def fold_sweep(records, expected_cus) -> dict:
    """Folds `cu_sweep` records `(xcc, hw_id, fail_bits, simds, lds_bad_off)` by CU.

    `expected_cus` is the set of `(xcc, cu_key)` the sweep should reach, or, where the keys
    are not known in advance, their number. `uncovered` lists the expected keys no record came
    from (empty when only the number is known; `cus_uncovered` counts them either way). A CU is
    failed when any of its visits failed; `simds_seen_min` is the smallest number of distinct
    SIMDs any CU's waves reported."""
    by_cu = _by_cu(records)
    n_expected, uncovered, n_uncovered = _coverage(by_cu, expected_cus)
    per_xcd: dict[int, int] = {}
    for xcc, _ in by_cu:
        per_xcd[xcc] = per_xcd.get(xcc, 0) + 1
    failed = []
    for k, visits in sorted(by_cu.items()):
        fail = _or(fail for fail, _simds, _bad in visits)
        if fail:
            failed.append({"xcc": k[0], "cu_key": k[1], "kinds": fail_kinds(fail),
                           "lds_bad_off": min((bad for _fail, _simds, bad in visits if bad >= 0), default=-1)})
    return {"cus_seen": len(by_cu), "cus_expected": n_expected, "per_xcd": dict(sorted(per_xcd.items())),
            "failed": failed, "uncovered": [list(k) for k in uncovered], "cus_uncovered": n_uncovered,
            "simds_seen_min": _simds_seen_min(by_cu, 1)}


# ---- matrix paths: the Python twin of native/include/nanogpu/selftest_paths_host.h -------------

PATHS = ("f16", "fp8", "bf8", "i8", "mxfp8", "mxfp6", "mxfp4", "f32", "f64")   # bit order of the records
PATH_STEPS = 8
PATH_K = {"f16": 16, "fp8": 16, "bf8": 16, "i8": 32, "mxfp8": 64, "mxfp6": 64, "mxfp4": 64, "f32": 2, "f64": 4}
PATH_CODE_BITS = {"f16": 16, "fp8": 8, "bf8": 8, "i8": 8, "mxfp8": 8, "mxfp6": 6, "mxfp4": 4, "f32": 32, "f64": 64}
PATH_FORMAT = {"f16": (5, 10, 15), "fp8": (4, 3, 7), "bf8": (5, 2, 15), "i8": (0, 8, 0), "mxfp8": (4, 3, 7),
               "mxfp6": (2, 3, 1), "mxfp4": (2, 1, 1), "f32": (8, 23, 127), "f64": (11, 52, 1023)}   # ebits, mbits, bias
PATH_EXP_WINDOW = {"fp8": (5, 6, 7, 8), "bf8": (14, 15, 16, 17), "mxfp8": (7, 8), "mxfp6": (0, 1, 2, 3),
                   "mxfp4": (0, 1, 2, 3), "f16": (8, 9, 10, 11, 15, 16), "f32": (120, 121, 122, 123, 127, 128),
                   "f64": (1016, 1017, 1018, 1019, 1023, 1024)}
PATH_LIMIT_BITS = {"i8": 31, "f64": 53}     # the others accumulate in fp32: 24
SCALED_PATHS = ("mxfp8", "mxfp6", "mxfp4")
SCALE_WINDOW = (127, 128)


def _parse_names(spec, known, noun: str) -> list[str]:
    """None / "" / [] -> [], "all" -> every name of `known`, "a,b" or a list of names -> those,
    in bit order. Raises ValueError on an unknown name."""
    if not spec:
        return []
    names = list(known) if spec == "all" else [n.strip() for n in spec.split(",")] if isinstance(spec, str) else list(spec)
    bad = [n for n in names if n not in known]
    if bad or not names:
        raise ValueError(f"unknown {noun}(s) {bad}: choose from {', '.join(known)} or 'all'")
    return [n for n in known if n in names]


def parse_paths(spec) -> list[str]:
    """`_parse_names` over `PATHS`: None / "" -> [], "all", "a,b" or a list of names; ValueError on an unknown one."""
    return _parse_names(spec, PATHS, "matrix path")


def path_dim(path: str) -> int:
    return 16 if path == "f64" else 32


def decode_minifloat(code: int, ebits: int, mbits: int, bias: int) -> tuple[int, int]:
    """(sig, exp) with value = sig * 2^exp of a finite sign / exponent / mantissa code; exponent
    field 0 is subnormal. Special exponents are the caller's."""
    m = code & ((1 << mbits) - 1)
    e = (code >> mbits) & ((1 << ebits) - 1)
    sig = ((1 << mbits) + m) if e else m
    return (-sig if (code >> (ebits + mbits)) & 1 else sig), (e if e else 1) - bias - mbits


def _value(sig: int, exp: int, negative_zero: bool) -> float:
    import math

    return -0.0 if negative_zero and sig == 0 else math.ldexp(sig, exp)


def decode_e4m3fn(c: int) -> float:
    """OCP e4m3fn: no Inf, S.1111.111 is NaN, largest 448."""
    if c & 0x7F == 0x7F:
        return float("nan")
    return _value(*decode_minifloat(c, 4, 3, 7), bool(c & 0x80))


def decode_e5m2(c: int) -> float:
    """OCP e5m2: exponent field 31 is Inf (mantissa 0) or NaN."""
    if (c >> 2) & 0x1F == 0x1F:
        return float("nan") if c & 3 else float("-inf") if c & 0x80 else float("inf")
    return _value(*decode_minifloat(c, 5, 2, 15), bool(c & 0x80))


def decode_e2m3(c: int) -> float:
    return _value(*decode_minifloat(c & 0x3F, 2, 3, 1), bool(c & 0x20))


def decode_e2m1(c: int) -> float:
    return _value(*decode_minifloat(c & 0xF, 2, 1, 1), bool(c & 0x8))


def decode_e8m0(c: int) -> float:
    import math

    return float("nan") if c == 0xFF else math.ldexp(1.0, c - 127)


def path_decode(path: str, code: int) -> tuple[int, int]:
    """(sig, exp) of one operand code of `path`."""
    if path == "i8":
        c = code & 0xFF
        return (c - 256 if c & 0x80 else c), 0
    return decode_minifloat(code, *PATH_FORMAT[path])


def _rotl32(x: int, r: int) -> int:
    r &= 31
    return ((x << r) | (x >> (32 - r))) & M32


def path_step_hash(path: str, op: int, s: int, idx: int) -> int:
    """One mix32 per (path, op, idx), varied by step with three operations: the generator runs
    on every wave of every visit, so it is cheap on purpose."""
    base = mix32(0x9E3779B9 ^ (PATHS.index(path) << 27) ^ (op << 26) ^ (idx << 8))
    return ((base ^ (base >> (s + 3))) + s * 0x9E3779B9) & M32


def path_hash(path: str, op: int, s: int, idx: int, d: int) -> int:
    """The hash behind dword d (0..15) of a row / column: one rotation of the step's hash."""
    return _rotl32(path_step_hash(path, op, s, idx), 7 * d + 3)


def wide_code(bits: int, mbits: int, bias: int, op: int, s: int, idx: int, k: int, hv: int) -> int:
    """f16 / f32 / f64: one FINE value ([2, 3), the mantissa below its top bit hashed) per
    accumulator, times +-1; everything else COARSE (2^-7..2^-4 x 1.xxx)."""
    sign = hv & (1 << (bits - 1))
    coarse = sign | ((bias - 7 + ((hv >> mbits) & 3)) << mbits) | (hv & (7 << (mbits - 3)))
    if k != 0 or s > 1:
        return coarse
    fine = sign | ((bias + 1) << mbits) | (hv & ((1 << (mbits - 1)) - 1))
    one = sign | (bias << mbits)
    if s == 0:
        return (coarse if idx & 1 else fine) if op == 0 else one
    return (one if idx & 1 else 0) if op == 0 else fine


def path_dword(path: str, op: int, s: int, idx: int, d: int) -> int:
    """Dword d of the packed operand row / column, as the kernel holds it."""
    if path == "f64":
        k = d >> 1
        hv = (path_hash(path, op, s, idx, 2 * k + 1) << 32) | path_hash(path, op, s, idx, 2 * k)
        return (wide_code(64, 52, 1023, op, s, idx, k, hv) >> (32 * (d & 1))) & M32
    h = path_hash(path, op, s, idx, d)
    if path == "fp8":
        return 0x28282828 + (h & 0x9F9F9F9F)
    if path in ("bf8", "mxfp8"):
        return 0x38383838 + (h & 0x8F8F8F8F)
    if path == "f16":
        return wide_code(16, 10, 15, op, s, idx, 2 * d, h & 0xFFFF) | (wide_code(16, 10, 15, op, s, idx, 2 * d + 1, h >> 16) << 16)
    if path == "f32":
        return wide_code(32, 23, 127, op, s, idx, d, h)
    return h


def path_codes(path: str, op: int, s: int, idx: int) -> list[int]:
    """The K codes of row (op 0) or column (op 1) `idx` at step s: code k is bits
    [k * code_bits, (k + 1) * code_bits) of the little-endian string of path_dword's."""
    cb, K = PATH_CODE_BITS[path], PATH_K[path]
    row = 0
    for d in range(K * cb // 32):
        row |= path_dword(path, op, s, idx, d) << (32 * d)
    return [(row >> (k * cb)) & ((1 << cb) - 1) for k in range(K)]


def path_opsel(op: int, s: int) -> int:
    return (s & 3) if op == 0 else ((s >> 1) & 3)


def path_scale(path: str, op: int, s: int, idx: int, block: int) -> int:
    dword = 0x7F7F7F7F + (_rotl32(path_step_hash(path, op, s, idx), 19 + 6 * block) & 0x01010101)
    return (dword >> (8 * path_opsel(op, s))) & 0xFF


def _operand_ints(path: str, codes, scales=None):
    """Rows of codes -> (rows of Python ints, exponent of their common unit). `scales[i][k // 32]`
    (E8M0) multiplies row i."""
    dec = [[path_decode(path, c) for c in row] for row in codes]
    if scales is not None:
        dec = [[(sg, e + scales[i][k // 32] - 127) for k, (sg, e) in enumerate(row)] for i, row in enumerate(dec)]
    emin = min((e for row in dec for sg, e in row if sg), default=0)
    return [[sg << (e - emin) if sg else 0 for sg, e in row] for row in dec], emin


def exact_product(path: str, a_codes, b_codes, scale_a=None, scale_b=None, acc=None):
    """The exact product of one instruction on codes, in Python integers: a_codes[row][k],
    b_codes[k][col], scale_a[row][k block], scale_b[k block][col]. Returns (units, abs_units,
    unit_exp): dim x dim lists with C = units * 2^unit_exp, and the sums of |term|."""
    dim, K = path_dim(path), PATH_K[path]
    bt = [[b_codes[k][c] for k in range(K)] for c in range(dim)]
    sbt = None if scale_b is None else [[scale_b[blk][c] for blk in range(2)] for c in range(dim)]
    a, ea = _operand_ints(path, a_codes, scale_a)
    b, eb = _operand_ints(path, bt, sbt)
    nz = [[(k, y) for k, y in enumerate(col) if y] for col in b]      # a zero operand adds no term
    units = [[sum(row[k] * y for k, y in col) for col in nz] for row in a]
    abs_units = [[sum(abs(row[k] * y) for k, y in col) for col in nz] for row in a]
    return units, abs_units, ea + eb


def _trailing_zeros(x: int) -> int:
    return (x & -x).bit_length() - 1


def path_expected(path: str) -> dict:
    """The expected tile of `path`'s chain of PATH_STEPS instructions on the generated data:
    {"dim", "units" (row-major ints), "unit_exp", "sum_abs_max", "limit_bits", "exact"}: every
    term is a multiple of 2^unit_exp (the smallest product exponent), and the chain is exact
    whatever the hardware's order while sum_abs_max < 2^limit_bits."""
    dim = path_dim(path)
    total = [[0] * dim for _ in range(dim)]
    total_abs = [[0] * dim for _ in range(dim)]
    steps = []
    for s in range(PATH_STEPS):
        a = [path_codes(path, 0, s, r) for r in range(dim)]
        bt = [path_codes(path, 1, s, c) for c in range(dim)]
        b = [[bt[c][k] for c in range(dim)] for k in range(PATH_K[path])]
        sa = sb = None
        if path in SCALED_PATHS:
            sa = [[path_scale(path, 0, s, r, blk) for blk in range(2)] for r in range(dim)]
            sb = [[path_scale(path, 1, s, c, blk) for c in range(dim)] for blk in range(2)]
        steps.append(exact_product(path, a, b, sa, sb))
    base = min(e for _, _, e in steps)
    for units, abs_units, e in steps:
        for r in range(dim):
            for c in range(dim):
                total[r][c] += units[r][c] << (e - base)
                total_abs[r][c] += abs_units[r][c] << (e - base)
    # every term is a multiple of 2^tz: the unit is the lowest set bit of the sums of |term|
    tz = min(_trailing_zeros(v) for row in total_abs for v in row if v)
    flat = [v >> tz for row in total for v in row]
    sum_abs_max = max(v >> tz for row in total_abs for v in row)
    limit = PATH_LIMIT_BITS.get(path, 24)
    return {"dim": dim, "units": flat, "unit_exp": base + tz, "sum_abs_max": sum_abs_max, "limit_bits": limit,
            "exact": sum_abs_max < (1 << limit)}


def tile_values(path: str, units, unit_exp: int) -> list:
    """units * 2^unit_exp as the accumulator holds it: ints for i8, floats elsewhere (exact)."""
    import math

    if path == "i8":
        return [u << unit_exp if unit_exp >= 0 else u >> -unit_exp for u in units]
    return [math.ldexp(u, unit_exp) for u in units]


def tile_words(path: str, values) -> list[int]:
    """The 32-bit words the kernel compares: fp32 bit patterns, i32, or (low, high) of each f64."""
    import struct

    if path == "i8":
        return [v & M32 for v in values]
    if path == "f64":
        out = []
        for v in values:
            bits = struct.unpack("<Q", struct.pack("<d", v))[0]
            out += [bits & M32, bits >> 32]
        return out
    return [struct.unpack("<I", struct.pack("<f", v))[0] for v in values]


def tile_checksum(words) -> int:
    """FNV-1a over the words' bytes, low byte first."""
    h = 0x811C9DC5
    for w in words:
        for b in range(4):
            h = ((h ^ ((w >> (8 * b)) & 0xFF)) * 0x01000193) & M32
    return h


def path_coverage(path: str) -> list[str]:
    """The coverage conditions `path`'s data does not meet (empty: all hold): "bits" (sign, every
    mantissa bit and every exponent bit the window varies take both values, in A and in B),
    "window", "asymmetry", "scales" (differ between rows, k blocks, A and B), "opsel"."""
    dim, K = path_dim(path), PATH_K[path]
    ebits, mbits, _bias = PATH_FORMAT[path]
    unmet = set()
    need = 0xFF
    if ebits:
        win = PATH_EXP_WINDOW[path]
        e_or = e_and = win[0]
        for e in win:
            e_or, e_and = e_or | e, e_and & e
        need = (1 << (ebits + mbits)) | ((e_or & ~e_and) << mbits) | ((1 << mbits) - 1)
    codes = [[[path_codes(path, op, s, i) for i in range(dim)] for s in range(PATH_STEPS)] for op in range(2)]
    full = (1 << PATH_CODE_BITS[path]) - 1
    for op in range(2):
        ones = zeros = 0
        for s in range(PATH_STEPS):
            for i in range(dim):
                for c in codes[op][s][i]:
                    ones |= c
                    zeros |= ~c & full
                    if ebits and not (path in ("f16", "f32", "f64") and c == 0):
                        if (c >> mbits) & ((1 << ebits) - 1) not in PATH_EXP_WINDOW[path]:
                            unmet.add("window")
        if ones & zeros & need != need:
            unmet.add("bits")
    n = min(dim, K)
    a_sym = all(codes[0][s][i][k] == codes[0][s][k][i] for s in range(PATH_STEPS) for i in range(n) for k in range(n))
    b_sym = all(codes[1][s][i][k] == codes[1][s][k][i] for s in range(PATH_STEPS) for i in range(n) for k in range(n))
    ab_t = all(codes[0][s][i] == codes[1][s][i] for s in range(PATH_STEPS) for i in range(dim))
    if a_sym or b_sym or ab_t:
        unmet.add("asymmetry")
    if path in SCALED_PATHS:
        sc = {(op, s, i, blk): path_scale(path, op, s, i, blk)
              for op in range(2) for s in range(PATH_STEPS) for i in range(dim) for blk in range(2)}
        if any(v not in SCALE_WINDOW for v in sc.values()):
            unmet.add("scales")
        rows = any(v != sc[(op, s, 0, blk)] for (op, s, i, blk), v in sc.items())
        blocks = any(v != sc[(op, s, i, 0)] for (op, s, i, blk), v in sc.items())
        ab = any(v != sc[(0, s, i, blk)] for (op, s, i, blk), v in sc.items())
        if not (rows and blocks and ab):
            unmet.add("scales")
        if not any(path_opsel(op, s) for op in range(2) for s in range(PATH_STEPS)):
            unmet.add("opsel")
    return sorted(unmet)


# ---- edge tiles: every operand code and every scale on the device, one term per accumulator ------
#
# The generators above stay inside an exponent window so that a chain of 8 instructions is exact
# in any order. A tile in which every accumulator has at most one non-zero term is exact whatever
# its codes, so these tiles hold what the window excludes: zero, subnormals, the largest normals,
# every code of the narrow formats and every E8M0 scale. One operand ("codes") holds the codes
# under test, the other ("units") a single +-1 per row or column (i8: -128 as well), at k =
# edge_kmap. They are inputs of `matrix_tile` (tests/test_gpu_selftest_edges.py) and are not part
# of the sweep.

EDGE_ROTATIONS = (0, 5)          # two placements of the units' k on the unscaled paths
EDGE_SCALE_TILES = 256           # scaled paths: 64 groups of scales x the 4 bytes of the scale register
EDGE_SCALE_SUM = (-2, 2)         # scale_a + scale_b - 254 of every (row, col, block) of a tile


def unit_codes(path: str) -> list[int]:
    """The codes of +1 and -1 (i8: and -128) that meet the codes under test."""
    if path == "i8":
        return [0x01, 0xFF, 0x80]
    _ebits, mbits, bias = PATH_FORMAT[path]
    one = bias << mbits
    return [one, one | 1 << (PATH_CODE_BITS[path] - 1)]


def code_is_finite(path: str, code: int) -> bool:
    """False for e4m3's S.1111.111 (NaN) and for an all-ones exponent field of e5m2, f16, f32 and
    f64 (Inf, NaN). e2m3, e2m1 and i8 have only finite codes."""
    if path in ("fp8", "mxfp8"):
        return code & 0x7F != 0x7F
    if path in ("bf8", "f16", "f32", "f64"):
        ebits, mbits, _bias = PATH_FORMAT[path]
        return (code >> mbits) & ((1 << ebits) - 1) != (1 << ebits) - 1
    return True


def edge_code_groups(path: str) -> list[list[int]]:
    """The codes the edge tiles of `path` put on the device, in groups that share a tile.
    Narrow formats: one group of all 2^bits codes, a non-finite one replaced by 0 (NaN x 0 would
    make its whole row NaN). f16 / f32 / f64: +-0 with, by magnitude, the smallest and largest
    subnormal and the smallest normal; 1, 1 + ulp and 2 - ulp; the largest finite value and the
    largest power of two. The codes of one group share the exponent of their last place, so the
    integers of `exact_product` stay small enough to convert to a float (f64 spans 2^2098)."""
    ebits, mbits, bias = PATH_FORMAT[path]
    bits = PATH_CODE_BITS[path]
    if path not in ("f16", "f32", "f64"):
        return [[c if code_is_finite(path, c) else 0 for c in range(1 << bits)]]
    ones, top = (1 << mbits) - 1, ((1 << ebits) - 2) << mbits
    groups = ([1, ones, 1 << mbits], [bias << mbits, bias << mbits | 1, bias << mbits | ones], [top | ones, top])
    sign = 1 << (bits - 1)
    return [[c | s for c in [0] + g for s in (0, sign)] for g in groups]


def edge_kmap(path: str, i: int, rot: int) -> int:
    """The one k at which row (units in A) or column (units in B) i of the units operand is
    non-zero. K <= dim: (i + rot) mod K. The scaled paths (K = 64, dim = 32) take k block
    (i >> 1) & 1, so that both blocks and both parities of i meet in every tile."""
    dim, K = path_dim(path), PATH_K[path]
    if K <= dim:
        return (i + rot) % K
    return (i + rot) % dim + dim * ((i >> 1) & 1)


def edge_tile(path: str, codes, side: int, rot: int = 0, offset: int = 0):
    """(a, b): a[row][k] and b[k][col]. side 0: `codes`, cyclically from `offset`, fill A at every
    k some column's unit sits at, and B holds the units; side 1: the codes fill B, the units A.
    Everything else is 0, so accumulator (row, col) has the one term at k = edge_kmap of its
    units index."""
    dim, K = path_dim(path), PATH_K[path]
    units = unit_codes(path)
    kmap = [edge_kmap(path, i, rot) for i in range(dim)]
    image = sorted(set(kmap))
    held = [[0] * K for _ in range(dim)]          # the codes operand, by its own index (row | col) and k
    n = offset
    for j in range(dim):
        for k in image:
            held[j][k] = codes[n % len(codes)]
            n += 1
    unit = [[0] * K for _ in range(dim)]
    for i in range(dim):
        unit[i][kmap[i]] = units[(i + (i >> 2)) % len(units)]
    a, bt = (held, unit) if side == 0 else (unit, held)
    return a, [[bt[c][k] for c in range(dim)] for k in range(K)]


def edge_scales(path: str, t: int):
    """(scale_a[row][block], scale_b[block][col], opsel) of scaled tile t (0..EDGE_SCALE_TILES-1).
    Block b of group q = t // 4 has s0 = min(4 q + 2 b, 253); A's scales are s0 + (row & 1), B's
    254 - s0 - (col & 1): scale_a + scale_b - 254 is -1, 0 or 1 for every (row, col, block), and
    over the groups A and B each take every value 0..254. t % 4 is A's byte of the scale
    register, (t % 4 + q) % 4 B's: every value meets every byte on both sides."""
    dim = path_dim(path)
    q, byte = divmod(t, 4)
    s0 = [min(4 * q + 2 * b, 253) for b in range(2)]
    sa = [[s0[b] + (r & 1) for b in range(2)] for r in range(dim)]
    sb = [[254 - s0[b] - (c & 1) for c in range(dim)] for b in range(2)]
    return sa, sb, (byte, (byte + q) % 4)


def edge_tiles(path: str):
    """Yields (a, b, scale_a, scale_b, opsel) of every edge tile of `path` (scales None and opsel
    (0, 0) on the unscaled paths). Unscaled: every group of edge_code_groups on both sides at both
    EDGE_ROTATIONS. Scaled: EDGE_SCALE_TILES tiles, the side alternating, each holding every code
    of the format (1,024 slots) under its own scales, rotation and offset."""
    groups = edge_code_groups(path)
    if path not in SCALED_PATHS:
        for g, codes in enumerate(groups):
            for side in range(2):
                for rot in EDGE_ROTATIONS:
                    a, b = edge_tile(path, codes, side, rot, 3 * rot + g)
                    yield a, b, None, None, (0, 0)
        return
    for t in range(EDGE_SCALE_TILES):
        sa, sb, opsel = edge_scales(path, t)
        a, b = edge_tile(path, groups[0], (t + t // 4) & 1, t % 32, 37 * t)
        yield a, b, sa, sb, opsel


def product_words(path: str, a, b, scale_a=None, scale_b=None) -> list[int]:
    """The words `matrix_tile` must return for one exact instruction: exact_product as the
    accumulator holds it. An accumulator whose only term is -0 holds +0."""
    units, _abs, unit_exp = exact_product(path, a, b, scale_a, scale_b)
    return tile_words(path, tile_values(path, [u for row in units for u in row], unit_exp))


def fold_paths(records, paths, expected_cus) -> dict:
    """Folds `cu_sweep_paths` records `(xcc, hw_id, fail, simds, lds_bad, path_fail_bits,
    path_waves)` by CU; `paths` names the bits of `path_fail_bits` in order. A CU failed a path
    when any of its visits did (a clean revisit clears nothing). `failed` maps each failed path
    to its `[xcc, cu_key]` list, `cus` lists per failed CU its paths and the waves (bit w: wave
    w) that saw one fail; `uncovered` / `cus_uncovered` as in `fold_sweep`: not a failure."""
    paths = list(paths)
    by_cu = _by_cu(records)
    failures = []
    for k, visits in sorted(by_cu.items()):
        bits = _or(v[3] for v in visits)
        if bits:
            names = [p for i, p in enumerate(paths) if bits >> i & 1] + (["record"] if bits >> len(paths) else [])
            failures.append((k, names, {"paths": names, "waves": _or(v[4] for v in visits)}))
    return _named_failures(by_cu, expected_cus, failures)


@dataclass
class DeepReport:
    device: int
    ok: bool = True
    seconds: float = 0.0
    sweep: dict | None = None        # fold_sweep's report + lds_bytes, launches, ms (last launch)
    hbm: dict | None = None          # hbm_pattern_check's report; None when not run
    error: str | None = None         # a HIP exception: the device failed
    masked: bool = False             # swept only the CUs in `cu_mask_bits`
    seed: int = 0
    notes: list[str] = field(default_factory=list)
    paths: dict | None = None        # {"checked": [names], "failed": {name: [[xcc, cu_key], ...]}}; None: not run
    cu_keys: list = field(default_factory=list, repr=False)   # sorted (xcc, cu_key) of every CU a record came from
    # {"checked": [names], "failed": {kind: [[xcc, cu_key], ...]}, "cus": fold_valu's, "reg_slots", "ms"}; None: not run
    valu: dict | None = field(default=None, repr=False)
    # {"checked": [names], "failed": {kind: [[xcc, cu_key], ...]}, "cus": fold_scalar's, "sreg_slots", "ms"}; None: not run
    scalar: dict | None = field(default=None, repr=False)

    def to_dict(self) -> dict:
        """What /metrics and --json show: every field but `cu_keys`, as before that field existed;
        `valu` only when the vector-ALU part ran, `scalar` only when the scalar part did."""
        d = asdict(self)
        del d["cu_keys"]
        for part in ("valu", "scalar"):
            if d[part] is None:
                del d[part]
        return d

    def describe_failure(self) -> str:
        """What failed, for the agent's warning line."""
        if self.error:
            return self.error
        parts = [f"CU (xcc {f['xcc']}, key {f['cu_key']:#x}) {'+'.join(f['kinds'])}"
                 + (f" at LDS dword {f['lds_bad_off']}" if f["lds_bad_off"] >= 0 else "")
                 for f in (self.sweep or {}).get("failed", [])]
        for name, where in sorted(((self.paths or {}).get("failed") or {}).items()):
            parts.append(f"matrix path {name} on " + ", ".join(f"CU (xcc {x}, key {k:#x})" for x, k in where))
        for c in (self.valu or {}).get("cus", []):
            at = f" at slot {c['bad_slot']}, wave {c['bad_wave']} lane {c['bad_lane']}" if c["bad_slot"] >= 0 else ""
            parts.append(f"vector ALU {'+'.join(c['kinds'])} on CU (xcc {c['xcc']}, key {c['cu_key']:#x}){at}")
        for c in (self.scalar or {}).get("cus", []):
            at = f", at slot {c['bad_slot']}, wave {c['bad_slot_wave']}" if c["bad_slot"] >= 0 else ""
            at += f", at word {c['bad_word']}, wave {c['bad_word_wave']}" if c["bad_word"] >= 0 else ""
            parts.append(f"scalar unit {'+'.join(c['kinds'])} on CU (xcc {c['xcc']}, key {c['cu_key']:#x}){at}")
        if self.hbm and self.hbm.get("errors"):
            first = self.hbm.get("first") or []
            at = f", first at byte {first[0][0]} (expected {first[0][1]:#010x}, got {first[0][2]:#010x})" if first else ""
            parts.append(f"{self.hbm['errors']} HBM elements wrong{at}")
        return "; ".join(parts)


def hbm_check_takes_mask(P) -> bool:
    """Whether this probe's `hbm_pattern_check` has the `cu_mask` argument: read from the binding's
    own signature (a Python stand-in's parameters, or the signature line pybind11 puts into the doc
    string), never from an error's text, so that a refused argument stays an error."""
    import inspect

    f = P.hbm_pattern_check
    try:
        params = inspect.signature(f).parameters
    except (TypeError, ValueError):            # a built-in without a text signature: its doc string has one
        return "cu_mask" in (getattr(f, "__doc__", None) or "")
    return "cu_mask" in params or any(p.kind is p.VAR_KEYWORD for p in params.values())


def free_hbm_bytes(P, device: int, cap_mib: int = 0) -> int:
    """What the HBM check may take: the free memory less 2 GiB of headroom, capped by
    `cap_mib` when positive, in whole 16-byte elements."""
    free, _total = P.mem_info(device)
    n = max(0, int(free) - HBM_HEADROOM)
    if cap_mib > 0:
        n = min(n, cap_mib << 20)
    return n & ~15


def _hbm_check(P, device: int, hbm_bytes: int, seed: int, mask: list[int], notes: list[str]) -> dict | None:
    """`hbm_pattern_check`'s report for `hbm_bytes`, or for the half, or the quarter, where that
    much cannot be allocated; on a stream masked to `mask` when it is not empty. None where nothing
    was checked; `notes` gets every allocation that failed and a probe that takes no mask."""
    want = hbm_bytes & ~15
    for _ in range(MAX_LAUNCHES):      # memory taken by someone else meanwhile is no device fault
        if want < 16:
            break
        if mask and not hbm_check_takes_mask(P):
            notes.append("this probe's hbm_pattern_check takes no cu_mask: HBM was not checked on the masked device")
            break
        try:
            # the keyword only with a mask: a probe from before it is never called with it
            return dict(P.hbm_pattern_check(device, want, seed, 2, cu_mask=mask) if mask
                        else P.hbm_pattern_check(device, want, seed, 2))
        except MemoryError:
            notes.append(f"{want} bytes of HBM could not be allocated")
            want = (want // 2) & ~15
    return None


def deep_selftest(P, device: int, cu_mask_bits: list[int] | None = None, hbm_bytes: int = 0,
                  seed: int | None = None, rounds: int = 4, paths=None, valu=None, scalar=None) -> DeepReport:
    """One deep check of HIP device `device` on the calling thread. `cu_mask_bits` restricts
    the sweep to those CU-mask bits (the agent passes the units no tenant holds; None: the
    whole chip). `hbm_bytes` > 0 adds the pattern check of that much fresh memory, on a stream
    with the same mask when one is given (a probe that cannot gets a note and no HBM check). `paths`
    (`parse_paths`: None, "all", "a,b" or a list of names) makes the sweep launches
    `cu_sweep_paths` with those matrix paths instead of `cu_sweep`: still one visit per CU.
    `valu` (`selftest_valu.parse_valu`) makes each launch of the coverage loop be followed by a
    `cu_sweep_valu` launch of those vector-ALU groups on the same mask. `scalar`
    (`selftest_scalar.parse_scalar`) adds, after that, a `cu_sweep_scalar` launch of those scalar groups.
    `ok` is false if and only if a CU failed a check, a path, a vector-ALU or a scalar group, HBM
    errors were counted, or HIP raised."""
    from .selftest_scalar import fold_scalar, parse_scalar
    from .selftest_valu import fold_valu, parse_valu

    from ..agent import cumask

    if seed is None:
        seed = int(time.time() * 1000) & M32   # another pattern every run
    rep = DeepReport(device=device, masked=cu_mask_bits is not None, seed=seed)
    names = parse_paths(paths)
    if names and not hasattr(P, "cu_sweep_paths"):
        rep.notes.append("this probe has no cu_sweep_paths: the plain sweep ran and no matrix path was checked")
        names = []
    vnames = parse_valu(valu)
    if vnames and not hasattr(P, "cu_sweep_valu"):
        rep.notes.append("this probe has no cu_sweep_valu: no vector-ALU group was checked")
        vnames = []
    snames = parse_scalar(scalar)
    if snames and not hasattr(P, "cu_sweep_scalar"):
        rep.notes.append("this probe has no cu_sweep_scalar: no scalar group was checked")
        snames = []
    t0 = time.perf_counter()
    try:
        cus = int(P.device_props(device)["cus"])
        mask = cumask.mask_words(cu_mask_bits, cus) if cu_mask_bits is not None else []
        expected = len(set(cu_mask_bits)) if cu_mask_bits is not None else cus
        records, launches, r, last = [], 0, rounds, {}
        vrecords, vlast = [], {}
        srecords, slast = [], {}
        while True:
            last = P.cu_sweep_paths(device, mask, r, seed, names) if names else P.cu_sweep(device, mask, r, seed)
            launches += 1
            records.extend(last["records"])
            if vnames:
                vlast = P.cu_sweep_valu(device, mask, r, seed, vnames)
                vrecords.extend(vlast["records"])
            if snames:
                slast = P.cu_sweep_scalar(device, mask, r, seed, snames)
                srecords.extend(slast["records"])
            sweep = fold_sweep([rec[:5] for rec in records], expected)
            if sweep["cus_uncovered"] == 0 or launches >= MAX_LAUNCHES:
                break
            r *= 2
        sweep.update(lds_bytes=int(last["lds_bytes"]), launches=launches, ms=float(last["ms"]))
        rep.sweep = sweep
        rep.cu_keys = sorted({(rec[0], cu_key(rec[1])) for rec in records})
        if names:
            rep.paths = {"checked": names, "failed": fold_paths(records, last["paths"], expected)["failed"]}
        if vnames:
            vf = fold_valu(vrecords, vlast["groups"], expected)
            rep.valu = {"checked": vnames, "failed": vf["failed"], "cus": vf["cus"], "reg_slots": int(vlast["reg_slots"]),
                        "ms": float(vlast["ms"])}
            rep.cu_keys = sorted(set(rep.cu_keys) | {(rec[0], cu_key(rec[1])) for rec in vrecords})
            if vf["cus_uncovered"]:
                rep.notes.append(f"{vf['cus_uncovered']} CUs not reached by the vector-ALU launches")
        if snames:
            sf = fold_scalar(srecords, slast["groups"], expected)
            rep.scalar = {"checked": snames, "failed": sf["failed"], "cus": sf["cus"], "sreg_slots": int(slast["sreg_slots"]),
                          "ms": float(slast["ms"])}
            rep.cu_keys = sorted(set(rep.cu_keys) | {(rec[0], cu_key(rec[1])) for rec in srecords})
            if sf["cus_uncovered"]:
                rep.notes.append(f"{sf['cus_uncovered']} CUs not reached by the scalar launches")
        if sweep["cus_uncovered"]:
            rep.notes.append(f"{sweep['cus_uncovered']} CUs not reached in {launches} launches")
        if hbm_bytes > 0:
            rep.hbm = _hbm_check(P, device, hbm_bytes, seed, mask, rep.notes)
        rep.ok = (not sweep["failed"] and not (rep.hbm and rep.hbm["errors"])
                  and not (rep.paths and rep.paths["failed"]) and not (rep.valu and rep.valu["failed"])
                  and not (rep.scalar and rep.scalar["failed"]))
    except Exception as e:                     # a HIP error is a failed device
        log.exception("deep self-test of device %d raised", device)
        rep.ok, rep.error = False, f"{type(e).__name__}: {e}"
    rep.seconds = time.perf_counter() - t0
    return rep


def failed_cus(report: DeepReport) -> set[tuple[int, int]]:
    """The `(xcc, cu_key)` of every CU that failed a check, a matrix path, a vector-ALU or a scalar group in `report`."""
    out = {(f["xcc"], f["cu_key"]) for f in (report.sweep or {}).get("failed", [])}
    for part in (report.paths, report.valu, report.scalar):
        for where in ((part or {}).get("failed") or {}).values():
            out |= {(x, k) for x, k in where}
    return out


def fenceable(report: DeepReport) -> bool:
    """Whether a failed report names CUs that a CU-mask fence could keep tenants off: no HIP
    error, no HBM errors, no CU whose record is garbled (the `record` kind: then the CU's
    identity is as doubtful as its result), and at least one failed CU or path."""
    if report.error or (report.hbm and report.hbm.get("errors")):
        return False
    if any("record" in f["kinds"] for f in (report.sweep or {}).get("failed", [])):
        return False
    if any("record" in ((part or {}).get("failed") or {}) for part in (report.paths, report.valu, report.scalar)):
        return False
    return bool(failed_cus(report))


@dataclass
class Localisation:
    bad_units: list[int] = field(default_factory=list)      # units whose own masked sweep failed
    unit_keys: dict = field(default_factory=dict)           # unit -> sorted [(xcc, cu_key)] its records came from
    unexplained: list = field(default_factory=list)         # failed CUs of the report outside every bad unit
    seconds: float = 0.0
    launches: dict = field(default_factory=dict)            # unit -> sweep launches it took
    uncovered: dict = field(default_factory=dict)           # unit -> CUs of it no launch reached (absent: 0)

    def to_dict(self) -> dict:
        return asdict(self)


def localise_failure(P, device: int, report: DeepReport, candidate_units, unit_size: int, paths=None,
                     seed: int | None = None, rounds: int = 4, valu=None, scalar=None) -> Localisation:
    """Which CU-mask units hold the CUs that failed in `report`. Every unit of `candidate_units`
    (unit u is mask bits [u * unit_size, (u + 1) * unit_size)) gets one `deep_selftest` masked to
    it: the same `paths`, `valu` and `scalar`, no HBM check, and the same re-launch for coverage. A unit is bad when
    that run is not ok. `unexplained` lists the failed CUs of `report` that no bad unit's sweep
    ran on: a failure that did not come back, or a mask that does not reach where it lives.
    Either way a fence of the bad units would not cover it."""
    t0 = time.perf_counter()
    loc = Localisation()
    for u in sorted(set(candidate_units)):
        bits = [u * unit_size + k for k in range(unit_size)]
        r = deep_selftest(P, device, cu_mask_bits=bits, seed=seed, rounds=rounds, paths=paths, valu=valu, scalar=scalar)
        loc.unit_keys[u] = list(r.cu_keys)
        if r.sweep:
            loc.launches[u] = r.sweep["launches"]
            if r.sweep["cus_uncovered"]:
                loc.uncovered[u] = r.sweep["cus_uncovered"]
        if not r.ok:
            loc.bad_units.append(u)
    explained = {k for u in loc.bad_units for k in loc.unit_keys[u]}
    loc.unexplained = sorted(failed_cus(report) - explained)
    loc.seconds = time.perf_counter() - t0
    return loc


def would_fence(P, device: int, report: DeepReport, max_units: int, paths=None, valu=None, scalar=None) -> dict:
    """What `--fence N` prints: {"units", "cus" (unit -> its CUs), "reason" (when no unit),
    "seconds"}. Only a whole MI355X: the unit is one CU on each of its 8 XCDs."""
    from .. import types as T

    out = {"units": [], "cus": {}, "reason": "", "seconds": 0.0}
    cus = int(P.device_props(device)["cus"])
    if cus != T.MI355X_CUS:
        out["reason"] = f"{cus} CUs: the CU-mask units are measured on a whole MI355X ({T.MI355X_CUS} CUs) only"
    elif not fenceable(report):
        out["reason"] = "a HIP error, HBM errors or a garbled record are not a CU's to fence"
    else:
        loc = localise_failure(P, device, report, range(cus // T.MI355X_XCDS), T.MI355X_XCDS, paths, valu=valu, scalar=scalar)
        out["seconds"] = loc.seconds
        if loc.unexplained:
            out["reason"] = f"failing CUs {loc.unexplained} did not fail again in any unit"
        elif len(loc.bad_units) > max_units:
            out["reason"] = f"{len(loc.bad_units)} units fail, more than {max_units}"
        else:
            out["units"] = loc.bad_units
            out["cus"] = {str(u): [list(k) for k in loc.unit_keys[u]] for u in loc.bad_units}
    return out


def main(argv: list[str] | None = None) -> int:
    import argparse
    import json

    from ..native import probe

    ap = argparse.ArgumentParser(prog="python -m nanogpu.probe.selftest",
                                 description="deep self-test of one GPU: every CU's MFMA and LDS, and HBM")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--hbm-mib", type=int, default=1024,
                    help="HBM to pattern-check in MiB (default 1024; 0: all free memory less 2 GiB)")
    ap.add_argument("--paths", default="", metavar="all|LIST",
                    help="matrix paths every CU also runs: 'all' or a comma-separated list of " + ", ".join(PATHS))
    ap.add_argument("--valu", default="", metavar="all|LIST",
                    help="vector-ALU groups, 'approx' and 'regs' every CU also runs: 'all' or a comma-separated list")
    ap.add_argument("--scalar", default="", metavar="all|LIST",
                    help="scalar-ALU groups, 'vcc', 'smem' and 'sregs' every CU also runs: 'all' or a comma-separated list")
    ap.add_argument("--fence", type=int, default=0, metavar="N",
                    help="after a failed sweep, print the CU-mask units (at most N) and CUs an agent started with "
                         "--selftest-fence N would fence; changes nothing on the device or the node")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args(argv)
    try:
        from .selftest_scalar import parse_scalar
        from .selftest_valu import parse_valu

        names = parse_paths(a.paths)
        vnames = parse_valu(a.valu)
        snames = parse_scalar(a.scalar)
    except ValueError as e:
        ap.error(str(e))
    P = probe(required=True)
    nbytes = free_hbm_bytes(P, a.device, a.hbm_mib)
    rep = deep_selftest(P, a.device, hbm_bytes=nbytes, paths=names, valu=vnames, scalar=snames)
    plan = would_fence(P, a.device, rep, a.fence, names, valu=vnames, scalar=snames) if a.fence > 0 and not rep.ok else None
    if a.json:
        print(json.dumps(dict(rep.to_dict(), fence=plan) if a.fence > 0 else rep.to_dict()))
    else:
        s, h = rep.sweep or {}, rep.hbm or {}
        print(f"device {a.device}: {'ok' if rep.ok else 'FAILED'} in {rep.seconds:.3f} s")
        if s:
            print(f"  CUs checked {s['cus_seen']}/{s['cus_expected']} (per XCD {s['per_xcd']}), "
                  f"{len(s['failed'])} failed, {s['cus_uncovered']} not reached, LDS {s['lds_bytes']} B per CU, "
                  f"sweep {s['ms']:.3f} ms in {s['launches']} launch(es)")
        def print_named(what: str, part: dict, detail: str = "") -> None:
            bad = part["failed"]
            print(f"  {what} {', '.join(part['checked'])}{detail}: "
                  + (", ".join(f"{n} failed on {len(w)} CU(s)" for n, w in sorted(bad.items())) if bad else "all clean"))

        if rep.paths:
            print_named("matrix paths", rep.paths)
        if rep.valu:
            print_named("vector ALU", rep.valu, f" ({rep.valu['reg_slots']} registers a lane, {rep.valu['ms']:.3f} ms)")
        if rep.scalar:
            print_named("scalar unit", rep.scalar, f" ({rep.scalar['sreg_slots']} registers a wave, {rep.scalar['ms']:.3f} ms)")
        if h:
            print(f"  HBM {h['bytes']} B x 2 passes: {h['errors']} errors, fill {h['fill_gbs']:.0f} GB/s, "
                  f"verify {h['verify_gbs']:.0f} GB/s, {h.get('verify_launches', 1)} launch(es) a pass")
        if not rep.ok:
            print("  " + rep.describe_failure())
        for n in rep.notes:
            print("  note: " + n)
        if plan is not None:
            if plan["units"]:
                print(f"  would fence {len(plan['units'])} unit(s) in {plan['seconds']:.3f} s:")
                for u in plan["units"]:
                    print(f"    unit {u}: " + ", ".join(f"(xcc {x}, key {k:#x})" for x, k in plan["cus"][str(u)]))
            else:
                print("  would fence nothing: " + plan["reason"])
    return 0 if rep.ok else 1


if __name__ == "__main__":
    raise SystemExit(main())
