"""Matrix-path part of the deep self-test: the Python twin of native/include/nanogpu/selftest_paths_host.h.

`cu_sweep_paths` (native/hip/probe_sweep.inc) is `cu_sweep` with, in every visit, an exact chain of 8
instructions of each selected matrix path (`PATHS`) on all 4 waves, every accumulator compared bit
for bit with a host tile. The operand data is generated as codes and decoded on the host; the
decoders, generators and expected tiles below are the twin of the header, which states the
exactness argument. `fold_paths` reports per CU which paths failed. What the generators leave out
(zero, subnormals, the largest normals, other scales) `edge_tiles` puts through `matrix_tile`.
"""
from __future__ import annotations

from .selftest_common import M32, Part, by_cu, mix32, named_failures, or_all, parse_names, rotl32

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


def parse_paths(spec) -> list[str]:
    """`parse_names` over `PATHS`: None / "" -> [], "all", "a,b" or a list of names; ValueError on an unknown one."""
    return parse_names(spec, PATHS, "matrix path")


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


def path_step_hash(path: str, op: int, s: int, idx: int) -> int:
    """One mix32 per (path, op, idx), varied by step with three operations: the generator runs
    on every wave of every visit, so it is cheap on purpose."""
    base = mix32(0x9E3779B9 ^ (PATHS.index(path) << 27) ^ (op << 26) ^ (idx << 8))
    return ((base ^ (base >> (s + 3))) + s * 0x9E3779B9) & M32


def path_hash(path: str, op: int, s: int, idx: int, d: int) -> int:
    """The hash behind dword d (0..15) of a row / column: one rotation of the step's hash."""
    return rotl32(path_step_hash(path, op, s, idx), 7 * d + 3)


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
    dword = 0x7F7F7F7F + (rotl32(path_step_hash(path, op, s, idx), 19 + 6 * block) & 0x01010101)
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
    cus = by_cu(records)
    failures = []
    for k, visits in sorted(cus.items()):
        bits = or_all(v[3] for v in visits)
        if bits:
            names = [p for i, p in enumerate(paths) if bits >> i & 1] + (["record"] if bits >> len(paths) else [])
            failures.append((k, names, {"paths": names, "waves": or_all(v[4] for v in visits)}))
    return named_failures(cus, expected_cus, failures)


PART = Part(
    key="paths", names=PATHS, noun="matrix path", flag_noun="path", binding="cu_sweep_paths", names_key="paths",
    fold=fold_paths, in_sweep=True, none_in_dict=True, label="matrix paths",
    clauses=lambda d: [f"matrix path {name} on " + ", ".join(f"CU (xcc {x}, key {k:#x})" for x, k in where)
                       for name, where in sorted((d.get("failed") or {}).items())],
    note_missing="this probe has no cu_sweep_paths: the plain sweep ran and no matrix path was checked",
    help="matrix paths every CU also runs: 'all' or a comma-separated list of " + ", ".join(PATHS),
    agent_help="the deep self-test also runs an exact MFMA chain of these matrix paths on every CU: "
               "'all' or a comma-separated list of f16, fp8, bf8, i8, mxfp8, mxfp6, mxfp4, f32, f64 "
               "(implies --selftest-deep; start-up and periodic runs alike)",
    metric_help="matrix paths the last deep self-test ran on every CU",
    failed_metric=("nanogpu_selftest_path_cus_failed", "path", "CUs that failed the matrix path in the last deep self-test"))
