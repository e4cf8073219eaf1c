"""Vector-ALU part of the deep self-test: the Python twin of native/include/nanogpu/selftest_valu_host.h.

`cu_sweep_valu` (native/hip/probe_valu.inc) makes all four waves of every CU run exact chains of
vector-ALU instructions (`GROUPS[:NUM_EXACT]`), the transcendental instructions (`approx`) and a
pattern test of the SIMD's vector register file (`regs`). This module computes what the exact
groups must give, in Python integers and `fractions.Fraction` (every IEEE step is the exact
rational result rounded to nearest-even by `round_rne`; nothing here calls a fused multiply-add),
the `approx` ranges, and folds the records by CU (`fold_valu`).
"""
from __future__ import annotations

import math
import struct
from fractions import Fraction

from .selftest_common import (M32, M64, Part, by_cu, mix32, named_failures, parse_names, rotl32, simds_seen_min,
                              tile_checksum)

GROUPS = ("fma32", "fma64", "pkfma16", "pkfma32", "addmul32", "int32", "int64", "bits", "dot", "cvt", "xlane",
          "approx", "regs")                      # bit order of the records
NUM_EXACT = 11
EXACT_GROUPS = GROUPS[:NUM_EXACT]
FP_GROUPS = GROUPS[:5]
STEPS = 8
LANES = 64
APPROX_OPS = ("exp2", "log2", "rcp", "rsq", "sqrt")
APPROX_ULPS = 8
REG_SLOTS = 448
RECORD_WORDS = 8
EXP_A, EXP_B, EXP_X0 = -3, 0, 0
# fail bits, by wave: exact groups, register file, approx bound, approx hash unlike wave 0's
FAIL_EXACT, FAIL_REGS, FAIL_BOUND, FAIL_HASH = 0xF, 0xF0, 0xF00, 0xF000

F64, F32, F16, BF16, E4M3, E5M2 = (53, 11, 1023), (24, 8, 127), (11, 5, 15), (8, 8, 127), (4, 4, 7), (3, 5, 15)


def parse_valu(spec) -> list[str]:
    """`parse_names` over `GROUPS`: None / "" -> [], "all", "a,b" or a list of names; ValueError on an unknown one."""
    return parse_names(spec, GROUPS, "vector-ALU group")


def operand(group: str, s: int, lane: int, k: int) -> int:
    return mix32(0x5A17C0DE ^ (GROUPS.index(group) << 24) ^ (s << 16) ^ (lane << 8) ^ k)


def f32_win(u: int, e: int) -> int:
    return (u & 0x807FFFFF) | ((127 + e) << 23)


def f64_win(hi: int, lo: int, e: int) -> int:
    return ((hi & 0x800FFFFF) << 32) | lo | ((1023 + e) << 52)


def f16_win(u: int, e: int) -> int:
    return (u & 0x83FF) | ((15 + e) << 10)


def f16x2_win(u: int, e: int) -> int:
    return f16_win(u & 0xFFFF, e) | (f16_win(u >> 16, e) << 16)


class Conds:
    """The header's condition counters, over one group's 64 lanes."""

    def __init__(self):
        self.eff_add = self.eff_sub = self.round_up = self.round_down = self.abnormal = 0
        self.carry31 = self.carry63 = self.borrow63 = 0
        self.tie_up, self.tie_down = [0] * 5, [0] * 5

    def to_dict(self) -> dict:
        return {k: getattr(self, k) for k in ("eff_add", "eff_sub", "round_up", "round_down", "carry31", "carry63",
                                              "borrow63", "tie_up", "tie_down")}


def decode(bits: int, fmt, c: Conds) -> Fraction:
    """The value of a finite normal code of format (precision, exponent bits, bias)."""
    p, ebits, bias = fmt
    m = p - 1
    ef = (bits >> m) & ((1 << ebits) - 1)
    if ef == 0 or ef == (1 << ebits) - 1:
        c.abnormal += 1
    v = Fraction((bits & ((1 << m) - 1)) | (1 << m)) * Fraction(2) ** (ef - bias - m)
    return -v if (bits >> (m + ebits)) & 1 else v


def round_rne(v: Fraction, fmt, c: Conds):
    """(code, tie) of the exact value v rounded to nearest, ties to even: tie is +1 / -1 when v lay
    exactly between two values and the magnitude went up / down, else 0."""
    p, ebits, bias = fmt
    if v == 0:
        c.abnormal += 1
        return 0, 0
    neg, a = v < 0, abs(v)
    e = a.numerator.bit_length() - a.denominator.bit_length()      # 2^e <= a < 2^(e + 2)
    if a < Fraction(2) ** e:
        e -= 1
    elif a >= Fraction(2) ** (e + 1):
        e += 1
    scaled = a / Fraction(2) ** (e - (p - 1))                        # in [2^(p-1), 2^p)
    kept = scaled.numerator // scaled.denominator
    rest = scaled - kept
    tie = 0
    if rest:
        up = rest > Fraction(1, 2) or (rest == Fraction(1, 2) and kept & 1)
        if rest == Fraction(1, 2):
            tie = 1 if up else -1
        if up:
            kept += 1
            c.round_up += 1
        else:
            c.round_down += 1
        if kept >> p:
            kept >>= 1
            e += 1
    ef = e + bias
    ef_max = (1 << ebits) - 2 + (1 if ebits == 4 else 0)
    if ef < 1 or ef > ef_max or (ebits == 4 and ef == 15 and kept & 7 == 7):
        c.abnormal += 1
    m = p - 1
    return (int(neg) << (m + ebits)) | (ef << m) | (kept & ((1 << m) - 1)), tie


def fma(a: int, x: int, b: int, fmt, c: Conds) -> int:
    prod, add = decode(a, fmt, c) * decode(x, fmt, c), decode(b, fmt, c)
    if (prod < 0) == (add < 0):
        c.eff_add += 1
    else:
        c.eff_sub += 1
    return round_rne(prod + add, fmt, c)[0]


def _fma_chain(group: str, lane: int, k: int, fmt, win, c: Conds) -> int:
    x = win(operand(group, 0, lane, 2 + 4 * k), EXP_X0)
    for s in range(STEPS):
        x = fma(win(operand(group, s, lane, 4 * k), EXP_A), x, win(operand(group, s, lane, 1 + 4 * k), EXP_B), fmt, c)
    return x


def lane_fma32(lane: int, c: Conds) -> list[int]:
    return [_fma_chain("fma32", lane, k, F32, f32_win, c) for k in range(2)]


def lane_fma64(lane: int, c: Conds) -> list[int]:
    g = "fma64"
    x = f64_win(operand(g, 0, lane, 4), operand(g, 0, lane, 5), EXP_X0)
    for s in range(STEPS):
        x = fma(f64_win(operand(g, s, lane, 0), operand(g, s, lane, 1), EXP_A), x,
                f64_win(operand(g, s, lane, 2), operand(g, s, lane, 3), EXP_B), F64, c)
    return [x & M32, x >> 32]


def lane_pkfma16(lane: int, c: Conds) -> list[int]:
    out = []
    for k in range(2):
        halves = []
        for h in range(2):                       # the two halves of a word are independent chains
            def win(u, e, h=h):
                return f16_win((u >> (16 * h)) & 0xFFFF, e)
            halves.append(_fma_chain("pkfma16", lane, k, F16, win, c))
        out.append(halves[0] | (halves[1] << 16))
    return out


def pkfma32(a, x, b, c: Conds) -> list[int]:
    """v_pk_fma_f32: two independent f32 FMAs, element j of each pair."""
    return [fma(a[j], x[j], b[j], F32, c) for j in range(2)]


def lane_pkfma32(lane: int, c: Conds) -> list[int]:
    g = "pkfma32"
    x = [f32_win(operand(g, 0, lane, 4 + j), EXP_X0) for j in range(2)]
    for s in range(STEPS):
        x = pkfma32([f32_win(operand(g, s, lane, j), EXP_A) for j in range(2)], x,
                    [f32_win(operand(g, s, lane, 2 + j), EXP_B) for j in range(2)], c)
    return x


def mul32(a: int, b: int, c: Conds) -> int:
    """v_mul_f32: the exact product rounded once."""
    return round_rne(decode(a, F32, c) * decode(b, F32, c), F32, c)[0]


def add32(a: int, b: int, c: Conds) -> int:
    """v_add_f32: the exact sum rounded once."""
    p, q = decode(a, F32, c), decode(b, F32, c)
    if (p < 0) == (q < 0):
        c.eff_add += 1
    else:
        c.eff_sub += 1
    return round_rne(p + q, F32, c)[0]


def lane_addmul32(lane: int, c: Conds) -> list[int]:
    g, out = "addmul32", []
    for k in range(2):
        x = f32_win(operand(g, 0, lane, 2 + 4 * k), EXP_X0)
        for s in range(STEPS):
            x = add32(mul32(f32_win(operand(g, s, lane, 4 * k), EXP_A), x, c), f32_win(operand(g, s, lane, 1 + 4 * k), EXP_B), c)
        out.append(x)
    return out


def _add64(a: int, b: int, c: Conds) -> int:
    if ((a & M32) + (b & M32)) >> 32:
        c.carry31 += 1
    if (a + b) >> 64:
        c.carry63 += 1
    return (a + b) & M64


def _sub64(a: int, b: int, c: Conds) -> int:
    if (a & M32) < (b & M32):
        c.carry31 += 1
    if a < b:
        c.borrow63 += 1
    return (a - b) & M64


def int32_step(x: int, y: int, a: int, b: int, k: int, c: Conds):
    """One step of int32 on the 64-bit state y:x: t = (a ^ y)(b ^ x) + (mulhi(y, b) : mullo(x, a)) is the
    64-bit multiply-add; the state becomes y:x + t - k, both as 32-bit operations with carry."""
    lo, hi = (x * a) & M32, (y * b) >> 32
    t = ((a ^ y) * (b ^ x) + ((hi << 32) | lo)) & M64
    acc = _sub64(_add64((y << 32) | x, t, c), k, c)
    return acc & M32, acc >> 32


def lane_int32(lane: int, c: Conds) -> list[int]:
    g = "int32"
    x, y = operand(g, 0, lane, 4), operand(g, 0, lane, 5)
    for s in range(STEPS):
        x, y = int32_step(x, y, operand(g, s, lane, 0), operand(g, s, lane, 1),
                          (operand(g, s, lane, 2) << 32) | operand(g, s, lane, 3), c)
    return [x, y]


def int64_step(x: int, k1: int, k2: int, sh: int, c: Conds) -> int:
    """One step of int64: add k1; shift left by sh[5:0] XOR logical right by sh[13:8]; subtract k2;
    arithmetic right by sh[21:16] XOR left by 7."""
    x = _add64(x, k1, c)
    x = ((x << (sh & 63)) & M64) ^ (x >> ((sh >> 8) & 63))
    x = _sub64(x, k2, c)
    signed = x - (1 << 64) if x >> 63 else x
    return ((signed >> ((sh >> 16) & 63)) & M64) ^ ((x << 7) & M64)


def lane_int64(lane: int, c: Conds) -> list[int]:
    g = "int64"
    x = (operand(g, 0, lane, 6) << 32) | operand(g, 0, lane, 7)
    for s in range(STEPS):
        k1 = (operand(g, s, lane, 0) << 32) | operand(g, s, lane, 1)
        k2 = (operand(g, s, lane, 2) << 32) | operand(g, s, lane, 3)
        x = int64_step(x, k1, k2, operand(g, s, lane, 4), c)
    return [x & M32, x >> 32]


def perm(s0: int, s1: int, sel: int) -> int:
    """v_perm_b32 with selectors 0..7: byte i of the result is byte sel_i of (s0 << 32 | s1)."""
    both = (s0 << 32) | s1
    return sum(((both >> (8 * ((sel >> (8 * i)) & 7))) & 0xFF) << (8 * i) for i in range(4))


def bfe_u(v: int, off: int, width: int) -> int:
    return (v >> off) & ((1 << width) - 1)


def bfe_i(v: int, off: int, width: int) -> int:
    f = bfe_u(v, off, width)
    return (f - (1 << width) if f >> (width - 1) else f) & M32


def lane_bits(lane: int, c: Conds) -> list[int]:
    g, out = "bits", []
    for k in range(2):
        x = operand(g, 0, lane, 3 + 4 * k)
        for s in range(STEPS):
            a, sel, u = (operand(g, s, lane, j + 4 * k) for j in range(3))
            p = perm(x, a, sel & 0x07070707)
            e = bfe_u(p, u & 15, 1 + ((u >> 4) & 15))
            sb = bfe_i(p, (u >> 8) & 15, 1 + ((u >> 12) & 15))
            al = (((p << 32) | a) >> ((u >> 16) & 31)) & M32
            cnt = bin(al).count("1") + e
            lowest = al | 0x80000000
            fl = (lowest & -lowest).bit_length() - 1
            fh = 32 - (al | 1).bit_length()
            x = ((al ^ rotl32(sb, 9)) + (cnt << 20) + (fl << 5) + (fh << 27) + x) & M32
        out.append(x)
    return out


def _s8(b: int) -> int:
    return b - 256 if b & 0x80 else b


def udot4(a: int, b: int, acc: int) -> int:
    """v_dot4_u32_u8 without clamp: acc + the four products of unsigned bytes, modulo 2^32."""
    return (acc + sum(((a >> (8 * i)) & 0xFF) * ((b >> (8 * i)) & 0xFF) for i in range(4))) & M32


def sdot4(a: int, b: int, acc: int) -> int:
    """v_dot4_i32_i8 without clamp: the bytes are signed."""
    return (acc + sum(_s8((a >> (8 * i)) & 0xFF) * _s8((b >> (8 * i)) & 0xFF) for i in range(4))) & M32


def lane_dot(lane: int, c: Conds) -> list[int]:
    g, out = "dot", []
    for k in range(2):
        x = operand(g, 0, lane, 3 + 4 * k)
        for s in range(STEPS):
            a, b, d = (operand(g, s, lane, j + 4 * k) for j in range(3))
            x = udot4(a ^ x, b, x)
            x = sdot4(b ^ x, d, x)
        out.append(x)
    return out


def cvt_tie_target(s: int, lane: int) -> int:
    t = (lane + 3 * s) & 7
    return t if t < 5 else -1


def _cvt(x: int, fmt, target: int, c: Conds) -> int:
    code, tie = round_rne(decode(x, F32, c), fmt, c)
    if tie > 0:
        c.tie_up[target] += 1
    if tie < 0:
        c.tie_down[target] += 1
    return code


def lane_cvt(lane: int, c: Conds) -> list[int]:
    g = "cvt"
    h0, h1 = operand(g, 0, lane, 6), operand(g, 0, lane, 7)
    drop = {0: 16, 1: 13, 2: 20, 3: 21}
    for s in range(STEPS):
        u2 = operand(g, s, lane, 2)
        ma, mb = operand(g, s, lane, 0) ^ h0, operand(g, s, lane, 1) ^ h1
        tie = cvt_tie_target(s, lane)
        if tie in drop:
            low, half = (1 << drop[tie]) - 1, 1 << (drop[tie] - 1)
            ma, mb = (ma & ~low) | half, (mb & ~low) | half
        xa, xb = f32_win(ma, u2 % 6 - 2), f32_win(mb, (u2 >> 8) % 6 - 2)
        w_bf = _cvt(xa, BF16, 0, c) | (_cvt(xb, BF16, 0, c) << 16)
        w_h = _cvt(xa, F16, 1, c) | (_cvt(xb, F16, 1, c) << 16)
        w_8 = _cvt(xa, E4M3, 2, c) | (_cvt(xb, E4M3, 2, c) << 8) | (_cvt(xa, E5M2, 3, c) << 16) | (_cvt(xb, E5M2, 3, c) << 24)
        xc = decode(f32_win(operand(g, s, lane, 3) ^ h0, 20 + ((u2 >> 16) & 7)), F32, c)
        ii = math.trunc(xc) & M32                         # toward zero
        mag = ((operand(g, s, lane, 4) ^ ii) & 0x3FFFFFFF) | 0x40000000
        if tie == 4:
            mag = (mag & ~0x7F) | 0x40
        negative = operand(g, s, lane, 5) & 1
        fi, t = round_rne(Fraction(-mag if negative else mag), F32, c)
        if t > 0:
            c.tie_up[4] += 1
        if t < 0:
            c.tie_down[4] += 1
        h0 = rotl32(h0, 5) ^ w_bf ^ rotl32(w_8, 11)
        h1 = rotl32(h1, 7) ^ w_h ^ rotl32(fi, 3) ^ ii
    return [h0, h1]


def xlane_step(x, n: int, read_lane: int, ks) -> list[int]:
    """One cross-lane step on the 64 values x: lane l combines d = x[lane (l - n) mod 16 of its own row of
    16] (DPP row_ror:n), b = x[l ^ 32] (ds_bpermute) and r = x[read_lane] (v_readlane) with its
    operand ks[l] as (d ^ rotl(b, 7)) + rotl(r, 13) + ks[l]."""
    return [((x[(lane & 48) | ((lane - n) & 15)] ^ rotl32(x[lane ^ 32], 7)) + rotl32(x[read_lane], 13) + ks[lane]) & M32
            for lane in range(LANES)]


def xlane_expected() -> list[int]:
    """All 64 lanes in lockstep: lane l reads lane (l - n) mod 16 of its row of 16, lane l ^ 32,
    and one fixed lane."""
    g = "xlane"
    out = [0] * (LANES * 2)
    for k in range(2):
        x = [operand(g, 0, lane, 1 + 4 * k) for lane in range(LANES)]
        for s in range(STEPS):
            x = xlane_step(x, 1 + (s * 5) % 15, (s * 27 + 5) & 63, [operand(g, s, lane, 4 * k) for lane in range(LANES)])
        for lane in range(LANES):
            out[2 * lane + k] = x[lane]
    return out


_LANE = {"fma32": lane_fma32, "fma64": lane_fma64, "pkfma16": lane_pkfma16, "pkfma32": lane_pkfma32,
         "addmul32": lane_addmul32, "int32": lane_int32, "int64": lane_int64, "bits": lane_bits, "dot": lane_dot,
         "cvt": lane_cvt}
_CACHE: dict = {}


def group_expected(group: str):
    """(words, conds) of exact group `group`: its 128 expected words [lane][2] and the counters."""
    if group not in _CACHE:
        c = Conds()
        if group == "xlane":
            words = xlane_expected()
        else:
            words = [w for lane in range(LANES) for w in _LANE[group](lane, c)]
        _CACHE[group] = (words, c)
    return _CACHE[group]


def uncovered_bits(words, w: int) -> int:
    """Bits of word w (0 | 1) that are the same in every lane."""
    ones = zeros = 0
    for lane in range(LANES):
        ones |= words[2 * lane + w]
        zeros |= ~words[2 * lane + w] & M32
    return ~(ones & zeros) & M32


# ---- approx ------------------------------------------------------------------------------------

def approx_input(op: str, lane: int) -> int:
    i = APPROX_OPS.index(op)
    u, v = operand("approx", i, lane, 0), operand("approx", i, lane, 1)
    if op == "exp2":
        return f32_win(u, v % 8 - 4)
    if op == "log2":
        return f32_win(u & 0x7FFFFFFF, 1 + v % 19)
    return f32_win(u & 0x7FFFFFFF, v % 40 - 20)


def bits_float(b: int) -> float:
    return struct.unpack("<f", struct.pack("<I", b))[0]


def float_bits(f: float) -> int:
    return struct.unpack("<I", struct.pack("<f", f))[0]


def ordered_key(bits: int) -> int:
    """A float's bits as an integer ordered like the floats."""
    return (~bits & M32) if bits & 0x80000000 else bits | 0x80000000


def approx_libm(op: str, x: float) -> float:
    return {"exp2": lambda: math.pow(2.0, x) if not hasattr(math, "exp2") else math.exp2(x), "log2": lambda: math.log2(x),
            "rcp": lambda: 1.0 / x, "rsq": lambda: 1.0 / math.sqrt(x), "sqrt": lambda: math.sqrt(x)}[op]()


def approx_center(op: str, lane: int) -> int:
    """The key of the double-precision libm value rounded to f32."""
    return ordered_key(float_bits(approx_libm(op, bits_float(approx_input(op, lane)))))


def approx_ranges() -> list[int]:
    """[op][lane](lo, hi): inclusive, as ordered keys."""
    out = []
    for op in APPROX_OPS:
        for lane in range(LANES):
            c = approx_center(op, lane)
            out += [c - APPROX_ULPS, c + APPROX_ULPS]
    return out


def approx_ulp_distance(op: str, lane: int, value: float) -> int:
    return abs(ordered_key(float_bits(value)) - approx_center(op, lane))


def reg_word(slot: int, thread: int, seed: int, pass_: int = 0) -> int:
    v = mix32(((slot << 8) | thread) ^ seed)
    return v ^ M32 if pass_ else v


# ---- folding -----------------------------------------------------------------------------------

def fold_valu(records, groups, expected_cus) -> dict:
    """Folds `cu_sweep_valu` records `(xcc, hw_id, fail, simds, group_bits, bad_slot, bad_thread,
    approx_hash)` by CU; `groups` names the bits of `group_bits` in order. `failed` maps each
    failed exact group, `regs`, `approx` or `record` (a garbled record) to its `[xcc, cu_key]`
    list; `cus` lists per failed CU its kinds, the waves (bit w: wave w) that saw any failure and
    the first bad register slot with its wave and lane (-1: none). The approx reference is the
    hash a strict majority of the records hold: a CU with a record holding another, or with a
    wave unlike its wave 0, or over the bound, fails `approx`; without a strict majority every
    CU does. `uncovered` / `cus_uncovered` as in `fold_sweep`: not a failure."""
    groups = list(groups)
    n_exact = len([g for g in groups if g not in ("approx", "regs")])
    records = [tuple(r) for r in records]
    counts: dict[int, int] = {}
    for r in records:
        counts[r[7]] = counts.get(r[7], 0) + 1
    majority = next((h for h, n in counts.items() if 2 * n > len(records)), None)
    cus = by_cu(records)
    failures = []
    for k, visits in sorted(cus.items()):
        found, waves, slot, thread = set(), 0, -1, -1
        for fail, _simds, gbits, s, t, ahash in visits:
            if fail >> 16 or gbits >> n_exact or bool(fail & FAIL_EXACT) != bool(gbits) or bool(fail & FAIL_REGS) != (s >= 0):
                found.add("record")
            found.update(groups[i] for i in range(n_exact) if gbits >> i & 1)
            if fail & FAIL_REGS:
                found.add("regs")
                if s >= 0 and (slot < 0 or (s, t) < (slot, thread)):
                    slot, thread = s, t
            if fail & (FAIL_BOUND | FAIL_HASH) or ahash != majority:
                found.add("approx")
            if ahash != majority and not fail & (FAIL_BOUND | FAIL_HASH):
                waves |= 0xF
            waves |= (fail | fail >> 4 | fail >> 8 | fail >> 12) & 0xF
        if found:
            kinds = [n for n in groups + ["record"] if n in found]
            failures.append((k, kinds, {"kinds": kinds, "waves": waves, "bad_slot": slot,
                                        "bad_wave": thread >> 6 if thread >= 0 else -1,
                                        "bad_lane": thread & 63 if thread >= 0 else -1}))
    return dict(named_failures(cus, expected_cus, failures), approx_hash=majority,
                simds_seen_min=simds_seen_min(cus, 1))


PART = Part(
    key="valu", names=GROUPS, noun="vector-ALU group", flag_noun="group", binding="cu_sweep_valu", names_key="groups",
    fold=fold_valu, kept=("cus", "reg_slots", "ms"), label="vector ALU", detail=" ({reg_slots} registers a lane, {ms:.3f} ms)",
    clauses=lambda d: [f"vector ALU {'+'.join(c['kinds'])} on CU (xcc {c['xcc']}, key {c['cu_key']:#x})"
                       + (f" at slot {c['bad_slot']}, wave {c['bad_wave']} lane {c['bad_lane']}" if c["bad_slot"] >= 0 else "")
                       for c in d.get("cus", [])],
    note_missing="this probe has no cu_sweep_valu: no vector-ALU group was checked",
    note_unreached="{n} CUs not reached by the vector-ALU launches",
    help="vector-ALU groups, 'approx' and 'regs' every CU also runs: 'all' or a comma-separated list",
    agent_help="the deep self-test also runs, on all four SIMDs of every CU, exact chains of vector-ALU "
               "instructions, the transcendentals and a pattern test of the vector register file: 'all' or a "
               "comma-separated list of fma32, fma64, pkfma16, pkfma32, addmul32, int32, int64, bits, dot, "
               "cvt, xlane, approx, regs (implies --selftest-deep; start-up and periodic runs alike)",
    metric_help="vector-ALU groups (with approx and regs) the last deep self-test ran on every CU")


def twin_summary() -> dict:
    """What the stand-alone host program prints, from this module: per exact group its checksum and
    counters, and the approx ranges' checksum."""
    out = {}
    for g in EXACT_GROUPS:
        words, c = group_expected(g)
        out[g] = dict(c.to_dict(), checksum=tile_checksum(words))
    return {"groups": out, "approx_checksum": tile_checksum([w & M32 for w in approx_ranges()]),
            "reg_slots": REG_SLOTS, "record_words": RECORD_WORDS}
