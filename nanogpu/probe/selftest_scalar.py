"""Scalar part of the deep self-test: the Python twin of native/include/nanogpu/selftest_scalar_host.h.

`cu_sweep_scalar` (native/hip/probe_scalar.inc) makes all four waves of every CU run exact chains of
scalar-ALU instructions (`EXACT_GROUPS`: add, mul, shift, logic, bits, cmp and the vector / scalar
boundary vcc), scalar loads of a read-only table (`smem`) and a pattern test of the wave's scalar
registers (`sregs`). This module computes what the exact groups must give, in plain Python integers:
one function per instruction, returning `(result, SCC)` where the instruction writes SCC, each
written from the instruction's definition in the CDNA ISA and not from a device's output. It also
folds the records by CU (`fold_scalar`).

Operand corners whose definition is not established independently are kept out of the chains (the
functions raise on them) and are listed under "Not covered" in the README: equal operands of
s_min / s_max, a magnitude of 2^31 in s_abs_i32 / s_absdiff_i32, a bit shifted out of S0 in
s_lshlN_add_u32, counts beyond the operand's width, extracts that run past the top bit or have
width 0, and find-first / find-leading-bit of an operand without the bit sought.
"""
from __future__ import annotations

from .selftest_common import (HI_MUL, M32, M64, Part, by_cu, mix32, named_failures, parse_names, rotl32, simds_seen_min,
                              tile_checksum)

GROUPS = ("add", "mul", "shift", "logic", "bits", "cmp", "vcc", "smem", "sregs")   # bit order of the records
NUM_EXACT = 7
EXACT_GROUPS = GROUPS[:NUM_EXACT]
WAVES = 4
WAVE_WORDS = 8
LANES = 64
SREG_SLOTS = 88
SREG_FIRST = 12
SMEM_WORDS = 4096
SMEM_SALT = 0x51ED270B
RECORD_WORDS = 8
ZERO_STEP, EQUAL_STEP = 5, 2
# fail bits, by wave: exact groups, scalar loads, scalar registers
FAIL_EXACT, FAIL_SMEM, FAIL_SREGS = 0xF, 0xF0, 0xF00
BAD_SREGS, BAD_SMEM = 0, 1


def parse_scalar(spec) -> list[str]:
    """`parse_names` over `GROUPS`: None / "" -> [], "all", "a,b" or a list of names; ValueError on an unknown one."""
    return parse_names(spec, GROUPS, "scalar group")


def operand(group: str, s: int, wave: int, k: int) -> int:
    return mix32(0x5CA1A2B3 ^ (GROUPS.index(group) << 24) ^ (s << 16) ^ (wave << 8) ^ k)


def fold(h: int, d: int, c: int) -> int:
    return (rotl32(h ^ d, 7) + c + 0x9E3779B9) & M32


def fold64(h: int, d: int, c: int) -> int:
    return fold(fold(h, d & M32, c), d >> 32, 0)


def s32(v: int) -> int:
    return v - (1 << 32) if v >> 31 else v


def s64(v: int) -> int:
    return v - (1 << 64) if v >> 63 else v


class Conds:
    """The header's condition counters, over one group."""

    def __init__(self):
        self.scc: dict[str, list[int]] = {}     # instruction -> times its SCC was consumed as [0, 1]
        self.carry31, self.carry63, self.borrow31, self.borrow63 = [0, 0], [0, 0], [0, 0], [0, 0]
        self.overflow_pos = self.overflow_neg = self.equal_operands = 0

    def note(self, name: str, scc) -> int:
        scc = int(bool(scc))
        self.scc.setdefault(name, [0, 0])[scc] += 1
        return scc


_NONE = Conds()     # the counters of calls made without one


# ---- add ---------------------------------------------------------------------------------------
def s_add_u32(a, b, c=_NONE, cin=None):
    """D = S0 + S1 (s_addc_u32 with `cin`: + SCC); SCC = the carry out of bit 31."""
    r = a + b + (cin or 0)
    return r & M32, c.note("add_u32" if cin is None else "addc_u32", r >> 32)


def s_sub_u32(a, b, c=_NONE, bin_=None):
    """D = S0 - S1 (s_subb_u32 with `bin_`: - SCC); SCC = the unsigned borrow."""
    r = a - b - (bin_ or 0)
    return r & M32, c.note("sub_u32" if bin_ is None else "subb_u32", r < 0)


def add64(a, b, c=_NONE):
    """s_add_u32 of the low words, s_addc_u32 of the high words."""
    lo, c0 = s_add_u32(a & M32, b & M32, c)
    hi, c1 = s_add_u32(a >> 32, b >> 32, c, cin=c0)
    c.carry31[c0] += 1
    c.carry63[c1] += 1
    return (hi << 32) | lo, c1


def sub64(a, b, c=_NONE):
    """s_sub_u32 of the low words, s_subb_u32 of the high words."""
    lo, c0 = s_sub_u32(a & M32, b & M32, c)
    hi, c1 = s_sub_u32(a >> 32, b >> 32, c, bin_=c0)
    c.borrow31[c0] += 1
    c.borrow63[c1] += 1
    return (hi << 32) | lo, c1


def _signed(name, r, c):
    over = not -(1 << 31) <= r < (1 << 31)
    if r >= 1 << 31:
        c.overflow_pos += 1
    if r < -(1 << 31):
        c.overflow_neg += 1
    return r & M32, c.note(name, over)


def s_add_i32(a, b, c=_NONE):
    """D = S0 + S1; SCC = signed overflow."""
    return _signed("add_i32", s32(a) + s32(b), c)


def s_sub_i32(a, b, c=_NONE):
    """D = S0 - S1; SCC = signed overflow."""
    return _signed("sub_i32", s32(a) - s32(b), c)


def _minmax(name, a, b, first, c):
    if a == b:
        raise ValueError(f"s_{name} with equal operands is left out")
    scc = c.note(name, first)
    return (a if scc else b), scc


def s_min_i32(a, b, c=_NONE):
    """D = the smaller, signed; SCC = 1 when that is S0."""
    return _minmax("min_i32", a, b, s32(a) < s32(b), c)


def s_max_i32(a, b, c=_NONE):
    return _minmax("max_i32", a, b, s32(a) > s32(b), c)


def s_min_u32(a, b, c=_NONE):
    return _minmax("min_u32", a, b, a < b, c)


def s_max_u32(a, b, c=_NONE):
    return _minmax("max_u32", a, b, a > b, c)


def s_absdiff_i32(a, b, c=_NONE):
    """D = |S0 - S1|, signed; SCC = D != 0."""
    d = abs(s32(a) - s32(b))
    if d >= 1 << 31:
        raise ValueError("s_absdiff_i32 whose difference overflows is left out")
    return d, c.note("absdiff_i32", d != 0)


def s_abs_i32(a, c=_NONE):
    """D = |S0|; SCC = D != 0."""
    if a == 0x80000000:
        raise ValueError("s_abs_i32 of -2^31 is left out")
    d = abs(s32(a))
    return d, c.note("abs_i32", d != 0)


# ---- mul ---------------------------------------------------------------------------------------
def s_mul_i32(a, b):
    return (a * b) & M32


def s_mul_hi_u32(a, b):
    return (a * b) >> 32


def s_mul_hi_i32(a, b):
    return ((s32(a) * s32(b)) >> 32) & M32


def s_lshl_add_u32(n, a, b, c=_NONE):
    """s_lshlN_add_u32: D = (S0 << N) + S1; SCC = the carry out of bit 31."""
    if a >> (32 - n):
        raise ValueError("s_lshlN_add_u32 with a bit shifted out of S0 is left out")
    r = (a << n) + b
    return r & M32, c.note(f"lshl{n}_add_u32", r >> 32)


# ---- shift -------------------------------------------------------------------------------------
def _count(n, bits):
    if not 0 <= n < bits:
        raise ValueError("a count beyond the operand's width is left out")
    return n


def s_lshl(a, n, bits=32, c=_NONE):
    """s_lshl_b32 / _b64: D = S0 << S1; SCC = D != 0."""
    d = (a << _count(n, bits)) & ((1 << bits) - 1)
    return d, c.note(f"lshl_b{bits}", d != 0)


def s_lshr(a, n, bits=32, c=_NONE):
    d = a >> _count(n, bits)
    return d, c.note(f"lshr_b{bits}", d != 0)


def s_ashr(a, n, bits=32, c=_NONE):
    """s_ashr_i32 / _i64: the sign fills."""
    signed = s32(a) if bits == 32 else s64(a)
    d = (signed >> _count(n, bits)) & ((1 << bits) - 1)
    return d, c.note(f"ashr_i{bits}", d != 0)


def s_bfm(width, off, bits=32):
    """s_bfm_b32 / _b64: D = ((1 << S0) - 1) << S1."""
    return (((1 << _count(width, bits)) - 1) << _count(off, bits)) & ((1 << bits) - 1)


def shift_amount32(s, u):
    return (0, 1, 31)[s] if s < 3 else u & 31


def shift_amount64(s, u):
    return (0, 31, 32, 63)[s] if s < 4 else (u >> 8) & 63


# ---- logic -------------------------------------------------------------------------------------
LOGIC = {"and": lambda a, b, m: a & b, "or": lambda a, b, m: a | b, "xor": lambda a, b, m: a ^ b,
         "nand": lambda a, b, m: ~(a & b) & m, "nor": lambda a, b, m: ~(a | b) & m, "xnor": lambda a, b, m: ~(a ^ b) & m,
         "andn2": lambda a, b, m: a & ~b & m, "orn2": lambda a, b, m: (a | ~b) & m}


def s_logic(name, a, b, bits=32, c=_NONE):
    """s_<name>_b32 / _b64; SCC = D != 0. andn2 is S0 & ~S1, orn2 S0 | ~S1."""
    d = LOGIC[name](a, b, (1 << bits) - 1)
    return d, c.note(f"{name}_b{bits}", d != 0)


def s_not(a, bits=32, c=_NONE):
    d = ~a & ((1 << bits) - 1)
    return d, c.note(f"not_b{bits}", d != 0)


# ---- bits --------------------------------------------------------------------------------------
def s_bfe(v, field, bits=32, signed=False, c=_NONE):
    """s_bfe_{u,i}{32,64}: offset = S1[4:0] (64 bits: [5:0]), width = S1[22:16]; SCC = D != 0."""
    off, width = field & (bits - 1), (field >> 16) & 0x7F
    if width == 0 or off + width > bits:
        raise ValueError("an extract of width 0 or past the top bit is left out")
    f = (v >> off) & ((1 << width) - 1)
    if signed and f >> (width - 1):
        f -= 1 << width
    d = f & ((1 << bits) - 1)
    return d, c.note(f"bfe_{'i' if signed else 'u'}{bits}", d != 0)


def bfe_field32(u):
    off = u & 31
    return off | ((1 + (u >> 8) % (32 - off)) << 16)


def bfe_field64(u):
    off = (u >> 16) & 63
    return off | ((1 + (u >> 24) % (64 - off)) << 16)


def s_brev(v, bits=32):
    return int(format(v, f"0{bits}b")[::-1], 2)


def s_bcnt(v, bit, bits=32, c=_NONE):
    """s_bcnt0 / s_bcnt1 _i32_b32 / _b64: the number of `bit`s; SCC = D != 0."""
    ones = bin(v).count("1")
    d = ones if bit else bits - ones
    return d, c.note(f"bcnt{bit}_i32_b{bits}", d != 0)


def _first(v, bits, bit, from_top):
    order = range(bits - 1, -1, -1) if from_top else range(bits)
    for n, k in enumerate(order):
        if (v >> k) & 1 == bit:
            return n
    raise ValueError("a search of an operand without the bit sought is left out")


def s_ff(v, bit, bits=32):
    """s_ff0 / s_ff1 _i32_b32 / _b64: the position of the first `bit` from bit 0."""
    return _first(v, bits, bit, False)


def s_flbit(v, bits=32, signed=False):
    """s_flbit_i32_b32 / _b64: leading zeros. s_flbit_i32 / _i64: how many bits from the top equal the sign."""
    return _first(v, bits, (v >> (bits - 1)) ^ 1 if signed else 1, True)


def s_bitset(d, n, bit):
    """s_bitset0 / s_bitset1 _b32: D[S0[4:0]] = bit."""
    return d & ~(1 << _count(n, 32)) & M32 if not bit else d | (1 << _count(n, 32))


def s_sext(a, bits):
    f = a & ((1 << bits) - 1)
    return (f - (1 << bits) if f >> (bits - 1) else f) & M32


def s_pack(kind, a, b):
    """s_pack_{ll,lh,hh}_b32_b16: the low half from S0, the high half from S1; l / h the half each one gives."""
    lo = a & 0xFFFF if kind[0] == "l" else a >> 16
    hi = b & 0xFFFF if kind[1] == "l" else b >> 16
    return lo | (hi << 16)


# ---- cmp ---------------------------------------------------------------------------------------
CMP32 = {"eq_i32": lambda a, b: a == b, "lg_i32": lambda a, b: a != b, "gt_i32": lambda a, b: s32(a) > s32(b),
         "ge_i32": lambda a, b: s32(a) >= s32(b), "lt_i32": lambda a, b: s32(a) < s32(b), "le_i32": lambda a, b: s32(a) <= s32(b),
         "eq_u32": lambda a, b: a == b, "lg_u32": lambda a, b: a != b, "gt_u32": lambda a, b: a > b, "ge_u32": lambda a, b: a >= b,
         "lt_u32": lambda a, b: a < b, "le_u32": lambda a, b: a <= b,
         "bitcmp0_b32": lambda a, b: (a >> (b & 31)) & 1 == 0, "bitcmp1_b32": lambda a, b: (a >> (b & 31)) & 1 == 1}
CMP64 = {"eq_u64": lambda a, b: a == b, "lg_u64": lambda a, b: a != b}


def s_cmp(name, a, b, x, y, how="sel", c=_NONE):
    """s_cmp_<name> (or s_bitcmp) consumed by a select (`how` "sel": s_cselect / s_cmov) or by a branch over one
    s_mov_b32 ("br"): either way SCC ? x : y."""
    scc = c.note(f"{how}_{name}", (CMP32.get(name) or CMP64[name])(a, b))
    if a == b:
        c.equal_operands += 1
    return x if scc else y


# ---- the chains --------------------------------------------------------------------------------
def _p64(hi, lo):
    return (hi << 32) | lo


def chain_add(wave, c):
    g, out = "add", []
    h = operand(g, 0, wave, 15)
    for s in range(WAVE_WORDS):
        a, p, q = operand(g, s, wave, 0), operand(g, s, wave, 2), operand(g, s, wave, 3)
        b = a if s == ZERO_STEP else operand(g, s, wave, 1)
        h = fold(h, *s_add_u32(a, b, c))
        h = fold(h, *s_sub_u32(a, b, c))
        h = fold64(h, *add64(_p64(a, p), _p64(b, q), c))
        h = fold64(h, *sub64(_p64(p, a), _p64(q, b), c))
        h = fold(h, *s_add_i32(a, b, c))
        h = fold(h, *s_sub_i32(p, b, c))
        h = fold(h, *s_min_i32(a, p, c))
        h = fold(h, *s_max_i32(a, p, c))
        h = fold(h, *s_min_u32(q, a, c))
        h = fold(h, *s_max_u32(q, a, c))
        ha, hb = (s32(a) >> 1) & M32, (s32(b) >> 1) & M32
        h = fold(h, *s_absdiff_i32(ha, hb, c))
        h = fold(h, *s_abs_i32(0 if s == ZERO_STEP else ha, c))
        out.append(h)
    return out


def chain_mul(wave, c):
    g, out = "mul", []
    h = operand(g, 0, wave, 15)
    for s in range(WAVE_WORDS):
        a, b, p = (operand(g, s, wave, k) for k in range(3))
        h = fold(h, s_mul_i32(a, b), 0)
        h = fold(h, s_mul_hi_u32(a, b), 0)
        h = fold(h, s_mul_hi_i32(a, b), 0)
        h = fold(h, s_mul_hi_i32(p, a), 0)
        h = fold(h, *s_lshl_add_u32(1, a >> 1, p, c))
        h = fold(h, *s_lshl_add_u32(2, b >> 2, p, c))
        h = fold(h, *s_lshl_add_u32(3, p >> 3, a, c))
        h = fold(h, *s_lshl_add_u32(4, a >> 4, b, c))
        out.append(h)
    return out


def chain_shift(wave, c):
    g, out = "shift", []
    h = operand(g, 0, wave, 15)
    for s in range(WAVE_WORDS):
        z = s == ZERO_STEP
        a, b = (0 if z else operand(g, s, wave, k) for k in range(2))
        u, v = operand(g, s, wave, 2), operand(g, s, wave, 3)
        n, m, x = shift_amount32(s, u), shift_amount64(s, u), _p64(a, b)
        h = fold(h, *s_lshl(a, n, 32, c))
        h = fold(h, *s_lshr(a, n, 32, c))
        h = fold(h, *s_ashr(a, n, 32, c))
        h = fold64(h, *s_lshl(x, m, 64, c))
        h = fold64(h, *s_lshr(x, m, 64, c))
        h = fold64(h, *s_ashr(x, m, 64, c))
        h = fold(h, s_bfm(v & 31, (v >> 8) & 31), 0)
        h = fold64(h, s_bfm((v >> 16) & 63, (v >> 24) & 63, 64), 0)
        out.append(h)
    return out


def _logic_operands(name, a, b, z, ones):
    """The operands of one logic instruction: (a, b), or at the zero step a pair whose result is 0."""
    if not z:
        return a, b
    return {"and": (a, a ^ ones), "or": (0, 0), "xor": (a, a), "nand": (ones, ones), "nor": (a, a ^ ones),
            "xnor": (a, a ^ ones), "andn2": (a, a), "orn2": (0, ones)}[name]


def chain_logic(wave, c):
    g, out = "logic", []
    h = operand(g, 0, wave, 15)
    for s in range(WAVE_WORDS):
        z = s == ZERO_STEP
        a, b = operand(g, s, wave, 0), operand(g, s, wave, 1)
        x, y = _p64(operand(g, s, wave, 2), a), _p64(operand(g, s, wave, 3), b)
        for name in LOGIC:
            h = fold(h, *s_logic(name, *_logic_operands(name, a, b, z, M32), 32, c))
        h = fold(h, *s_not(M32 if z else a, 32, c))
        for name in LOGIC:
            h = fold64(h, *s_logic(name, *_logic_operands(name, x, y, z, M64), 64, c))
        h = fold64(h, *s_not(M64 if z else y, 64, c))
        out.append(h)
    return out


def chain_bits(wave, c):
    g, out = "bits", []
    h = operand(g, 0, wave, 15)
    for s in range(WAVE_WORDS):
        z = s == ZERO_STEP
        a, b = (0 if z else operand(g, s, wave, k) for k in range(2))
        u, p = operand(g, s, wave, 2), operand(g, s, wave, 3)
        x = _p64(a, b)
        h = fold(h, *s_bfe(a, bfe_field32(u), 32, False, c))
        h = fold(h, *s_bfe(a, bfe_field32(p), 32, True, c))
        h = fold64(h, *s_bfe(x, bfe_field64(u), 64, False, c))
        h = fold64(h, *s_bfe(x, bfe_field64(p), 64, True, c))
        h = fold(h, s_brev(a), 0)
        h = fold64(h, s_brev(x, 64), 0)
        h = fold(h, *s_bcnt(a ^ M32, 0, 32, c))
        h = fold(h, *s_bcnt(a, 1, 32, c))
        h = fold(h, *s_bcnt(x ^ M64, 0, 64, c))
        h = fold(h, *s_bcnt(x, 1, 64, c))
        h = fold(h, s_ff(a & 0x7FFFFFFF, 0), 0)
        h = fold(h, s_ff(a | 0x80000000, 1), 0)
        h = fold(h, s_ff(x & ~(1 << 63) & M64, 0, 64), 0)
        h = fold(h, s_ff(x | 1 << 63, 1, 64), 0)
        h = fold(h, s_flbit(a | 1), 0)
        h = fold(h, s_flbit(x | 1, 64), 0)
        h = fold(h, s_flbit((a & ~1 & M32) | ((a ^ M32) >> 31), 32, True), 0)
        h = fold(h, s_flbit((x & ~1 & M64) | ((x ^ M64) >> 63), 64, True), 0)
        h = fold(h, s_bitset(p, u & 31, 0), 0)
        h = fold(h, s_bitset(p, (u >> 8) & 31, 1), 0)
        h = fold(h, s_sext(p, 8), 0)
        h = fold(h, s_sext(u, 16), 0)
        for kind in ("ll", "lh", "hh"):
            h = fold(h, s_pack(kind, p, u), 0)
        out.append(h)
    return out


def chain_cmp(wave, c):
    g, out = "cmp", []
    h = operand(g, 0, wave, 15)
    for s in range(WAVE_WORDS):
        eq = s == EQUAL_STEP
        a = operand(g, s, wave, 0)
        b = a if eq else operand(g, s, wave, 1)
        x, y, ah = operand(g, s, wave, 2), operand(g, s, wave, 3), operand(g, s, wave, 4)
        bh = ah if eq or s & 1 else operand(g, s, wave, 5)
        for name in CMP32:
            h = fold(h, s_cmp(name, a, b, x, y, "sel", c), 0)
            h = fold(h, s_cmp(name, b, a, y, x, "br", c), 0)
        for name in CMP64:
            h = fold(h, s_cmp(name, _p64(ah, a), _p64(bh, b), x, y, "sel", c), 0)
            h = fold(h, s_cmp(name, _p64(a, ah), _p64(b, bh), y, x, "br", c), 0)
        out.append(h)
    return out


def vcc_lane_value(u0: int, lane: int) -> int:
    return mix32(u0 ^ (lane * HI_MUL & M32))


def vcc_step(h: int, u0: int, thr: int, m: int, k: int) -> int:
    """One step of the vcc group on the wave's 64 lanes, lane l holding v = vcc_lane_value(u0, l): mask = the lanes
    with v < thr, counted and searched (the search on mask | 2^63); lane 0's v ^ h through readfirstlane; w = v + k
    where bit l of m is set, else v ^ k; mask2 = the lanes with w < k."""
    v = [vcc_lane_value(u0, lane) for lane in range(LANES)]
    mask = sum(1 << lane for lane in range(LANES) if v[lane] < thr)
    w = [(v[lane] + k) & M32 if (m >> lane) & 1 else v[lane] ^ k for lane in range(LANES)]
    mask2 = sum(1 << lane for lane in range(LANES) if w[lane] < k)
    first = v[0] ^ h                      # h as the step found it
    h = fold(h, mask & M32, bin(mask).count("1"))
    h = fold(h, mask >> 32, s_ff(mask | 1 << 63, 1, 64))
    h = fold(h, first, 0)
    return fold64(h, mask2, 0)


def chain_vcc(wave, c):
    g, out = "vcc", []
    h = operand(g, 0, wave, 15)
    for s in range(WAVE_WORDS):
        h = vcc_step(h, operand(g, s, wave, 0), operand(g, s, wave, 1), _p64(operand(g, s, wave, 3), operand(g, s, wave, 2)),
                     operand(g, s, wave, 4))
        out.append(h)
    return out


_CHAIN = {"add": chain_add, "mul": chain_mul, "shift": chain_shift, "logic": chain_logic, "bits": chain_bits,
          "cmp": chain_cmp, "vcc": chain_vcc}
_CACHE: dict = {}


def group_expected(group: str):
    """(words, conds) of exact group `group`: its 32 expected words [wave][8] and the counters."""
    if group not in _CACHE:
        c = Conds()
        _CACHE[group] = ([w for wave in range(WAVES) for w in _CHAIN[group](wave, c)], c)
    return _CACHE[group]


def uncovered_bits(words) -> int:
    """Bits that are the same in every word."""
    ones = zeros = 0
    for w in words:
        ones |= w
        zeros |= ~w & M32
    return ~(ones & zeros) & M32


def smem_word(index: int) -> int:
    return mix32(index ^ SMEM_SALT)


def sreg_word(slot: int, key: int, pass_: int = 0) -> int:
    """What register s(12 + slot) holds: key * odd_slot ^ c_slot with key = seed ^ wave; pass 1 holds the complement."""
    v = ((key * (0x9E3779B1 + 2 * slot)) & M32) ^ ((0x7F4A7C15 + 0x01000193 * slot) & M32)
    return v ^ M32 if pass_ else v


# ---- folding -----------------------------------------------------------------------------------
def fold_scalar(records, groups, expected_cus) -> dict:
    """Folds `cu_sweep_scalar` records `(xcc, hw_id, fail, simds, group_bits, bad_index, bad_wave, bad_which)` by
    CU; `groups` names the bits of `group_bits` in order. `failed` maps each failed exact group, `smem`, `sregs` or
    `record` (a garbled record) to its `[xcc, cu_key]` list; `cus` lists per failed CU its kinds, the waves (bit w:
    wave w) that saw any failure, and the first bad register slot and the first bad table word with their waves
    (-1: none). `uncovered` / `cus_uncovered` as in `fold_sweep`: not a failure."""
    groups = list(groups)
    n_exact = len([g for g in groups if g not in ("smem", "sregs")])
    cus = by_cu([tuple(r) for r in records])
    failures = []
    for k, visits in sorted(cus.items()):
        found, waves = set(), 0
        first = {BAD_SREGS: (-1, -1), BAD_SMEM: (-1, -1)}
        for fail, _simds, gbits, index, wave, which in visits:
            located = fail & (FAIL_SREGS | FAIL_SMEM)
            if (fail >> 12 or gbits >> n_exact or bool(fail & FAIL_EXACT) != bool(gbits) or bool(located) != (index >= 0)
                    or (index >= 0 and (which not in first or not 0 <= wave < WAVES or not fail & (FAIL_SMEM, FAIL_SREGS)[which == BAD_SREGS]))):
                found.add("record")
            found.update(groups[i] for i in range(n_exact) if gbits >> i & 1)
            if fail & FAIL_SMEM:
                found.add("smem")
            if fail & FAIL_SREGS:
                found.add("sregs")
            if index >= 0 and which in first and (first[which][0] < 0 or (index, wave) < first[which]):
                first[which] = (index, wave)
            waves |= (fail | fail >> 4 | fail >> 8) & 0xF
        if found:
            kinds = [n for n in groups + ["record"] if n in found]
            failures.append((k, kinds, {"kinds": kinds, "waves": waves, "bad_slot": first[BAD_SREGS][0],
                                        "bad_slot_wave": first[BAD_SREGS][1], "bad_word": first[BAD_SMEM][0],
                                        "bad_word_wave": first[BAD_SMEM][1]}))
    return dict(named_failures(cus, expected_cus, failures), simds_seen_min=simds_seen_min(cus, 1))


PART = Part(
    key="scalar", names=GROUPS, noun="scalar group", flag_noun="group", binding="cu_sweep_scalar", names_key="groups",
    fold=fold_scalar, kept=("cus", "sreg_slots", "ms"), label="scalar unit", detail=" ({sreg_slots} registers a wave, {ms:.3f} ms)",
    clauses=lambda d: [f"scalar unit {'+'.join(c['kinds'])} on CU (xcc {c['xcc']}, key {c['cu_key']:#x})"
                       + (f", at slot {c['bad_slot']}, wave {c['bad_slot_wave']}" if c["bad_slot"] >= 0 else "")
                       + (f", at word {c['bad_word']}, wave {c['bad_word_wave']}" if c["bad_word"] >= 0 else "")
                       for c in d.get("cus", [])],
    note_missing="this probe has no cu_sweep_scalar: no scalar group was checked",
    note_unreached="{n} CUs not reached by the scalar launches",
    help="scalar-ALU groups, 'vcc', 'smem' and 'sregs' every CU also runs: 'all' or a comma-separated list",
    agent_help="the deep self-test also runs, on all four waves of every CU, exact chains of scalar-ALU "
               "instructions, the vector / scalar boundary, scalar loads of every width and a pattern test of the "
               "wave's scalar registers: 'all' or a comma-separated list of add, mul, shift, logic, bits, cmp, "
               "vcc, smem, sregs (implies --selftest-deep; start-up and periodic runs alike)",
    metric_help="scalar groups (with smem and sregs) the last deep self-test ran on every CU")


def twin_summary() -> dict:
    """What the stand-alone host program prints, from this module."""
    return {"groups": {g: group_expected(g)[0] for g in EXACT_GROUPS},
            "smem_checksum": tile_checksum([smem_word(i) for i in range(SMEM_WORDS)]), "smem_words": SMEM_WORDS,
            "sreg_slots": SREG_SLOTS, "record_words": RECORD_WORDS}
