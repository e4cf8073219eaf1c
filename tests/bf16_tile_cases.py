"""What tests/test_basic_selftest.py (host) and tests/test_gpu_basic_selftest.py (device) share: a model
of the probe's `mfma_tile` kernel with pluggable lane maps, exact bf16 arithmetic in integers, the
one-term tiles that put every bf16 code through `gemm_tile`, the tiles that reach the host's rounding,
and a reference of `mfma_burn`'s sums. No test in here, and nothing that needs a GPU."""
import struct

import numpy as np

# ---------------------------------------------------------------------------------------------- bf16

SCALE_BITS = 133          # every finite bf16 value is an integer multiple of 2^-133


def bf16_code(x: float) -> int:
    """The code of a float that is a bf16 value."""
    w = struct.unpack("<I", struct.pack("<f", x))[0]
    assert w & 0xFFFF == 0 and struct.unpack("<f", struct.pack("<I", w))[0] == x, x
    return w >> 16


def bf16_value(code: int) -> float:
    return struct.unpack("<f", struct.pack("<I", code << 16))[0]


def f32_word(x: float) -> int:
    """The fp32 bit pattern of a float that is an fp32 value."""
    w = struct.unpack("<I", struct.pack("<f", x))[0]
    assert struct.unpack("<f", struct.pack("<I", w))[0] == x or x != x, x
    return w


def bf16_scaled(code: int):
    """A finite code's value as an integer count of 2^-133; None for Inf and NaN."""
    e, m = (code >> 7) & 0xFF, code & 0x7F
    if e == 0xFF:
        return None
    n = m if e == 0 else (128 + m) << (e - 1)
    return -n if code & 0x8000 else n


def round_to_f32(n: int, scale_bits: int) -> float:
    """n * 2^-scale_bits rounded to fp32, nearest even, in integer arithmetic: to 24 bits, or to a
    multiple of 2^-149 where that is coarser (the subnormal range)."""
    if n == 0:
        return 0.0
    sign, n = (-1.0 if n < 0 else 1.0), abs(n)
    shift = max(n.bit_length() - 24, scale_bits - 149, 0)
    q = n
    if shift > 0:
        q, rem = n >> shift, n & ((1 << shift) - 1)
        half = 1 << (shift - 1)
        q += int(rem > half or (rem == half and q & 1 == 1))
    if q.bit_length() + shift - scale_bits > 128:
        return sign * float("inf")
    return sign * float(np.ldexp(float(q), shift - scale_bits))


# ------------------------------------------------------------------------------------- kernel model
# mfma_tile: lane l gives the instruction a[j] = A[a_map(l, j)] and b[j] = B[b_map(l, j)] and stores its
# accumulator `reg` to C[c_map(l, reg)]. The instruction itself is fixed: a[j] of lane l is its operand
# A'[l & 31][8 (l >> 5) + j], b[j] is B'[8 (l >> 5) + j][l & 31], and accumulator `reg` of lane l is
# D[(reg & 3) + 8 (reg >> 2) + 4 (l >> 5)][l & 31] of D = A' B'. The maps take numpy arrays.

def faithful_a(lane, j):
    return lane & 31, 8 * (lane >> 5) + j


def faithful_b(lane, j):
    return 8 * (lane >> 5) + j, lane & 31


def faithful_c(lane, reg):
    return (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5), lane & 31


_LANE = np.arange(64)[:, None]
_J = np.arange(8)[None, :]
_REG = np.arange(16)[None, :]


def _flat(first, second, width, shape):
    first, second = np.broadcast_arrays(np.asarray(first), np.asarray(second))
    return np.broadcast_to(first * width + second, shape)


def c_map_is_bijection(c_map) -> bool:
    row, col = c_map(_LANE, _REG)
    flat = _flat(row, col, 32, (64, 16))
    return bool(((flat >= 0) & (flat < 1024)).all()) and len(set(flat.ravel().tolist())) == 1024


def model_tile(a, b, a_map=faithful_a, b_map=faithful_b, c_map=faithful_c) -> list:
    """C as the kernel with these maps leaves it, in exact integer arithmetic: a and b are the flat
    operands, integers (as ints or floats). c_map must be a bijection onto the 1,024 places."""
    a = np.array([int(v) for v in a], dtype=np.int64)
    b = np.array([int(v) for v in b], dtype=np.int64)
    assert a.shape == (512,) and b.shape == (512,)
    a_op = np.zeros((32, 16), dtype=np.int64)
    b_op = np.zeros((16, 32), dtype=np.int64)
    a_op[np.broadcast_to(_LANE & 31, (64, 8)), 8 * (_LANE >> 5) + _J] = a[_flat(*a_map(_LANE, _J), 16, (64, 8))]
    b_op[8 * (_LANE >> 5) + _J, np.broadcast_to(_LANE & 31, (64, 8))] = b[_flat(*b_map(_LANE, _J), 32, (64, 8))]
    d = a_op @ b_op
    held = d[np.broadcast_to(faithful_c(_LANE, _REG)[0], (64, 16)), np.broadcast_to(_LANE & 31, (64, 16))]
    c = np.zeros(1024, dtype=np.int64)
    c[_flat(*c_map(_LANE, _REG), 32, (64, 16))] = held
    return [float(v) for v in c.tolist()]


def exact_products(sa, sb, places) -> dict:
    """{(row, col): fp32 value} of C = A B from the operands' `bf16_scaled` values, every sum exact in
    integers and rounded once; nan where a factor is Inf or NaN."""
    out = {}
    for r, c in places:
        fa, fb = sa[r * 16:(r + 1) * 16], sb[c::32]
        if None in fa or None in fb:
            out[(r, c)] = float("nan")
        else:
            out[(r, c)] = round_to_f32(sum(x * y for x, y in zip(fa, fb)), 2 * SCALE_BITS)
    return out


# --------------------------------------------------------------------------------- every code, once
# One-term tiles as the deep self-test's edge tiles: side 1 has A[r][k] != 0 only at k = r % 16 and B
# dense, so accumulator (r, c) holds the one term A[r][r % 16] * B[r % 16][c]; side 0 is the mirror,
# B[k][c] != 0 only at k = c % 16 and A dense, with the term A[r][c % 16] * B[c % 16][c]. A group is 32
# consecutive codes from a multiple of 32, so of one sign and one exponent field E; it fills one k of
# the dense operand (B's row k, or A's column k) and meets the two powers of two that the other
# operand holds at that k: 2^p1 and -2^p2, chosen so that the product is a normal fp32.

NORMAL_GROUPS = [first for sign in (0, 0x8000) for first in range(sign | 0x0080, sign | 0x7F80, 32)]
ZERO_GROUP = -1           # stands for the group 0x0000, 0x8000, 0x0000, ...
SUBNORMAL_GROUPS = [first for sign in (0, 0x8000) for first in range(sign, sign | 0x0080, 32)]   # holds +-0 too


def group_codes(first: int) -> list[int]:
    if first == ZERO_GROUP:
        return [0x0000 if i % 2 == 0 else 0x8000 for i in range(32)]
    return list(range(first, first + 32))


def group_partners(first: int) -> tuple[float, float]:
    """(2^p1, -2^p2) for a group. Normal codes of exponent field E are in [2^(E-127), 2^(E-126)): p1 puts
    the product into [1, 2), p2 at the lowest binade of normal fp32 where E <= 127 and at the highest
    where E > 127. p in -126..127 is a normal bf16 wherever E is 1..254. A subnormal code is m * 2^-133
    with m < 128: 2^127 and 2^100 take it to m * 2^-6 and m * 2^-33. Zero meets 1 and -2."""
    e = (first >> 7) & 0xFF if first != ZERO_GROUP else -1
    if first == ZERO_GROUP:
        p1, p2 = 0, 1
    elif e == 0:
        p1, p2 = 127, 100
    else:
        p1, p2 = max(127 - e, -126), (1 - e if e <= 127 else 254 - e)
    assert -126 <= p1 <= 127 and -126 <= p2 <= 127
    return float(2.0 ** p1), float(-(2.0 ** p2))


def code_tile(groups, side: int):
    """(a, b) flat float lists of the one-term tile of 16 groups, the codes in B (side 1) or in A (side 0)."""
    assert len(groups) == 16 and side in (0, 1)
    a, b = [0.0] * 512, [0.0] * 512
    for k, first in enumerate(groups):
        codes, (u1, u2) = group_codes(first), group_partners(first)
        for i, code in enumerate(codes):
            if side == 1:
                b[k * 32 + i] = bf16_value(code)
            else:
                a[i * 16 + k] = bf16_value(code)
        if side == 1:
            a[k * 16 + k], a[(k + 16) * 16 + k] = u1, u2
        else:
            b[k * 32 + k], b[k * 32 + k + 16] = u1, u2
    return a, b


def code_tile_term(a, b, r: int, c: int, side: int):
    """The two factors of accumulator (r, c)'s one term."""
    k = r % 16 if side == 1 else c % 16
    return a[r * 16 + k], b[k * 32 + c]


def normal_code_tiles():
    """(side, groups, a, b) of the tiles that hold every normal bf16 code and +-0: 128 a side."""
    groups = NORMAL_GROUPS + [ZERO_GROUP] * 16
    assert len(groups) % 16 == 0
    for side in (1, 0):
        for t in range(0, len(groups), 16):
            yield (side, groups[t:t + 16], *code_tile(groups[t:t + 16], side))


def subnormal_code_tiles():
    """The same for the 2 x 127 subnormal codes: one tile a side (8 groups, each twice)."""
    for side in (1, 0):
        yield (side, SUBNORMAL_GROUPS * 2, *code_tile(SUBNORMAL_GROUPS * 2, side))


def code_tile_expected(a, b, side: int) -> list[int]:
    """The 1,024 fp32 words of the tile: the one product, exact (the caller's conditions make it a
    normal fp32), and +0 where a factor is zero."""
    words = []
    for r in range(32):
        for c in range(32):
            x, y = code_tile_term(a, b, r, c, side)
            p = x * y                      # two 8-bit significands: exact in a double
            words.append(0 if p == 0 else f32_word(p))
    return words


# ------------------------------------------------------------------------------ the host's rounding
# 512 float32 bit patterns that are no bf16 values (low half != 0), finite and normal: ties with an even
# and an odd neighbour, one float32 ulp on either side of a tie, and the carry from the mantissa into
# the exponent, in both signs.

_ROUNDING_FIRST = [0x3FFFFFFF, 0x3FFF8000, 0x3FFF8001, 0x3FFF7FFF, 0xBFFFFFFF, 0xBFFF8000, 0x3F7FFFFF, 0x3F7F8000,
                   0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001, 0xBF808000, 0xBF818000,
                   0x3F800001, 0x3F80FFFF, 0x7F7F7FFF, 0x00808000, 0x00818000, 0x0080FFFF]
_ROUNDING_LOWS = [0x8000, 0x7FFF, 0x8001, 0x0001, 0xFFFF, 0x4000, 0xC000]


def rounding_patterns() -> list[int]:
    out = list(_ROUNDING_FIRST)
    i = 0
    while len(out) < 512:
        high = (0x3E80 + 3 * (i // len(_ROUNDING_LOWS)) % 0x180) | (0x8000 if i % 3 == 1 else 0)
        out.append(high << 16 | _ROUNDING_LOWS[i % len(_ROUNDING_LOWS)])
        i += 1
    return out


def pattern_float(word: int) -> float:
    return struct.unpack("<f", struct.pack("<I", word))[0]


def rounding_tile(side: int):
    """(a, b): the 512 values in A (side 0) against B[k][c] = 1 iff c % 16 == k, so that C[r][c] is
    A[r][c % 16] as gemm_tile rounded it; or in B (side 1) against A[r][k] = 1 iff k == r % 16, so that
    C[r][c] is B[r % 16][c]."""
    values = [pattern_float(w) for w in rounding_patterns()]
    if side == 0:
        return values, [1.0 if c % 16 == k else 0.0 for k in range(16) for c in range(32)]
    return [1.0 if k == r % 16 else 0.0 for r in range(32) for k in range(16)], values


# ------------------------------------------------------------------------------------ mfma_burn sums

def burn_reference(bf16_bits, chains=(0, 1, 2, 3)):
    """s1[lane]: what one iteration of mfma_burn (of these of its four chains) adds to the sum a thread of that lane ends with, exact, as
    a float64 (a multiple of 2^-34 below 1). `bf16_bits` is the probe's binding. Every term is >= 0, so
    s1 is the sum of the terms' magnitudes too."""
    lanes = np.arange(64)
    fa = np.zeros((64, 8))
    fb = np.zeros((64, 8))
    for j in range(8):
        fa[:, j] = [bf16_value(c) for c in bf16_bits((np.float32(0.001) * ((lanes + j) & 7).astype(np.float32)).astype(np.float32))]
        fb[:, j] = [bf16_value(c) for c in bf16_bits((np.float32(0.002) * ((lanes * 3 + j) & 7).astype(np.float32)).astype(np.float32))]

    def as_a(frag):        # the instruction's A'[32][16] from the lanes' first operand
        m = np.zeros((32, 16))
        m[np.broadcast_to(_LANE & 31, (64, 8)), 8 * (_LANE >> 5) + _J] = frag
        return m

    def as_b(frag):
        m = np.zeros((16, 32))
        m[8 * (_LANE >> 5) + _J, np.broadcast_to(_LANE & 31, (64, 8))] = frag
        return m

    # operands are multiples of 2^-17 below 2^-6 (asserted): products of 2^-34 below 2^-12, and the sum of the
    # 4 x 16 x 16 that reach a thread is exact in a double
    for f in (fa, fb):
        assert (f >= 0).all() and (f < 2.0 ** -6).all() and (np.ldexp(f, 17) == np.floor(np.ldexp(f, 17))).all()
    chain = [as_a(fa) @ as_b(fb), as_a(fb) @ as_b(fa), as_a(fa) @ as_b(fa), as_a(fb) @ as_b(fb)]   # c0..c3
    d = sum(chain[i] for i in chains)
    rows = np.broadcast_to(faithful_c(_LANE, _REG)[0], (64, 16))
    return d[rows, np.broadcast_to(_LANE & 31, (64, 16))].sum(axis=1)


def burn_bound(iters: int, s1: float) -> float:
    """The standard forward bound of the sum of N + 1 terms added one at a time in fp32, N * 2^-24 * S:
    N = 16 iters additions inside the MFMAs on the way of one product, and the 64 of the final reduction;
    S = iters * s1 is the sum of the magnitudes of all terms."""
    return (16 * iters + 64) * 2.0 ** -24 * iters * s1
