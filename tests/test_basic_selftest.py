"""The basic self-test's one tile (nanogpu.agent.node.gpu_selftest) can fail: a model of the probe's
`mfma_tile` kernel with wrong lane maps, changed operands, flipped operand bits and changed outputs
stands in for the device, and every one of them must make `gpu_selftest` return False. Also here, on
the host: the conditions `basic_tile_operands` states, the host's float32 -> bf16 rounding against
torch's, and the conditions of the tiles tests/test_gpu_basic_selftest.py puts on the device."""
import itertools
import math
from fractions import Fraction

import numpy as np
import pytest

import bf16_tile_cases as K            # tests/ is on sys.path (no package)
from nanogpu.agent.node import basic_tile_operands, gpu_selftest


class ModelProbe:
    """A probe whose gemm_tile is the kernel model with the given maps."""

    def __init__(self, a_map=K.faithful_a, b_map=K.faithful_b, c_map=K.faithful_c):
        self.maps = (a_map, b_map, c_map)
        self.tiles = 0

    def copy_check(self, dev, n_floats):
        return True

    def gemm_tile(self, a, b):
        self.tiles += 1
        return K.model_tile(a, b, *self.maps)


def swap(n, i, j):
    p = np.arange(n)
    p[i], p[j] = j, i
    return p


def a_rows(p):
    return lambda l, j: (p[l & 31], 8 * (l >> 5) + j)


def a_ks(p):
    return lambda l, j: (l & 31, p[8 * (l >> 5) + j])


def b_cols(p):
    return lambda l, j: (8 * (l >> 5) + j, p[l & 31])


def b_ks(p):
    return lambda l, j: (p[8 * (l >> 5) + j], l & 31)


def c_rows(p):
    return lambda l, reg: (p[K.faithful_c(l, reg)[0]], l & 31)


def c_cols(p):
    return lambda l, reg: (K.faithful_c(l, reg)[0], p[l & 31])


def column_major(rows, cols):
    """The element a kernel reads at (i, j) of a [rows][cols] row-major operand when it indexes it as
    [cols][rows]: flat index j * rows + i, given as (row, col) of the true layout."""
    return lambda i, j: divmod(j * rows + i, cols)


def mutants():
    """(name, kwargs of ModelProbe) of every wrong kernel of the family."""
    for i, j in itertools.combinations(range(32), 2):
        yield f"A rows {i}<->{j}", {"a_map": a_rows(swap(32, i, j))}
        yield f"B columns {i}<->{j}", {"b_map": b_cols(swap(32, i, j))}
        yield f"C rows {i}<->{j}", {"c_map": c_rows(swap(32, i, j))}
        yield f"C columns {i}<->{j}", {"c_map": c_cols(swap(32, i, j))}
    for i, j in itertools.combinations(range(16), 2):
        yield f"A k {i}<->{j}", {"a_map": a_ks(swap(16, i, j))}
        yield f"B k {i}<->{j}", {"b_map": b_ks(swap(16, i, j))}
    half = np.arange(16) ^ 8
    yield "A half-waves swapped", {"a_map": a_ks(half)}
    yield "B half-waves swapped", {"b_map": b_ks(half)}
    yield "C half-waves swapped", {"c_map": lambda l, reg: K.faithful_c(l ^ 32, reg)}
    yield "A j reversed", {"a_map": lambda l, j: (l & 31, 8 * (l >> 5) + 7 - j)}
    yield "A column-major", {"a_map": lambda l, j: column_major(32, 16)(l & 31, 8 * (l >> 5) + j)}
    yield "B column-major", {"b_map": lambda l, j: column_major(16, 32)(8 * (l >> 5) + j, l & 31)}
    for name, row in WRONG_ROWS.items():
        c_map = (lambda row: lambda l, reg: (row(reg, l >> 5), l & 31))(row)
        if K.c_map_is_bijection(c_map):
            yield f"C row = {name}", {"c_map": c_map}


WRONG_ROWS = {
    "reg + 16h": lambda reg, h: reg + 16 * h,
    "(reg&3) + 4(reg>>2) + 16h": lambda reg, h: (reg & 3) + 4 * (reg >> 2) + 16 * h,
    "(reg&7) + 8(reg>>3) + 16h": lambda reg, h: (reg & 7) + 8 * (reg >> 3) + 16 * h,
    "(reg&7) + 8(reg>>3) + 4h": lambda reg, h: (reg & 7) + 8 * (reg >> 3) + 4 * h,       # no bijection: skipped
    "4(reg&3) + (reg>>2) + 16h": lambda reg, h: 4 * (reg & 3) + (reg >> 2) + 16 * h,
    "(reg&3) + 4h + 8(reg>>2) with reg>>2 reversed": lambda reg, h: (reg & 3) + 8 * (3 - (reg >> 2)) + 4 * h,
}


def test_the_faithful_kernel_passes_and_runs_one_tile():
    probe = ModelProbe()
    assert gpu_selftest(probe, 0) is True
    assert probe.tiles == 1
    a, b = basic_tile_operands()
    want = (np.array(a).reshape(32, 16) @ np.array(b).reshape(16, 32)).ravel().tolist()
    assert K.model_tile(a, b) == want                      # the model with the faithful maps is the product


def test_every_routing_mutant_fails():
    names = []
    passed = []
    for name, maps in mutants():
        names.append(name)
        if gpu_selftest(ModelProbe(**maps), 0):
            passed.append(name)
    counts = {prefix: sum(n.startswith(prefix) for n in names) for prefix in
              ("A rows", "B columns", "A k", "B k", "C rows", "C columns", "C row =")}
    assert counts == {"A rows": 496, "B columns": 496, "A k": 120, "B k": 120, "C rows": 496, "C columns": 496, "C row =": 5}
    assert len(names) == 2 * 496 + 2 * 120 + 2 * 496 + 3 + 1 + 2 + 5
    assert not passed, passed[:20]


class TamperProbe:
    """gemm_tile is the faithful model after `change(a, b)`, a pair of flat integer lists to multiply."""

    def __init__(self, change):
        self.change = change

    def copy_check(self, dev, n_floats):
        return True

    def gemm_tile(self, a, b):
        return K.model_tile(*self.change(list(a), list(b)))


def test_every_operand_element_changed_by_one_fails():
    passed = []
    for side, i, d in itertools.product((0, 1), range(512), (-1.0, 1.0)):
        def change(a, b):
            (a, b)[side][i] += d
            return a, b
        if gpu_selftest(TamperProbe(change), 0):
            passed.append((side, i, d))
    assert not passed, passed[:20]


class FlipProbe:
    """gemm_tile as a device would compute it had one bit of one operand's bf16 code flipped on the way:
    the flipped code decoded, every sum exact and rounded once to fp32, Inf or NaN in the row or column
    where the flip makes one. Only the row (a flip in A) or column (in B) that the element reaches is
    computed again; the rest is the faithful model's."""

    def __init__(self):
        self.flip = None          # (side, element, bit)
        self.base = None

    def copy_check(self, dev, n_floats):
        return True

    def gemm_tile(self, a, b):
        if self.base is None or self.base[0] != (a, b):
            self.base = ((list(a), list(b)), [[K.bf16_code(v) for v in a], [K.bf16_code(v) for v in b]],
                         [[K.bf16_scaled(K.bf16_code(v)) for v in a], [K.bf16_scaled(K.bf16_code(v)) for v in b]],
                         K.model_tile(a, b))
        _, codes, scaled, c = self.base
        side, i, bit = self.flip
        scaled = [list(scaled[0]), list(scaled[1])]
        scaled[side][i] = K.bf16_scaled(codes[side][i] ^ (1 << bit))
        assert scaled[side][i] != self.base[2][side][i]
        places = [(i // 16, col) for col in range(32)] if side == 0 else [(row, i % 32) for row in range(32)]
        c = list(c)
        for (row, col), v in K.exact_products(scaled[0], scaled[1], places).items():
            c[row * 32 + col] = v
        return c


def test_every_flipped_bit_of_every_operand_code_fails():
    probe = FlipProbe()
    passed = []
    for flip in itertools.product((0, 1), range(512), range(16)):
        probe.flip = flip
        if gpu_selftest(probe, 0):
            passed.append(flip)
    assert not passed, passed[:20]


def test_every_output_changed_by_one_ulp_fails():
    a, b = basic_tile_operands()
    c = K.model_tile(a, b)

    class Probe:
        def __init__(self, i, toward):
            self.i, self.toward = i, toward

        def copy_check(self, dev, n_floats):
            return True

        def gemm_tile(self, a_, b_):
            out = list(c)
            out[self.i] = float(np.nextafter(np.float32(out[self.i]), np.float32(self.toward)))
            assert out[self.i] != c[self.i]
            return out

    passed = [(i, t) for i in range(1024) for t in (-math.inf, math.inf) if gpu_selftest(Probe(i, t), 0)]
    assert not passed, passed[:20]


# ------------------------------------------------------------------------- the operands' conditions

def rank(rows) -> int:
    """Rank over the rationals, by elimination in exact arithmetic."""
    m = [[Fraction(v) for v in row] for row in rows]
    r = 0
    for col in range(len(m[0])):
        pivot = next((i for i in range(r, len(m)) if m[i][col] != 0), None)
        if pivot is None:
            continue
        m[r], m[pivot] = m[pivot], m[r]
        for i in range(r + 1, len(m)):
            if m[i][col] != 0:
                f = m[i][col] / m[r][col]
                m[i] = [x - f * y for x, y in zip(m[i], m[r])]
        r += 1
    return r


@pytest.fixture(scope="module")
def tile():
    a, b = basic_tile_operands()
    assert len(a) == len(b) == 512
    A = [[int(a[r * 16 + k]) for k in range(16)] for r in range(32)]
    B = [[int(b[k * 32 + c]) for c in range(32)] for k in range(16)]
    C = [[sum(A[r][k] * B[k][c] for k in range(16)) for c in range(32)] for r in range(32)]
    return a, b, A, B, C


def test_operands_are_a_fixed_function_of_the_index():
    assert basic_tile_operands() == basic_tile_operands()
    assert all(type(v) is float for side in basic_tile_operands() for v in side)


def test_operands_are_exact(tile):
    a, b, A, B, _C = tile
    for v in a + b:
        assert v == int(v) and abs(v) <= 256
        assert K.bf16_value(K.bf16_code(v)) == v                       # a bf16 value
    bound = max(sum(abs(A[r][k]) * abs(B[k][c]) for k in range(16)) for r in range(32) for c in range(32))
    assert bound < 2 ** 24
    assert bound < 2 ** 17            # what the docstring adds: a change of 2^-7 stays visible


def test_every_element_matters(tile):
    _a, _b, A, B, _C = tile
    for k in range(16):
        assert any(B[k][c] for c in range(32)) and any(A[r][k] for r in range(32))
    assert all(v != 0 for row in A + B for v in row)                    # so a flipped sign bit is a change too


def test_operands_route(tile):
    _a, _b, A, B, C = tile
    At = [list(col) for col in zip(*A)]
    Bt = [list(col) for col in zip(*B)]
    assert len({tuple(row) for row in A}) == 32 and len({tuple(col) for col in Bt}) == 32
    assert len({tuple(col) for col in At}) == 16 and len({tuple(row) for row in B}) == 16     # the k-slices differ
    assert rank(A) == 16 and rank(B) == 16
    for k1, k2 in itertools.combinations(range(16), 2):                 # a k-permutation of one operand alone
        p = swap(16, k1, k2)
        assert [[sum(A[r][p[k]] * B[k][c] for k in range(16)) for c in range(32)] for r in range(32)] != C
    flat_a = [v for row in A for v in row]
    flat_b = [v for row in B for v in row]
    A_cm = [[flat_a[k * 32 + r] for k in range(16)] for r in range(32)]   # A and B as read column-major
    B_cm = [[flat_b[c * 16 + k] for c in range(32)] for k in range(16)]
    assert [[sum(A_cm[r][k] * B[k][c] for k in range(16)) for c in range(32)] for r in range(32)] != C
    assert [[sum(A[r][k] * B_cm[k][c] for k in range(16)) for c in range(32)] for r in range(32)] != C


def test_operands_cover_every_bit_of_the_code(tile):
    a, b, _A, _B, _C = tile
    for side in (a, b):
        codes = [K.bf16_code(v) for v in side]
        ones = zeros = 0
        for c in codes:
            ones |= c
            zeros |= ~c & 0xFFFF
        assert ones == 0xFFFF and zeros == 0xFFFF
        assert 0x3F80 in codes and 0x4000 in codes                      # 1.0 and 2.0: all eight exponent bits toggle
        assert any(abs(v) >= 129 and int(v) % 2 == 1 for v in side)     # mantissa bit 0
        assert any(v < 0 for v in side) and any(v > 0 for v in side)


def test_product_is_not_constant_and_repeats_no_row_or_column(tile):
    _a, _b, _A, _B, C = tile
    assert len({v for row in C for v in row}) > 1
    assert len({tuple(row) for row in C}) == 32
    assert len({tuple(col) for col in zip(*C)}) == 32


# ------------------------------------------------------------------------------ the host's rounding

@pytest.fixture(scope="module")
def P():
    from nanogpu.native import probe

    return probe(required=True)      # the extension loads without a GPU; bf16_bits touches none


def both_roundings(P, words):
    """(the binding's codes, torch's codes, which inputs are NaN) of float32 bit patterns (an int64
    tensor), as tensors. No value passes through a Python float: the words become a float32 tensor by
    a view, and the binding reads that memory."""
    import torch

    x = words.to(torch.int32).view(torch.float32) if words.dtype != torch.int32 else words.view(torch.float32)
    ours = torch.tensor(P.bf16_bits(x.numpy()), dtype=torch.int32)
    theirs = x.bfloat16().view(torch.int16).to(torch.int32) & 0xFFFF
    return ours, theirs, torch.isnan(x)


def assert_same_rounding(P, words):
    import torch

    ours, theirs, nan = both_roundings(P, words)
    is_nan_code = lambda c: ((c & 0x7F80) == 0x7F80) & ((c & 0x007F) != 0)   # noqa: E731
    assert bool((is_nan_code(ours) == nan).all()) and bool((is_nan_code(theirs) == nan).all())
    wrong = torch.nonzero(~nan & (ours != theirs)).ravel()
    assert wrong.numel() == 0, [(hex(int(words[i]) & 0xFFFFFFFF), hex(int(ours[i])), hex(int(theirs[i]))) for i in wrong[:8]]
    # a NaN keeps its sign
    u = words.to(torch.int64) & 0xFFFFFFFF
    assert bool(((ours >> 15) == (u >> 31).to(torch.int32))[nan].all())
    return int(nan.sum())


def test_bf16_bits_equals_torch_on_every_high_half_and_the_deciding_low_halves(P):
    import torch

    lows = torch.tensor([0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF], dtype=torch.int64)
    words = ((torch.arange(0x10000, dtype=torch.int64)[:, None] << 16) | lows[None, :]).ravel()
    assert words.numel() == 393216
    words = torch.where(words >= 1 << 31, words - (1 << 32), words).to(torch.int32)
    nans = assert_same_rounding(P, words)
    assert nans == 2 * (127 * 6 + 5)
    pinned = {0x7F800001: None, 0xFF800001: None, 0x7F7FFFFF: 0x7F80, 0x7F7F8000: 0x7F80, 0x7F7F7FFF: 0x7F7F,
              0x7F800000: 0x7F80, 0xFF800000: 0xFF80, 0x00000000: 0x0000, 0x80000000: 0x8000, 0x3F808000: 0x3F80,
              0x3F818000: 0x3F82, 0x3FFFFFFF: 0x4000, 0x00008000: 0x0000, 0x00008001: 0x0001, 0x007FFFFF: 0x0080}
    got = P.bf16_bits(np.array(list(pinned), dtype=np.uint32).view(np.float32))
    for (word, want), code in zip(pinned.items(), got):
        if want is None:              # a NaN whose payload lies in the low half alone stays a NaN, with its sign
            assert code & 0x7F80 == 0x7F80 and code & 0x7F and code >> 15 == word >> 31, (hex(word), hex(code))
        else:
            assert code == want, (hex(word), hex(code))


def test_bf16_bits_equals_torch_on_random_patterns(P):
    import torch

    g = torch.Generator().manual_seed(0xB16)
    words = torch.randint(-(1 << 31), 1 << 31, (1 << 20,), generator=g, dtype=torch.int64).to(torch.int32)
    assert assert_same_rounding(P, words) > 0


def test_bf16_bits_takes_a_list_and_rejects_other_buffers(P):
    assert P.bf16_bits([1.0, -2.0, 255.0, 0.0, -0.0, 1.00390625]) == [0x3F80, 0xC000, 0x437F, 0x0000, 0x8000, 0x3F80]
    assert P.bf16_bits([]) == []
    # 1 + 2^-8 + 2^-30 is no float32: it rounds to the tie 1 + 2^-8 first and then to even, 1.0, where one
    # rounding of the double would give 0x3f81 (the note in docs/REFERENCE.md)
    assert P.bf16_bits([1.0 + 2.0 ** -8 + 2.0 ** -30]) == [0x3F80]
    for bad in (np.zeros(4, dtype=np.float64), np.zeros((2, 2), dtype=np.float32), np.zeros(8, dtype=np.float32)[::2], b"abcd"):
        with pytest.raises(ValueError):
            P.bf16_bits(bad)


# ------------------------------------------------------- the tiles of test_gpu_basic_selftest.py

def test_code_tiles_have_one_term_an_exact_normal_product_and_every_code_on_both_sides():
    seen = {0: set(), 1: set()}
    tiles = list(K.normal_code_tiles())
    assert len(tiles) == 256
    for side, _groups, a, b in tiles:
        codes_a, codes_b = [K.bf16_code(v) for v in a], [K.bf16_code(v) for v in b]
        assert all((c >> 7) & 0xFF != 0xFF for c in codes_a + codes_b)                 # no Inf, no NaN
        assert all((c >> 7) & 0xFF != 0 or c & 0x7F == 0 for c in codes_a + codes_b)   # no subnormal
        words = K.code_tile_expected(a, b, side)
        for r in range(32):
            nz_a = [k for k in range(16) if a[r * 16 + k] != 0]
            for c in range(32):
                ks = [k for k in nz_a if b[k * 32 + c] != 0]
                x, y = K.code_tile_term(a, b, r, c, side)
                word = words[r * 32 + c]
                if x == 0 or y == 0:                                   # the term is +-0: no other term either
                    assert ks == [] and word == 0
                    continue
                assert ks == [r % 16 if side == 1 else c % 16]         # one term
                exact = Fraction(x) * Fraction(y)
                assert Fraction(K.pattern_float(word)) == exact        # the expected word is the product, unrounded
                assert 0 < (word >> 23) & 0xFF < 255                   # and a normal fp32
        under_test, partner = (codes_a, codes_b) if side == 0 else (codes_b, codes_a)
        seen[side].update(under_test)
        assert all(c & 0x7F == 0 for c in partner)                     # the partners are powers of two, or zero
    normal = {c for c in range(1 << 16) if 0 < (c >> 7) & 0xFF < 255}
    assert len(normal) == 65024
    for side in (0, 1):
        assert normal | {0x0000, 0x8000} == seen[side]


def test_subnormal_code_tiles_have_one_term_and_a_normal_product():
    tiles = list(K.subnormal_code_tiles())
    assert [side for side, *_ in tiles] == [1, 0]
    subnormal = {c for c in range(1 << 16) if (c >> 7) & 0xFF == 0 and c & 0x7F}
    assert len(subnormal) == 254
    for side, _groups, a, b in tiles:
        held = {K.bf16_code(v) for v in (a if side == 0 else b)}
        assert subnormal <= held <= subnormal | {0x0000, 0x8000}
        for word in K.code_tile_expected(a, b, side):
            assert word == 0 or 0 < (word >> 23) & 0xFF < 255
        for r in range(32):
            for c in range(32):
                assert sum(1 for k in range(16) if a[r * 16 + k] != 0 and b[k * 32 + c] != 0) <= 1


def test_rounding_tile_values_are_no_bf16_values_and_cover_the_cases():
    words = K.rounding_patterns()
    assert len(words) == 512
    assert all(w & 0xFFFF and 0 < (w >> 23) & 0xFF < 255 for w in words)
    low, odd = (lambda w: w & 0xFFFF), (lambda w: (w >> 16) & 1)
    for parity in (0, 1):
        for half in (0x8000, 0x7FFF, 0x8001):                          # a tie, and one ulp on either side of it
            assert any(low(w) == half and odd(w) == parity for w in words)
    assert any(w & 0x007FFFFF >= 0x007F8000 for w in words)            # the carry into the exponent
    assert 0x3FFFFFFF in words
    assert any(w >> 31 for w in words) and any(not w >> 31 for w in words)
    for side in (0, 1):
        a, b = K.rounding_tile(side)
        assert len(a) == len(b) == 512 and all(K.pattern_float(K.f32_word(v)) == v for v in a + b)


def test_burn_reference_tells_adjacent_iteration_counts_apart(P):
    s1 = K.burn_reference(P.bf16_bits)
    assert s1.shape == (64,) and (s1 > 0).all()
    for lane in range(64):
        for iters in (1, 8, 9, 64):       # s_ref(iters + 1) - s_ref(iters) = s1 exceeds the two bounds together
            assert s1[lane] > K.burn_bound(iters, s1[lane]) + K.burn_bound(iters + 1, s1[lane])
    parts = [K.burn_reference(P.bf16_bits, chains=(chain,)) for chain in range(4)]
    assert np.array_equal(sum(parts), s1)
    for part in parts:                    # a dropped chain is iters * part away: more than the bound
        for iters in (1, 8, 9, 64):
            assert all(iters * part[lane] > K.burn_bound(iters, s1[lane]) for lane in range(64))
