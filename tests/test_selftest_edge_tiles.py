"""The edge tiles of the deep self-test's matrix paths (nanogpu.probe.selftest_paths.edge_tiles): the
conditions that make them exact and complete, checked on the host. tests/test_gpu_selftest_edges.py
runs the same tiles through `matrix_tile` on the device."""
import functools
import math
import struct

import pytest

from nanogpu.probe import selftest_paths as SP

NARROW = ("fp8", "bf8", "i8", "mxfp8", "mxfp6", "mxfp4")
WIDE = ("f16", "f32", "f64")
WIDE_STRUCT = {"f16": ("<H", "<e"), "f32": ("<I", "<f"), "f64": ("<Q", "<d")}
NARROW_DECODE = {"fp8": SP.decode_e4m3fn, "mxfp8": SP.decode_e4m3fn, "bf8": SP.decode_e5m2, "mxfp6": SP.decode_e2m3,
                 "mxfp4": SP.decode_e2m1}


def decode(path, code):
    """The value of one operand code by the format's own decoder (not path_decode, which
    exact_product uses)."""
    if path == "i8":
        return code - 256 if code & 0x80 else code
    if path in WIDE:
        u, f = WIDE_STRUCT[path]
        return struct.unpack(f, struct.pack(u, code))[0]
    return NARROW_DECODE[path](code)


@functools.lru_cache(maxsize=None)
def tiles(path):
    return list(SP.edge_tiles(path))


_TERMS = {}


def terms(path, a, b):
    """[(row, col, k)] of the non-zero terms of a tile (of `tiles`, which keeps them alive)."""
    key = (path, id(a), id(b))
    if key not in _TERMS:
        _TERMS[key] = _terms(path, a, b)
    return _TERMS[key]


def _terms(path, a, b):
    dim, K = SP.path_dim(path), SP.PATH_K[path]
    nz_a = [[k for k in range(K) if decode(path, a[r][k]) != 0] for r in range(dim)]
    nz_b = [{k for k in range(K) if decode(path, b[k][c]) != 0} for c in range(dim)]
    return [(r, c, k) for r in range(dim) for c in range(dim) for k in nz_a[r] if k in nz_b[c]]


def codes_side(path, a, b):
    """0 when A holds the codes under test and B the units, 1 the other way round."""
    dim, K = SP.path_dim(path), SP.PATH_K[path]
    a_sparse = all(sum(1 for k in range(K) if a[r][k]) == 1 for r in range(dim))
    return 1 if a_sparse else 0


@pytest.mark.parametrize("path", SP.PATHS)
def test_every_accumulator_has_at_most_one_term_and_every_operand_is_finite(path):
    dim = SP.path_dim(path)
    assert tiles(path)
    for a, b, _sa, _sb, _opsel in tiles(path):
        t = terms(path, a, b)
        assert len({(r, c) for r, c, _k in t}) == len(t)            # no accumulator twice
        assert len(t) > dim * dim // 2                              # and the tile is not empty
        assert all(SP.code_is_finite(path, c) for row in a for c in row)
        assert all(SP.code_is_finite(path, c) for row in b for c in row)


@pytest.mark.parametrize("path", SP.PATHS)
def test_every_code_meets_a_unit_on_both_sides(path):
    """Every finite code of the narrow formats, and the edge codes of f16 / f32 / f64, is a
    factor of some accumulator's one term in A against a unit in B, and in B against a unit in A."""
    units = set(SP.unit_codes(path))
    assert {decode(path, u) for u in units} == ({1, -1, -128} if path == "i8" else {1.0, -1.0})
    seen = [set(), set()]
    units_used = set()
    for a, b, _sa, _sb, _opsel in tiles(path):
        side = codes_side(path, a, b)
        for r, c, k in terms(path, a, b):
            code, unit = (a[r][k], b[k][c]) if side == 0 else (b[k][c], a[r][k])
            assert unit in units
            seen[side].add(code)
            units_used.add(unit)
    if path in NARROW:
        want = {c for c in range(1 << SP.PATH_CODE_BITS[path]) if SP.code_is_finite(path, c) and decode(path, c) != 0}
        assert len(want) == {"fp8": 252, "mxfp8": 252, "bf8": 246, "i8": 255, "mxfp6": 62, "mxfp4": 14}[path]
    else:
        ebits, mbits, bias = SP.PATH_FORMAT[path]
        ones, sign = (1 << mbits) - 1, 1 << (SP.PATH_CODE_BITS[path] - 1)
        edge = [1, ones, 1 << mbits, ((1 << ebits) - 2) << mbits | ones, bias << mbits]
        want = {c | s for c in edge for s in (0, sign)}
        assert [decode(path, c) for c in edge[:4]] == {
            "f16": [2.0 ** -24, 2.0 ** -14 - 2.0 ** -24, 2.0 ** -14, 65504.0],
            "f32": [2.0 ** -149, 2.0 ** -126 - 2.0 ** -149, 2.0 ** -126, (2.0 - 2.0 ** -23) * 2.0 ** 127],
            "f64": [5e-324, 2.0 ** -1022 - 5e-324, 2.0 ** -1022, 1.7976931348623157e308]}[path]
    assert want <= seen[0] and want <= seen[1], (sorted(want - seen[0]), sorted(want - seen[1]))
    assert units_used == units
    # zero and minus zero are operands of the tiles too (their terms vanish, so `terms` skips them)
    for side in range(2):
        held = {c for a, b, *_ in tiles(path) if codes_side(path, a, b) == side
                for row in (a if side == 0 else b) for c in row}
        assert {0, 0x80 if path == "i8" else 1 << (SP.PATH_CODE_BITS[path] - 1)} <= held


@pytest.mark.parametrize("path", SP.SCALED_PATHS)
def test_every_scale_multiplies_a_term_in_every_byte_on_both_sides(path):
    """Every E8M0 value 0..254 scales a non-zero term as A's scale and as B's, carried in each of
    the four bytes of the scale register; within a tile scale_a + scale_b - 254 stays in
    [-2, 2] for every (row, col, block), terms or not."""
    dim = SP.path_dim(path)
    seen = [set(), set()]          # (scale, byte) of A and of B
    for a, b, sa, sb, opsel in tiles(path):
        lo, hi = SP.EDGE_SCALE_SUM
        assert all(lo <= sa[r][blk] + sb[blk][c] - 254 <= hi for r in range(dim) for c in range(dim) for blk in range(2))
        assert all(0 <= v <= 254 for row in sa + sb for v in row)
        for r, c, k in terms(path, a, b):
            seen[0].add((sa[r][k // 32], opsel[0]))
            seen[1].add((sb[k // 32][c], opsel[1]))
    every = {(s, byte) for s in range(255) for byte in range(4)}
    assert seen[0] == every and seen[1] == every, (sorted(every - seen[0])[:8], sorted(every - seen[1])[:8])
    assert len(tiles(path)) == SP.EDGE_SCALE_TILES


def _smallest_normal(path):
    return 2.0 ** -1022 if path == "f64" else 1 if path == "i8" else 2.0 ** -126


@pytest.mark.parametrize("path", SP.PATHS)
def test_exact_product_is_decode_times_scale_in_every_slot(path):
    """`exact_product` (integers, path_decode) against the formats' decoders in floating point:
    every accumulator is its one term's decode(a) x 2^(sa - 127) x decode(b) x 2^(sb - 127), or
    +0. The result is exactly representable in the accumulator, and normal there. The one
    exception to "normal" is forced: a subnormal of f32 or f64 times +-1 is that subnormal, since
    the operand's format is the accumulator's."""
    dim = SP.path_dim(path)
    subnormal_in = 0
    for a, b, sa, sb, _opsel in tiles(path):
        units, abs_units, unit_exp = SP.exact_product(path, a, b, sa, sb)
        values = SP.tile_values(path, [u for row in units for u in row], unit_exp)
        want = [0] * (dim * dim) if path == "i8" else [0.0] * (dim * dim)
        for r, c, k in terms(path, a, b):
            v = decode(path, a[r][k]) * decode(path, b[k][c])
            if sa is not None:                      # every factor and partial product is exact in a double
                v = v * SP.decode_e8m0(sa[r][k // 32]) * SP.decode_e8m0(sb[k // 32][c])
            want[r * dim + c] = v
            assert abs(units[r][c]) == abs_units[r][c] != 0
            if abs(v) < _smallest_normal(path):
                assert path in ("f32", "f64") and abs(decode(path, a[r][k])) * abs(decode(path, b[k][c])) == abs(v)
                assert min(abs(decode(path, a[r][k])), abs(decode(path, b[k][c]))) < _smallest_normal(path)
                subnormal_in += 1
            assert not math.isinf(v)
        assert values == want
        assert all(math.copysign(1.0, v) > 0 for v in values if v == 0)        # no -0 in an expected tile
        # representable: the words decode back to the same values
        words = SP.tile_words(path, values)
        if a is tiles(path)[0][0]:
            assert SP.product_words(path, a, b, sa, sb) == words
        if path == "i8":
            assert [w - (1 << 32) if w >> 31 else w for w in words] == want
        elif path == "f64":
            assert [struct.unpack("<d", struct.pack("<II", words[2 * i], words[2 * i + 1]))[0] for i in range(dim * dim)] == want
        else:
            assert [struct.unpack("<f", struct.pack("<I", w))[0] for w in words] == want
    assert (subnormal_in > 0) == (path in ("f32", "f64"))


def test_edge_tile_counts():
    """What the GPU test puts on the device: tiles per path (recorded in profiles/gpu_calibration.md)."""
    assert {p: len(tiles(p)) for p in SP.PATHS} == {"f16": 12, "fp8": 4, "bf8": 4, "i8": 4, "mxfp8": 256, "mxfp6": 256,
                                                   "mxfp4": 256, "f32": 12, "f64": 12}


def test_a_naive_scale_choice_is_rejected_by_the_window():
    """scale_b = 254 - scale_a per block, but independent of the row's parity, leaves the window at
    the ends only by +-1; scale_b[c] = 254 - scale_a[c] taken per index does not: row 0 against
    column 31 of such a tile has scale sum -31. The builder's sums are in [-1, 1]."""
    for t in (0, 1, 130, 255):
        sa, sb, _ = SP.edge_scales("mxfp8", t)
        sums = {sa[r][blk] + sb[blk][c] - 254 for r in range(32) for c in range(32) for blk in range(2)}
        assert sums == {-1, 0, 1}
