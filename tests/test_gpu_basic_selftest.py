"""`gemm_tile`, the one bf16 MFMA tile of the basic self-test, bit-exact on a real MI355X (`pytest -m gpu`):
the self-test's own operands, the self-test failing through the real kernel on misrouted operands, random
integer tiles, every normal bf16 code once in A and once in B, and the host's rounding on the way in. Every
comparison is == on fp32 bit patterns against integer arithmetic on the host; there is no tolerance in this
file but the derived bound of the burn's sums. tests/test_basic_selftest.py checks the tiles' own conditions."""
import collections
import time

import numpy as np
import pytest

import bf16_tile_cases as K            # tests/ is on sys.path (no package)

pytestmark = pytest.mark.gpu


def record(key: str, value) -> None:
    """Measured facts for profiles/gpu_calibration.md, into the same file as test_gpu.py's."""
    from test_gpu import record as record_fact

    record_fact(key, value)


@pytest.fixture(scope="module")
def P():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    from nanogpu.native import probe

    return probe(required=True)


@pytest.fixture(scope="module", autouse=True)
def wall_time():
    t0 = time.perf_counter()
    yield
    record("basic_selftest_gpu_file_wall_seconds", round(time.perf_counter() - t0, 2))


def words(values) -> np.ndarray:
    """The fp32 bit patterns of what gemm_tile returned."""
    return np.array(values, dtype=np.float32).view(np.uint32)


def test_production_operands_give_the_integer_product(P):
    from nanogpu.agent.node import basic_tile_operands, gpu_selftest

    a, b = basic_tile_operands()
    want = np.array(a, dtype=np.int64).reshape(32, 16) @ np.array(b, dtype=np.int64).reshape(16, 32)
    got = words(P.gemm_tile(a, b))
    assert (got == want.astype(np.float32).view(np.uint32).ravel()).all()
    assert gpu_selftest(P, 0) is True


class Proxy:
    """The real probe behind a change of the operands on their way to the real gemm_tile."""

    def __init__(self, P, change):
        self.P, self.change = P, change

    def copy_check(self, dev, n_floats):
        return self.P.copy_check(dev, n_floats)

    def gemm_tile(self, a, b):
        return self.P.gemm_tile(*self.change(list(a), list(b)))


def test_the_self_test_fails_through_the_real_kernel_on_misrouted_operands(P):
    from nanogpu.agent.node import gpu_selftest

    def a_read_transposed(a, b):           # what a kernel indexing A as [16][32] would load
        return [a[(k * 32 + r) // 16 * 16 + (k * 32 + r) % 16] for r in range(32) for k in range(16)], b

    def b_columns_swapped(a, b):
        for k in range(16):
            b[k * 32 + 3], b[k * 32 + 20] = b[k * 32 + 20], b[k * 32 + 3]
        return a, b

    assert gpu_selftest(Proxy(P, lambda a, b: (a, b)), 0) is True
    assert gpu_selftest(Proxy(P, a_read_transposed), 0) is False
    assert gpu_selftest(Proxy(P, b_columns_swapped), 0) is False


def test_random_integer_tiles_are_exact(P):
    """|element| <= 255, so 16 * 255^2 = 1,040,400 < 2^24: exact in any order. The second set scales row r
    of A by 2^e_r and column c of B by 2^f_c, e and f in [-30, 30]: every element is still a bf16 value, and
    every product and sum is the integer one times 2^(e_r + f_c), a normal fp32."""
    rng = np.random.RandomState(20260)
    wrong = 0
    for scaled in (False, True):
        for _ in range(64):
            a = rng.randint(-255, 256, size=(32, 16)).astype(np.int64)
            b = rng.randint(-255, 256, size=(16, 32)).astype(np.int64)
            e = rng.randint(-30, 31, size=32) if scaled else np.zeros(32, dtype=np.int64)
            f = rng.randint(-30, 31, size=32) if scaled else np.zeros(32, dtype=np.int64)
            fa = np.ldexp(a.astype(np.float64), e[:, None])
            fb = np.ldexp(b.astype(np.float64), f[None, :])
            want = np.ldexp((a @ b).astype(np.float64), e[:, None] + f[None, :]).astype(np.float32)
            assert (want.astype(np.float64) == np.ldexp((a @ b).astype(np.float64), e[:, None] + f[None, :])).all()
            got = words(P.gemm_tile(fa.ravel().tolist(), fb.ravel().tolist()))
            wrong += int((got != want.view(np.uint32).ravel()).sum())
    assert wrong == 0


def run_code_tiles(P, tiles):
    """[(side, code under test, its partner, expected word, got word)] of every accumulator of the tiles."""
    out = []
    for side, _groups, a, b in tiles:
        want = K.code_tile_expected(a, b, side)
        got = words(P.gemm_tile(a, b)).tolist()
        assert len(got) == 1024
        for r in range(32):
            for c in range(32):
                x, y = K.code_tile_term(a, b, r, c, side)
                code, partner = (x, y) if side == 0 else (y, x)
                out.append((side, K.bf16_code(code), partner, want[r * 32 + c], got[r * 32 + c]))
    return out


def test_every_normal_bf16_code_is_exact_once_as_a_and_once_as_b(P):
    """Each accumulator's one term is a code times a power of two, an exact normal fp32; +0 where the
    code is +-0. 128 tiles a side."""
    t0 = time.perf_counter()
    results = run_code_tiles(P, K.normal_code_tiles())
    wall = time.perf_counter() - t0
    wrong = [(side, hex(code), partner, hex(want), hex(got)) for side, code, partner, want, got in results if want != got]
    seen = [{code for side, code, *_ in results if side == s} for s in (0, 1)]
    facts = {"tiles": len(results) // 1024, "accumulators": len(results), "codes_in_a": len(seen[0]),
             "codes_in_b": len(seen[1]), "wrong_words": len(wrong), "wall_seconds": round(wall, 3)}
    print(facts, wrong[:12])
    record("basic_selftest_bf16_codes", facts)
    assert facts["codes_in_a"] == facts["codes_in_b"] == 65024 + 2
    assert not wrong, wrong[:12]


def test_bf16_subnormal_operands_give_the_product_or_zero(P):
    """Recorded, not established: whether a bf16 operand with exponent field 0 is used or flushed. Asserted is
    only that each word is the exact product (a normal fp32: the partner is 2^127 or -2^100) or +0."""
    results = [r for r in run_code_tiles(P, K.subnormal_code_tiles()) if r[1] & 0x7FFF]   # without the groups' +-0
    by_side = {}
    neither = []
    for side in (0, 1):
        kinds = collections.Counter()
        for s, code, partner, want, got in results:
            if s != side:
                continue
            assert want != 0
            kind = "product" if got == want else "flushed" if got == 0 else "neither"
            kinds[kind] += 1
            if kind == "neither":
                neither.append((side, hex(code), partner, hex(want), hex(got)))
        by_side["a" if side == 0 else "b"] = dict(kinds)
    same = len({k for kinds in by_side.values() for k in kinds}) == 1
    facts = {"by_operand": by_side, "same_for_all_codes": same,
             "codes": len({code for _s, code, *_ in results})}
    print(facts, neither[:12])
    record("basic_selftest_bf16_subnormal_operands", facts)
    assert facts["codes"] == 254
    assert not neither, neither[:12]


@pytest.mark.parametrize("side", [0, 1])
def test_gemm_tile_rounds_its_operands_as_torch_does(P, side):
    """512 float32 values that are no bf16 values against the one-term selection of ones: C[r][c] is the
    value as the host's rounding left it, which must be torch's round-to-nearest-even, bit for bit."""
    import torch

    a, b = K.rounding_tile(side)
    values = torch.tensor(a if side == 0 else b, dtype=torch.float32)
    assert values.view(torch.int32).tolist() == [w - (1 << 32) if w >> 31 else w for w in K.rounding_patterns()]
    rounded = values.bfloat16().float()
    assert int((rounded != values).sum()) == 512                        # every one of them is rounded
    if side == 0:
        want = rounded.view(32, 16)[:, torch.arange(32) % 16]           # C[r][c] = A[r][c % 16]
    else:
        want = rounded.view(16, 32)[torch.arange(32) % 16, :]           # C[r][c] = B[r % 16][c]
    got = words(P.gemm_tile(a, b))
    assert (got == want.contiguous().view(torch.int32).numpy().view(np.uint32).ravel()).all()


def test_mfma_burn_sums_refuses_a_burn(P):
    for blocks, iters in ((0, 8), (9, 8), (2, 0), (2, 1025)):
        with pytest.raises(ValueError):
            P.mfma_burn_sums(0, blocks, iters)


def test_the_burn_adds_four_chains_an_iteration(P):
    """Every thread's sum against s_ref = iters * s1, s1 from the faithful maps in exact arithmetic, within
    |s - s_ref| <= N * 2^-24 * S: the standard forward bound of N fp32 additions on the way of one value
    (16 iters inside the MFMAs, 64 in the final reduction) over terms whose magnitudes sum to S (= s_ref:
    every term is >= 0). One iteration more or fewer is s1 away, which exceeds the bounds of adjacent
    iteration counts together; a dropped chain is that chain's part of s_ref away, which exceeds the
    bound: both asserted here and in tests/test_basic_selftest.py."""
    s1 = K.burn_reference(P.bf16_bits)
    assert (s1 > 0).all()
    for chain in range(4):
        part = K.burn_reference(P.bf16_bits, chains=(chain,))
        for iters in (1, 8, 9, 64):
            assert all(iters * part[lane] > K.burn_bound(iters, s1[lane]) for lane in range(64))
    worst = {}
    for iters in (1, 8, 9, 64):
        sums = np.array(P.mfma_burn_sums(0, 2, iters), dtype=np.float64)
        assert sums.shape == (512,)
        ref = iters * np.tile(s1, 8)
        bound = np.array([K.burn_bound(iters, v) for v in np.tile(s1, 8)])
        err = np.abs(sums - ref)
        worst[iters] = float((err / bound).max())
        print("iters", iters, "largest |s - s_ref| / bound:", worst[iters])
        assert (err <= bound).all(), (iters, int(np.argmax(err / bound)), float(err.max()))
    for lane in range(64):
        assert s1[lane] > K.burn_bound(8, s1[lane]) + K.burn_bound(9, s1[lane])
    record("basic_selftest_burn_sums_error_over_bound", {str(k): round(v, 4) for k, v in worst.items()})
