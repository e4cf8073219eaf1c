"""The GEMM tenant on a real MI355X (`pytest -m gpu`): `gemm_bf16` against integer and float64 products at the
smallest shapes at which the kernel (128 x 128 tiles of C, K in LDS tiles of 64, two stages) can go wrong, and the
host code of `gemm_throughput` and `gemm_colocated`: the shape they echo, the rates' formulas, every refusal.
The rates themselves are profiles/gpu_calibration.md's to record; nothing here provokes a fault, a timeout or an
out-of-memory."""
import math

import numpy as np
import pytest

from gpu_harness import P   # tests/ is on sys.path (no package)

pytestmark = pytest.mark.gpu

MIB = 1 << 20


def gemm(P, a, b):
    (m, k), n = a.shape, b.shape[1]
    c = P.gemm_bf16(a.ravel().tolist(), b.ravel().tolist(), m, n, k)
    return np.array(c, dtype=np.float64).reshape(m, n)


@pytest.mark.parametrize("m,n,k", [
    (128, 128, 64),    # one workgroup, one K tile
    (128, 128, 128),   # both LDS stages
    (128, 128, 192),   # a stage reused, odd tile count
    (256, 128, 64),    # two tiles along M only
    (128, 256, 64),    # two tiles along N only
    (384, 640, 192),   # 15 workgroups: more than 8, no multiple of 8, row tiles != column tiles
])
def test_integer_operands_give_the_exact_product(P, m, n, k):
    """Seeded integers in +-1..8: every sum is below 192 * 64 < 2^24, so every fp32 partial sum is exact in any
    order and the comparison needs no tolerance."""
    rng = np.random.default_rng(m * 1_000_003 + n * 1_009 + k)
    a = rng.integers(1, 9, (m, k)) * rng.choice([-1, 1], (m, k))
    b = rng.integers(1, 9, (k, n)) * rng.choice([-1, 1], (k, n))
    assert np.linalg.matrix_rank(a.astype(np.float64)) == min(m, k) and np.linalg.matrix_rank(b.astype(np.float64)) == min(k, n)
    want = a.astype(np.int64) @ b.astype(np.int64)
    got = gemm(P, a.astype(np.float32), b.astype(np.float32))
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:8].tolist())


def test_rounded_operands_within_the_forward_bound_of_fp32_accumulation(P):
    """Normal floats, rounded to bf16 as the binding rounds them: the products of two bf16 values are exact in fp32,
    so what remains is the accumulation of K terms, bounded elementwise by K * 2^-24 * (|A| |B|)[i][j]."""
    m, n, k = 256, 256, 192
    rng = np.random.default_rng(20250)
    a, b = rng.standard_normal((m, k)).astype(np.float32), rng.standard_normal((k, n)).astype(np.float32)

    def rounded(x):
        codes = np.array(P.bf16_bits(x.ravel()), dtype=np.uint32) << 16
        return codes.view(np.float32).astype(np.float64).reshape(x.shape)

    ra, rb = rounded(a), rounded(b)
    got = gemm(P, a, b)
    err, bound = np.abs(got - ra @ rb), k * 2.0 ** -24 * (np.abs(ra) @ np.abs(rb))
    print(f"largest error / bound: {float((err / bound).max()):.4f}")
    assert (err <= bound).all(), float((err / bound).max())


def is_rate(x) -> bool:
    return isinstance(x, float) and math.isfinite(x) and x > 0


def test_throughput_echoes_its_shape_and_follows_its_formulas(P):
    m, n, k, iters = 256, 384, 128, 3
    r = P.gemm_throughput(0, [], m, n, k, iters)
    assert (r["m"], r["n"], r["k"], r["iters"]) == (m, n, k, iters) and r["ms"] > 0, r
    assert r["tflops"] == pytest.approx(2 * m * n * k * iters / (r["ms"] * 1e-3) / 1e12, rel=1e-6), r
    assert r["gbs"] == pytest.approx((2 * k * (m + n) + 4 * m * n) * iters / (r["ms"] * 1e-3) / 1e9, rel=1e-6), r


@pytest.fixture(scope="module")
def masks():
    """The agent's disjoint 25 % / 75 % masks of a 256-CU device, as mask words."""
    from nanogpu.agent import cumask

    d = cumask.DeviceCUs(256, 8)
    a, b = d.grant("a", 25), d.grant("b", 75)
    return cumask.mask_words(a), cumask.mask_words(b)


def test_colocated_small_gives_two_rates(P, masks):
    rates = P.gemm_colocated(0, masks[1], masks[0], 512, 384, 128, 2, 4 * MIB, 2)
    assert len(rates) == 2 and all(is_rate(r) for r in rates), rates


BIG = 128 * 4096   # BIG x BIG is 2^24 workgroups: 2^32 work-items in one launch


def shapes(*more):
    """(m, n, k) no tile divides, zero sizes, and the launch that is too large."""
    return [(100, 128, 64), (128, 130, 64), (128, 128, 32), (0, 128, 64), (128, 0, 64), (128, 128, 0), (BIG, BIG, 64), *more]


def refusals(masks):
    a, b = masks
    ones = [1.0] * (128 * 128)
    return {
        "gemm_bf16": ([(ones, ones, *s) for s in shapes((1152, 128, 64), (128, 128, 1088))] + [(ones[:-1], ones, 128, 128, 128)],
                      (ones[:128 * 64], ones[:64 * 128], 128, 128, 64)),
        "gemm_throughput": ([(0, [], *s, 2) for s in shapes()] + [(0, [], 128, 128, 64, 0), (0, [], 128, 128, 64, 2**24)],
                            (0, [], 128, 128, 64, 2)),
        "gemm_colocated": ([(0, b, a, *s, 2, 4 * MIB, 2) for s in shapes()] +
                           [(0, b, a, 128, 128, 64, 0, 4 * MIB, 2), (0, b, a, 128, 128, 64, 2, 15, 2),
                            (0, b, a, 128, 128, 64, 2, 4 * MIB, 0), (0, b, a, 128, 128, 64, 2, 1 << 38, 2)],
                           (0, b, a, 128, 128, 64, 2, 4 * MIB, 2)),
    }


@pytest.mark.parametrize("name", ["gemm_bf16", "gemm_throughput", "gemm_colocated"])
def test_refusals_raise_value_error_and_leave_the_binding_usable(P, masks, name):
    """Every refusal comes before any allocation or launch, and the proper call straight after each one succeeds."""
    refused, proper = refusals(masks)[name]
    fn = getattr(P, name)
    for args in refused:
        with pytest.raises(ValueError):
            fn(*args)
        assert fn(*proper)
