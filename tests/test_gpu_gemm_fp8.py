"""The FP8 GEMM tenant on a real MI355X (`pytest -m gpu`): `gemm_fp8` against the integer product at the smallest
shapes at which the kernel (128 x 128 tiles of C, K in LDS tiles of 128, two stages, B stored [N][K]) can go wrong,
and the `dtype` option of `gemm_throughput` and `gemm_colocated`: what they echo, the formulas, every refusal. The
rates themselves are profiles/gpu_calibration.md's to record."""
import numpy as np
import pytest

from gpu_harness import P   # tests/ is on sys.path (no package)
from test_gpu_gemm import MIB, is_rate, masks, shapes

pytestmark = pytest.mark.gpu


def codes_and_eighths(rng, rows, k):
    """Random e4m3 codes sign | exponent field 7 or 8 | any mantissa, and 8 x their values: integers of 8..30 in size."""
    sign, exp, mant = rng.integers(0, 2, (rows, k)), rng.integers(7, 9, (rows, k)), rng.integers(0, 8, (rows, k))
    codes = (sign << 7 | exp << 3 | mant).astype(np.uint8)
    return codes, ((8 + mant) << (exp - 7)) * (1 - 2 * sign)


@pytest.mark.parametrize("m,n,k", [
    (128, 128, 128),   # one workgroup, one K tile
    (128, 128, 256),   # both LDS stages
    (128, 128, 384),   # a stage reused
    (256, 128, 128),   # two tiles along M only
    (128, 256, 128),   # two tiles along N only
    (384, 640, 384),   # 15 workgroups: more than 8, no multiple of 8, row tiles != column tiles
])
def test_codes_give_the_exact_product(P, m, n, k):
    """|values| in 1 .. 3.75 in eighths: 64 a b is an integer of at most 900, and 64 times any partial sum of up to
    1,024 terms an integer below 2^20, so every fp32 partial sum is exact in any order and the comparison needs no
    tolerance. The reference decodes the codes' three fields itself."""
    rng = np.random.default_rng(m * 1_000_003 + n * 1_009 + k)
    (a, a8), (b, b8) = codes_and_eighths(rng, m, k), codes_and_eighths(rng, n, k)
    assert np.linalg.matrix_rank(a8.astype(np.float64)) == min(m, k) and np.linalg.matrix_rank(b8.astype(np.float64)) == min(n, k)
    want = (a8.astype(np.int64) @ b8.astype(np.int64).T) / 64.0
    got = np.array(P.gemm_fp8(a.ravel(), b.ravel(), m, n, k), dtype=np.float64).reshape(m, n)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:8].tolist())


def test_throughput_echoes_its_shape_and_dtype_and_follows_its_formulas(P):
    m, n, k, iters = 256, 384, 256, 3
    r = P.gemm_throughput(0, [], m, n, k, iters, "fp8")
    assert (r["m"], r["n"], r["k"], r["iters"], r["dtype"]) == (m, n, k, iters, "fp8") and r["ms"] > 0, r
    assert r["tflops"] == pytest.approx(2 * m * n * k * iters / (r["ms"] * 1e-3) / 1e12, rel=1e-6), r
    assert r["gbs"] == pytest.approx((k * (m + n) + 4 * m * n) * iters / (r["ms"] * 1e-3) / 1e9, rel=1e-6), r


def test_colocated_small_gives_two_rates(P, masks):
    rates = P.gemm_colocated(0, masks[1], masks[0], 512, 384, 256, 2, 4 * MIB, 2, "fp8")
    assert len(rates) == 2 and all(is_rate(r) for r in rates), rates


def refusals(masks):
    a, b = masks
    ones = np.full(128 * 128, 0x38, dtype=np.uint8)
    odd = shapes((128, 128, 64), (128, 128, 192))   # a K tile of the bf16 kernel is half of this one's
    return {
        "gemm_fp8": ([(ones, ones, *s) for s in odd + [(1152, 128, 128)]] + [(ones[:-1], ones, 128, 128, 128), (ones, ones[:-1], 128, 128, 128)],
                     (ones, ones.tolist(), 128, 128, 128)),
        "gemm_throughput": ([(0, [], *s, 2, "fp8") for s in odd] + [(0, [], 128, 128, 128, 2, "fp4")], (0, [], 128, 128, 128, 2, "fp8")),
        "gemm_colocated": ([(0, b, a, *s, 2, 4 * MIB, 2, "fp8") for s in odd] + [(0, b, a, 128, 128, 128, 2, 4 * MIB, 2, "fp4")],
                           (0, b, a, 128, 128, 128, 2, 4 * MIB, 2, "fp8")),
    }


@pytest.mark.parametrize("name", ["gemm_fp8", "gemm_throughput", "gemm_colocated"])
def test_refusals_raise_value_error_and_leave_the_binding_usable(P, masks, name):
    """Every refusal comes before any allocation or launch, and the proper call straight after each one succeeds."""
    refused, proper = refusals(masks)[name]
    fn = getattr(P, name)
    for args in refused:
        with pytest.raises(ValueError):
            fn(*args)
        assert fn(*proper)
