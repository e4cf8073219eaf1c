"""The attention tenant on a real MI355X (`pytest -m gpu`): `attn_bf16` against an exact gather and a float64 softmax at
the smallest shapes at which its two kernels (wide: 128 queries a workgroup, K/V tiles of 64 in two LDS stages; split: 32
queries, tiles of 128 shared out among four waves and merged) can go wrong, and the host code of `attn_throughput` and
`attn_colocated`. The rates are profiles/gpu_calibration.md's to record; nothing here provokes a fault, a timeout or an
out-of-memory."""
import math

import numpy as np
import pytest

from gpu_harness import P   # tests/ is on sys.path (no package)

pytestmark = pytest.mark.gpu

MIB = 1 << 20
WIDE = [(1, 128, 64), (1, 128, 128), (1, 128, 192), (1, 256, 64), (3, 128, 64), (5, 384, 192)]
SPLIT = [(1, 32, 128), (1, 32, 256), (1, 32, 384), (1, 96, 128), (5, 96, 384)]


def attn(P, q, k, v):
    (heads, sq, _), skv = q.shape, k.shape[1]
    o = P.attn_bf16(q.ravel().tolist(), k.ravel().tolist(), v.ravel().tolist(), heads, sq, skv)
    return np.array(o, dtype=np.float64).reshape(heads, sq, 128)


@pytest.mark.parametrize("heads,sq,skv", WIDE + SPLIT)
def test_one_hot_scores_gather_rows_of_v_bit_for_bit(P, heads, sq, skv):
    """K's rows are rows of [H; -H; 0 ...], H the 128 x 128 Hadamard matrix, cut to skv and permuted; query q is 16 H[q mod
    min(128, skv)] (so that its target is among the rows kept when skv is 64). The target row scores 2048 and every
    other 0 or -2048: in the exp2 domain the gap is 2048 log2(e) / sqrt(128) = 261, so every other weight and every
    rescale across the target is exactly 0 in fp32, every partial sum is a sum of sixteenths below 2^24, and O[q] is
    V[target(q)] whatever the order of accumulation: no tolerance."""
    h = np.ones((1, 1))
    for _ in range(7):
        h = np.block([[h, h], [h, -h]])
    rows = np.vstack([h, -h, np.zeros((128, 128))])[:skv]
    rng = np.random.default_rng(9 + heads * 1_000_003 + sq * 1_009 + skv)
    perms = [rng.permutation(skv) for _ in range(heads)]
    k = np.stack([rows[p] for p in perms])
    q = np.broadcast_to(16 * h[np.arange(sq) % min(128, skv)], (heads, sq, 128))
    v = rng.integers(-127, 128, (heads, skv, 128)) / 16.0
    target = np.stack([np.argsort(p)[np.arange(sq) % min(128, skv)] for p in perms])   # where row q of H went
    assert set((target // 32).ravel()) == set(range(skv // 32)), "a target in every 32-row block of every tile"
    got = attn(P, q, k, v)
    want = np.stack([v[b][target[b]] for b in range(heads)])
    bad = np.argwhere(got != want)
    assert bad.size == 0, (len(bad), bad[:8].tolist())


@pytest.mark.parametrize("heads,sq,skv", [(2, 256, 1024), (1, 128, 64), (2, 32, 1024)])
def test_rounded_normals_within_the_bound_of_bf16_weights_and_fp32_sums(P, heads, sq, skv):
    """Against a float64 softmax of the operands as the binding rounds them, elementwise within (2^-7 + skv 2^-23) (P |V|):
    2^-8 for the weights' rounding to bf16 in the numerator, 2^-8 for a denominator that may sum rounded weights, and
    the fp32 accumulation of skv terms."""
    rng = np.random.default_rng(20251 + sq + skv)

    def rounded(shape):
        x = rng.standard_normal(shape).astype(np.float32)
        codes = np.array(P.bf16_bits(x.ravel()), dtype=np.uint32) << 16
        return x, codes.view(np.float32).astype(np.float64).reshape(shape)

    (q, rq), (k, rk), (v, rv) = rounded((heads, sq, 128)), rounded((heads, skv, 128)), rounded((heads, skv, 128))
    s = rq @ rk.transpose(0, 2, 1) / math.sqrt(128)
    p = np.exp(s - s.max(axis=2, keepdims=True))
    p /= p.sum(axis=2, keepdims=True)
    err, bound = np.abs(attn(P, q, k, v) - p @ rv), (2.0 ** -7 + skv * 2.0 ** -23) * (p @ np.abs(rv))
    print(f"largest error / bound: {float((err / bound).max()):.4f}")
    assert (err <= bound).all(), float((err / bound).max())


@pytest.mark.parametrize("heads,sq,skv,kernel", [(3, 256, 192, "wide"), (3, 96, 256, "split")])
def test_throughput_echoes_its_shape_and_follows_its_formulas(P, heads, sq, skv, kernel):
    r = P.attn_throughput(0, [], heads, sq, skv, 3)
    assert (r["heads"], r["sq"], r["skv"], r["iters"], r["kernel"]) == (heads, sq, skv, 3, kernel) and r["ms"] > 0, r
    assert r["tflops"] == pytest.approx(4 * heads * sq * skv * 128 * 3 / (r["ms"] * 1e-3) / 1e12, rel=1e-6), r
    assert r["gbs"] == pytest.approx((256 * heads * (sq + 2 * skv) + 512 * heads * sq) * 3 / (r["ms"] * 1e-3) / 1e9, rel=1e-6), r


@pytest.fixture(scope="module")
def masks():
    """The agent's disjoint 25 % / 75 % masks of a 256-CU device, as mask words."""
    from nanogpu.agent import cumask

    d = cumask.DeviceCUs(256, 8)
    a, b = d.grant("a", 25), d.grant("b", 75)
    return cumask.mask_words(a), cumask.mask_words(b)


def test_colocated_small_gives_two_rates(P, masks):
    rates = P.attn_colocated(0, masks[1], masks[0], 4, 256, 128, 2, 4 * MIB, 2)
    assert len(rates) == 2 and all(isinstance(r, float) and math.isfinite(r) and r > 0 for r in rates), rates


# (heads, sq, skv) no tile divides, sq = 160, zero sizes, and the launch of 2^24 workgroups
SHAPES = [(1, 100, 128), (1, 128, 100), (1, 32, 64), (1, 160, 128), (0, 128, 64), (1, 0, 64), (1, 128, 0), (1 << 24, 32, 128)]


def refusals(masks):
    a, b = masks
    ones = [1.0] * (128 * 128)
    return {
        "attn_bf16": ([(ones, ones, ones, *s) for s in SHAPES + [(9, 128, 64), (1, 640, 64), (1, 128, 1088)]] +
                      [(ones[:-1], ones, ones, 1, 128, 128)], (ones, ones[:64 * 128], ones[:64 * 128], 1, 128, 64)),
        "attn_throughput": ([(0, [], *s, 2) for s in SHAPES] + [(0, [], 1, 128, 64, 0), (0, [], 1, 128, 64, 2**24)],
                            (0, [], 1, 32, 128, 2)),
        "attn_colocated": ([(0, b, a, *s, 2, 4 * MIB, 2) for s in SHAPES] +
                           [(0, b, a, 1, 128, 64, 0, 4 * MIB, 2), (0, b, a, 1, 128, 64, 2**24, 4 * MIB, 2),
                            (0, b, a, 1, 128, 64, 2, 15, 2), (0, b, a, 1, 128, 64, 2, 4 * MIB, 0)],
                           (0, b, a, 1, 128, 64, 2, 4 * MIB, 2)),
    }


@pytest.mark.parametrize("name", ["attn_bf16", "attn_throughput", "attn_colocated"])
def test_refusals_raise_value_error_and_leave_the_binding_usable(P, masks, name):
    """Every refusal comes before any allocation or launch, and the proper call straight after each one succeeds."""
    refused, proper = refusals(masks)[name]
    fn = getattr(P, name)
    for args in refused:
        with pytest.raises(ValueError):
            fn(*args)
        assert fn(*proper)
