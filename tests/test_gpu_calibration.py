"""The calibration rate probes' host code on a real MI355X (`pytest -m gpu`): `hbm_bandwidth`, `mfma_throughput`,
`mfma_colocated`, `hbm_colocated` and `mixed_colocated` are one list of tenants each behind one runner, and these
are the smallest shapes at which that host code can go wrong: the order of the results, the iteration count a rate
is charged with, the copy kernel's tail, the fill that precedes the census, and every refusal. The rates
themselves are test_gpu.py's to record; nothing here provokes a fault, a timeout or an out-of-memory."""
import math

import pytest

pytestmark = pytest.mark.gpu

MIB = 1 << 20


@pytest.fixture(scope="module")
def P():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    from nanogpu.native import probe

    return probe(required=True)


@pytest.fixture(scope="module")
def masks():
    """The agent's disjoint 25 % / 75 % masks of a 256-CU device, as mask words."""
    from nanogpu.agent import cumask

    d = cumask.DeviceCUs(256, 8)
    a, b = d.grant("a", 25), d.grant("b", 75)
    return cumask.mask_words(a), cumask.mask_words(b)


def is_rate(x) -> bool:
    return isinstance(x, float) and math.isfinite(x) and x > 0


@pytest.mark.parametrize("iters_each", [[], [1, 3, 2]], ids=["iters", "iters_each"])
@pytest.mark.parametrize("tenants", [1, 2, 3])
def test_hbm_colocated_runs_the_copy_tail_for_every_mask(P, masks, tenants, iters_each):
    """4 MiB + 16 bytes are 262,145 float4, no multiple of the 1,024 a block copies: the last block takes the
    kernel's tail branch. One rate per mask, in mask order."""
    cu_masks = [masks[0], masks[1], []][:tenants]
    rates = P.hbm_colocated(0, cu_masks, 4 * MIB + 16, 2, iters_each[:tenants])
    assert len(rates) == tenants and all(is_rate(r) for r in rates), rates


def test_mfma_colocated_small(P, masks):
    rates = P.mfma_colocated(0, list(masks), [8, 24], 64)
    assert len(rates) == 2 and all(is_rate(r) for r in rates), rates


def test_mixed_colocated_small_gives_copy_rate_then_burn_rate(P, masks):
    rates = P.mixed_colocated(0, masks[0], masks[1], 4 * MIB, 2, 24, 256)
    assert len(rates) == 2 and all(is_rate(r) for r in rates), rates
    gbs, tflops = rates
    # Which is which: 24 blocks are 96 waves, and even one to a SIMD at the chip's 2.5 PF/s bf16 peak over its
    # 1,024 SIMDs they stay below 235 TF/s. The copies move 2 x 2 x 4 MiB: below 250 GB/s they would take over
    # 33 us each, where 64 CUs stream a copy of 4 MiB in about 3 us (2,963 GB/s recorded) after a launch of a few us.
    assert tflops < 250 < gbs, rates


def test_hbm_bandwidth_small(P):
    assert is_rate(P.hbm_bandwidth(0, 16 * MIB, 2))


def test_mfma_throughput_small_echoes_its_shape(P):
    r = P.mfma_throughput(0, [], 64, 64)
    assert r["ms"] > 0 and is_rate(r["tflops"]), r
    assert (r["blocks"], r["iters"]) == (64, 64), r
    # tflops is burn_tflops over the same ms: 4 chains x 4 waves x 32,768 FLOP an instruction
    assert r["tflops"] == pytest.approx(4 * 32768 * 64 * 64 * 4 / (r["ms"] * 1e-3) / 1e12, rel=1e-6), r


def test_copy_rate_is_charged_with_its_own_iteration_count(P):
    """The same copy at 2 and at 8 iterations gives the same rate. Charging the wrong count moves the rate by
    the ratio of the counts, 4; the launch overhead of a copy of about 90 us cannot move it by 2."""
    r2 = P.hbm_colocated(0, [[]], 256 * MIB, 2)[0]
    r8 = P.hbm_colocated(0, [[]], 256 * MIB, 8)[0]
    print(f"hbm_colocated 256 MiB: {r2:.1f} GB/s at 2 iterations, {r8:.1f} GB/s at 8")
    assert 0.5 < r2 / r8 < 2.0, (r2, r8)


def test_burn_rate_is_charged_with_its_own_iteration_count(P):
    """As above for the burn: 2,048 blocks take about 145 us at 256 iterations."""
    r256 = P.mfma_throughput(0, [], 2048, 256)["tflops"]
    r1024 = P.mfma_throughput(0, [], 2048, 1024)["tflops"]
    print(f"mfma_throughput 2048 blocks: {r256:.1f} TF/s at 256 iterations, {r1024:.1f} TF/s at 1024")
    assert 0.5 < r256 / r1024 < 2.0, (r256, r1024)


def test_census_fill_lands_before_the_kernel(P):
    """The records are filled with 0xff on the kernel's own stream: a fill that landed after the kernel would
    show as xcc 0xffffffff."""
    recs = P.cu_census(0, [], 256, 1)
    assert len(recs) == 256
    assert all(0 <= x <= 7 for x, _ in recs), sorted({x for x, _ in recs})


def refusals(masks):
    """(binding, refused arguments..., proper arguments): every refusal the five rate probes make."""
    a, b = masks
    return {
        "hbm_bandwidth": ([(0, 15, 2), (0, 16 * MIB, 0), (0, 1 << 38, 2)], (0, 16 * MIB, 2)),
        "mfma_throughput": ([(0, [], 0, 64), (0, [], 64, 0), (0, [], 2**24, 64)], (0, [], 64, 64)),
        "mfma_colocated": ([(0, [], [], 64), (0, [a, b], [8], 64), (0, [a, b], [8, 24, 8], 64), (0, [a, b], [8, 24], 0),
                            (0, [a, b], [8, 2**24], 64), (0, [a, b], [0, 24], 64)], (0, [a, b], [8, 24], 64)),
        "hbm_colocated": ([(0, [], 4 * MIB, 2), (0, [a, b], 15, 2), (0, [a, b], 4 * MIB, 0),
                           (0, [a, b], 4 * MIB, 2, [1]), (0, [a, b], 4 * MIB, 2, [1, 2, 3]),
                           (0, [a, b], 4 * MIB, 2, [1, 1001]), (0, [a, b], 4 * MIB, 2, [0, 1]),
                           (0, [a, b], 1 << 38, 2)], (0, [a, b], 4 * MIB, 2)),
        "mixed_colocated": ([(0, a, b, 15, 2, 24, 256), (0, a, b, 4 * MIB, 0, 24, 256), (0, a, b, 4 * MIB, 2, 0, 256),
                             (0, a, b, 4 * MIB, 2, 24, 0), (0, a, b, 4 * MIB, 2, 2**24, 256),
                             (0, a, b, 1 << 38, 2, 24, 256)], (0, a, b, 4 * MIB, 2, 24, 256)),
    }


@pytest.mark.parametrize("name", ["hbm_bandwidth", "mfma_throughput", "mfma_colocated", "hbm_colocated",
                                  "mixed_colocated"])
def test_refusals_raise_value_error_and_leave_the_binding_usable(P, masks, name):
    """Every refusal comes before any allocation or launch (2^38 bytes and 2^24 blocks would need 2^32
    work-items in one launch), and the proper call straight after each one succeeds."""
    refused, proper = refusals(masks)[name]
    fn = getattr(P, name)
    for args in refused:
        with pytest.raises(ValueError):
            fn(*args)
        assert fn(*proper)


def test_peer_bandwidth_refuses_one_device_and_measures_two(P):
    with pytest.raises(ValueError):
        P.peer_bandwidth(0, 0, MIB, 1)
    if P.device_count() < 2:
        pytest.skip("single visible GPU")
    r = P.peer_bandwidth(0, 1, MIB, 1)
    assert is_rate(r["dma_gbs"]), r
