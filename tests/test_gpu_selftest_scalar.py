"""Scalar part of the deep self-test on a real MI355X: the kernels' instruction sequences are the
twin's arithmetic, a clean device passes on every CU, and every compared word, every kind of
injected fault and every mask is seen. Nothing here corrupts anything but data the kernel owns or
the host's own upload."""
import statistics
import time

import pytest

pytestmark = pytest.mark.gpu

SEED = 0x1234ABCD


def record(key: str, value) -> None:
    """Measured facts for profiles/gpu_calibration.md, into the same file as test_gpu.py's."""
    from test_gpu import record as record_fact   # tests/ is on sys.path (no package)

    record_fact(key, value)


@pytest.fixture(scope="module")
def P():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    from nanogpu.native import probe

    return probe(required=True)


def _sweep_all(P, groups, rounds=4, inject=None, corrupt=None, mask=(), cus=256):
    """One sweep (unmasked, or of the `cus` CUs of `mask`) with deep_selftest's own policy for coverage
    (doubled rounds, three launches)."""
    from nanogpu.probe.selftest_scalar import fold_scalar

    mask = list(mask)
    r = P.cu_sweep_scalar(0, mask, rounds, SEED, groups, inject, corrupt)
    records = list(r["records"])
    for more in (rounds * 2, rounds * 4):
        if fold_scalar(records, r["groups"], cus)["cus_uncovered"] == 0:
            break
        records += list(P.cu_sweep_scalar(0, mask, more, SEED, groups, inject, corrupt)["records"])
    r["records"] = records
    return r, fold_scalar(records, r["groups"], cus)


@pytest.fixture(scope="module")
def clean(P):
    from nanogpu.probe.selftest_scalar import GROUPS

    return _sweep_all(P, list(GROUPS))


def test_every_exact_group_is_the_twins_arithmetic(P):
    from nanogpu.probe import selftest_scalar as V

    for g in V.EXACT_GROUPS:
        got = [int(w) for w in P.scalar_words(g)]
        want = V.group_expected(g)[0]
        diff = [(i // 8, i % 8, hex(a), hex(b)) for i, (a, b) in enumerate(zip(got, want)) if a != b]
        print(g, "differing (wave, word, device, twin):", diff[:8])
        assert not diff, (g, len(diff), diff[:4])


def test_clean_sweep_covers_every_cu(P, clean):
    from nanogpu.probe.selftest_scalar import SREG_SLOTS

    r, f = clean
    print({k: r[k] for k in ("sreg_slots", "num_regs", "scratch_bytes", "ms")}, f["cus_seen"])
    assert f["cus_seen"] == 256 and f["cus_uncovered"] == 0 and f["failed"] == {}
    assert all(rec[2] == 0 and rec[4] == 0 and rec[5] == rec[6] == rec[7] == -1 for rec in r["records"])
    assert all(rec[3] == 0xF for rec in r["records"])
    assert r["scratch_bytes"] == 0 and r["sreg_slots"] == SREG_SLOTS >= 80
    assert r["checked"] == list(r["groups"]) and len(r["groups"]) == 9


@pytest.mark.parametrize("kind,arg", [("scalar", "add"), ("scalar", "cmp"), ("scalar", "vcc"), ("smem", 0), ("smem", 4095),
                                      ("sregs", 0), ("sregs", 87)])
def test_injection_fails_exactly_that_cu_and_kind(P, clean, kind, arg):
    """An exact group and the registers are corrupted on wave 0. A table word is read by one wave only (wave w
    reads quarter w), so word 4095 fails on wave 3, the wave that compares it, and word 0 on wave 0."""
    from nanogpu.probe import selftest as S
    from nanogpu.probe import selftest_common as C
    from nanogpu.probe.selftest_scalar import GROUPS

    rec = clean[0]["records"][len(clean[0]["records"]) // 3]
    cu = (rec[0], C.cu_key(rec[1]))
    r, f = _sweep_all(P, list(GROUPS), inject=cu + (kind, arg))
    name = arg if kind == "scalar" else kind
    assert f["failed"] == {name: [list(cu)]}, f["failed"]
    assert f["cus_seen"] == 256
    c = f["cus"][0]
    wave = arg // 1024 if kind == "smem" else 0
    assert c["waves"] == 1 << wave
    assert (c["bad_slot"], c["bad_slot_wave"]) == ((arg, 0) if kind == "sregs" else (-1, -1))
    assert (c["bad_word"], c["bad_word_wave"]) == ((arg, wave) if kind == "smem" else (-1, -1))
    rep = S.DeepReport(device=0, ok=False, scalar={"checked": list(GROUPS), "failed": f["failed"], "cus": f["cus"]})
    assert S.fenceable(rep) and S.failed_cus(rep) == {cu}
    if kind == "sregs":
        assert f"at slot {arg}, wave 0" in rep.describe_failure()
    if kind == "smem":
        assert f"at word {arg}, wave {wave}" in rep.describe_failure()


def test_corrupt_expected_fails_that_wave_of_every_record(P):
    from nanogpu.probe.selftest_common import mix32
    from nanogpu.probe.selftest_scalar import EXACT_GROUPS, GROUPS

    for i, g in enumerate(EXACT_GROUPS):
        word = mix32(i) % 32
        r = P.cu_sweep_scalar(0, [], 1, SEED, list(GROUPS), None, (g, word, 1 << (mix32(word) & 31)))
        assert r["records"] and all(rec[2] == 1 << (word // 8) and rec[4] == 1 << i and rec[5] == -1 for rec in r["records"]), g
    r = P.cu_sweep_scalar(0, [], 1, SEED, list(GROUPS), None, ("smem", 2049, 1 << 30))
    assert r["records"] and all(rec[2] == 0x10 << 2 and rec[4] == 0 and rec[5:] == (2049, 2, 1) for rec in r["records"])


def test_every_word_of_every_table_can_fail_the_sweep(P):
    from nanogpu.probe.selftest_common import mix32
    from nanogpu.probe.selftest_scalar import EXACT_GROUPS

    t0 = time.perf_counter()
    for i, g in enumerate(EXACT_GROUPS):
        r = P.scalar_sensitivity(0, g, [(w, 1 << (mix32(w) & 31)) for w in range(32)])
        assert r["records"] >= 256 and len(r["words"]) == 32
        for w, (a, o) in enumerate(r["words"]):
            assert a[1] == 1 << i == o[1], (g, w, a, o)             # AND: the group's bit on every record; OR: no foreign bit
            assert a[0] == 1 << (w // 8) == o[0], (g, w, a, o)      # the word's own wave, and no other kind
            assert a[2] == -1 == o[2], (g, w, a, o)
    print(f"sensitivity: {32 * len(EXACT_GROUPS)} sweeps in {time.perf_counter() - t0:.2f} s")


def test_every_word_of_the_load_table_can_fail_the_sweep(P):
    """All 4096 words, 512 a call (a sweep takes a fraction of a millisecond); the time is printed."""
    from nanogpu.probe.selftest_common import mix32

    t0 = time.perf_counter()
    for first in range(0, 4096, 512):
        r = P.scalar_sensitivity(0, "smem", [(w, 1 << (mix32(w) & 31)) for w in range(first, first + 512)])
        assert r["records"] >= 256 and len(r["words"]) == 512
        for k, (a, o) in enumerate(r["words"]):
            w = first + k
            assert a[0] == 0x10 << (w // 1024) == o[0], (w, a, o)   # the smem bit of the wave that reads the word
            assert a[1] == 0 == o[1] and a[2] == w == o[2], (w, a, o)
    print(f"smem sensitivity: 4096 sweeps in {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("group,fails", [("add", (1, 1, -1)), ("smem", (0x10, 0, 5))])
def test_a_flipped_word_is_restored_before_the_next_flip(P, group, fails):
    """A word left corrupted would hide behind the next one's failure. A zero XOR of the word flipped before is
    clean on every record: the XOR starts from the host's word each time, and the host's table was not written. A
    zero XOR of another word is clean only if the word flipped before was put back; the words around both must
    still fail."""
    def words(flips):
        return [tuple(tuple(half) for half in w) for w in P.scalar_sensitivity(0, group, flips)["words"]]

    bad5, clean = (fails, fails), ((0, 0, -1), (0, 0, -1))
    bad6 = tuple(f[:2] + ((6,) if group == "smem" else (-1,)) for f in bad5)
    assert words([(5, 1 << 3), (5, 0), (6, 1 << 9)]) == [bad5, clean, bad6]
    assert words([(5, 1 << 3), (6, 0), (6, 1 << 9)]) == [bad5, clean, bad6]   # word 5 restored


def test_masked_to_one_unit(P):
    from nanogpu.agent import cumask
    from nanogpu.probe.selftest_scalar import GROUPS

    mask = cumask.mask_words(list(range(5 * 8, 6 * 8)), 256)             # unit 5
    r, f = _sweep_all(P, list(GROUPS), mask=mask, cus=8)
    assert f["cus_seen"] == 8 and f["cus_uncovered"] == 0 and f["failed"] == {} and len(r["records"]) % 8 == 0
    assert sorted({rec[0] for rec in r["records"]}) == list(range(8))     # one CU per XCD
    ours = {(rec[0], (rec[1] >> 8) & 0xFF) for rec in r["records"]}
    # which CUs the unit is: what the census kernel reports from a stream with the same mask
    unit = {(xcc, (hw_id >> 8) & 0xFF) for xcc, hw_id in P.cu_census(0, mask, 512, 64)}
    assert len(unit) == 8 and ours == unit


def test_deep_selftest_with_all_parts_and_the_metric(P):
    from nanogpu.agent.metrics import render
    from nanogpu.probe import selftest as S
    from nanogpu.topology.model import synthetic_mi355x

    rep = S.deep_selftest(P, 0, scalar="all", valu="all", paths="all")
    assert rep.ok, rep.describe_failure()
    assert len(rep.scalar["checked"]) == 9 and rep.scalar["failed"] == {} and rep.scalar["sreg_slots"] == 88 and rep.scalar["ms"] > 0
    assert len(rep.valu["checked"]) == 13 and len(rep.paths["checked"]) == 9 and rep.sweep["cus_seen"] == 256
    stats = {"reports": {0: rep.to_dict()}, "at": {0: time.time()}, "runs": {(0, "pass"): 1}}
    assert 'nanogpu_selftest_scalar_checked{device="0"} 9' in render(synthetic_mi355x(1), None, None, "/nonexistent", stats)


def test_cost_of_the_scalar_launch(P):
    """No threshold: the window in which a new grant could share CUs with the test is reported."""
    from nanogpu.probe.selftest_scalar import GROUPS

    plain, scalar, last = [], [], {}
    for _ in range(11):                                   # interleaved pairs in one process
        plain.append(P.cu_sweep(0, [], 4, SEED)["ms"])
        last = P.cu_sweep_scalar(0, [], 4, SEED, list(GROUPS))
        scalar.append(last["ms"])
    facts = {"sweep_ms": statistics.median(plain), "scalar_ms": statistics.median(scalar),
             "sweep_plus_scalar_ms": statistics.median(a + b for a, b in zip(plain, scalar)), "pairs": len(plain)}
    print("scalar cost", facts)
    record("selftest_scalar_cost", facts)
    record("selftest_scalar_regs", {"sreg_slots": last["sreg_slots"], "num_regs": last["num_regs"], "scratch_bytes": last["scratch_bytes"]})
