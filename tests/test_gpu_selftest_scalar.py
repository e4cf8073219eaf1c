"""Scalar part of the deep self-test on a real MI355X: the kernels' instruction sequences are the
twin's arithmetic, a clean device passes on every CU, and every compared word, every kind of
injected fault and every mask is seen. Nothing here corrupts anything but data the kernel owns or
the host's own upload."""
import time

import pytest

from gpu_harness import SEED, P, a_cu, assert_fails_exactly, sweep_all   # tests/ is on sys.path (no package)
from nanogpu.probe.selftest_scalar import GROUPS, PART

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def clean(P):
    return sweep_all(P, PART, GROUPS)


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
    cu = a_cu(clean[0]["records"])
    r, f = sweep_all(P, PART, GROUPS, inject=cu + (kind, arg))
    rep = assert_fails_exactly(PART, GROUPS, f, cu, arg if kind == "scalar" else kind)
    c = f["cus"][0]
    wave = arg // 1024 if kind == "smem" else 0
    assert c["waves"] == 1 << wave
    assert (c["bad_slot"], c["bad_slot_wave"]) == ((arg, 0) if kind == "sregs" else (-1, -1))
    assert (c["bad_word"], c["bad_word_wave"]) == ((arg, wave) if kind == "smem" else (-1, -1))
    if kind == "sregs":
        assert f"at slot {arg}, wave 0" in rep.describe_failure()
    if kind == "smem":
        assert f"at word {arg}, wave {wave}" in rep.describe_failure()


def test_corrupt_expected_fails_that_wave_of_every_record(P):
    from nanogpu.probe.selftest_common import mix32
    from nanogpu.probe.selftest_scalar import EXACT_GROUPS

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
