"""Vector-ALU part of the deep self-test on a real MI355X: the kernels' instruction sequences are
the twin's arithmetic, a clean device passes on every CU, and every compared word, every kind of
injected fault and every mask is seen. Nothing here corrupts anything but data the kernel owns
or the host's own upload."""
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
    from nanogpu.probe.selftest_valu import fold_valu

    mask = list(mask)
    r = P.cu_sweep_valu(0, mask, rounds, SEED, groups, inject, corrupt)
    records = list(r["records"])
    for more in (rounds * 2, rounds * 4):
        if fold_valu(records, r["groups"], cus)["cus_uncovered"] == 0:
            break
        records += list(P.cu_sweep_valu(0, mask, more, SEED, groups, inject, corrupt)["records"])
    r["records"] = records
    return r, fold_valu(records, r["groups"], cus)


@pytest.fixture(scope="module")
def clean(P):
    from nanogpu.probe.selftest_valu import GROUPS

    return _sweep_all(P, list(GROUPS))


def test_every_exact_group_is_the_twins_arithmetic(P):
    from nanogpu.probe import selftest_valu as V

    for g in V.EXACT_GROUPS:
        got = [int(w) for w in P.valu_lanes(g)]
        want = V.group_expected(g)[0]
        diff = [(i // 2, i % 2, hex(a), hex(b)) for i, (a, b) in enumerate(zip(got, want)) if a != b]
        assert not diff, (g, len(diff), diff[:4])


def test_approx_outputs_lie_in_the_twins_ranges(P):
    from nanogpu.probe import selftest_valu as V

    out = P.valu_lanes("approx")
    ranges = V.approx_ranges()
    worst = {}
    for i, op in enumerate(V.APPROX_OPS):
        d = [V.approx_ulp_distance(op, lane, out[i * 64 + lane]) for lane in range(64)]
        worst[op] = max(d)
        for lane in range(64):
            key = V.ordered_key(V.float_bits(out[i * 64 + lane]))
            assert ranges[(i * 64 + lane) * 2] <= key <= ranges[(i * 64 + lane) * 2 + 1], (op, lane, out[i * 64 + lane])
    print("approx max ulp", worst)
    record("selftest_valu_approx_max_ulp", worst)
    assert max(worst.values()) <= V.APPROX_ULPS


def test_clean_sweep_covers_every_cu(P, clean):
    r, f = clean
    print({k: r[k] for k in ("reg_slots", "regs_per_lane", "scratch_bytes", "ms")}, f["cus_seen"])
    assert f["cus_seen"] == 256 and f["cus_uncovered"] == 0 and f["failed"] == {}
    assert all(rec[2] == 0 and rec[4] == 0 and rec[5] == -1 and rec[6] == -1 for rec in r["records"])
    assert all(rec[3] == 0xF for rec in r["records"])
    assert len({rec[7] for rec in r["records"]}) == 1                      # one approx hash on the whole device
    assert r["scratch_bytes"] == 0 and r["reg_slots"] >= 448
    assert r["checked"] == list(r["groups"]) and len(r["groups"]) == 13
    record("selftest_valu_regs", {"reg_slots": r["reg_slots"], "regs_per_lane": r["regs_per_lane"],
                                  "scratch_bytes": r["scratch_bytes"]})


@pytest.mark.parametrize("kind,arg", [("valu", "fma32"), ("valu", "int64"), ("valu", "cvt"), ("valu", "xlane"),
                                      ("regs", 0), ("regs", 255), ("regs", 447), ("approx", None)])
def test_injection_fails_exactly_that_cu_and_kind(P, clean, kind, arg):
    from nanogpu.probe import selftest as S
    from nanogpu.probe import selftest_common as C
    from nanogpu.probe.selftest_valu import GROUPS

    rec = clean[0]["records"][len(clean[0]["records"]) // 3]
    cu = (rec[0], C.cu_key(rec[1]))
    inject = cu + ((kind, arg) if arg is not None else (kind,))
    r, f = _sweep_all(P, list(GROUPS), inject=inject)
    name = arg if kind == "valu" else kind
    assert f["failed"] == {name: [list(cu)]}, f["failed"]
    assert f["cus_seen"] == 256
    c = f["cus"][0]
    # wave 0, lane 0 was corrupted: an exact group or the registers fail on wave 0; after an approx flip it is
    # waves 1..3 whose hashes are unlike wave 0's (and the record's hash unlike the device's)
    assert c["waves"] == (0b1110 if kind == "approx" else 1)
    if kind == "regs":
        assert (c["bad_slot"], c["bad_wave"], c["bad_lane"]) == (arg, 0, 0)
    else:
        assert c["bad_slot"] == -1
    rep = S.DeepReport(device=0, ok=False, valu={"checked": list(GROUPS), "failed": f["failed"], "cus": f["cus"]})
    assert S.fenceable(rep) and S.failed_cus(rep) == {cu}
    if kind == "regs":
        assert f"slot {arg}" in rep.describe_failure()


def test_corrupt_expected_fails_every_wave_of_every_record(P):
    from nanogpu.probe.selftest_common import mix32
    from nanogpu.probe.selftest_valu import EXACT_GROUPS, GROUPS

    for i, g in enumerate(EXACT_GROUPS):
        word = mix32(i) % 128
        r = P.cu_sweep_valu(0, [], 1, SEED, list(GROUPS), None, (g, word, 1 << (mix32(word) & 31)))
        assert r["records"] and all(rec[2] == 0xF and rec[4] == 1 << i and rec[5] == -1 for rec in r["records"]), g


def test_every_word_of_every_table_can_fail_the_sweep(P):
    from nanogpu.probe.selftest_common import mix32
    from nanogpu.probe.selftest_valu import EXACT_GROUPS

    t0 = time.perf_counter()
    for i, g in enumerate(EXACT_GROUPS):
        r = P.valu_sensitivity(0, g, [(w, 1 << (mix32(w) & 31)) for w in range(128)])
        assert r["records"] >= 256 and len(r["words"]) == 128
        for w, (a, o) in enumerate(r["words"]):
            assert a[1] == 1 << i == o[1], (g, w, a, o)       # AND: the group's bit on every record; OR: no foreign bit
            assert a[0] == 0xF == o[0], (g, w, a, o)         # the word reaches the same lane of all four waves, and no other kind
    print(f"sensitivity: {128 * len(EXACT_GROUPS)} sweeps in {time.perf_counter() - t0:.2f} s")


def test_a_flipped_word_is_restored_before_the_next_flip(P):
    """Within one group a word left corrupted would hide behind the next one's failure. A zero XOR of
    the word flipped before is clean on every record: the XOR starts from the host's word each time, and
    the host's table was not written. A zero XOR of another word is clean only if the word flipped before
    was put back; the words around both must still fail."""
    def words(flips):
        return [tuple(tuple(half) for half in w) for w in P.valu_sensitivity(0, "fma32", flips)["words"]]

    fails, clean = ((0xF, 1), (0xF, 1)), ((0, 0), (0, 0))
    assert words([(5, 1 << 3), (5, 0), (6, 1 << 9)]) == [fails, clean, fails]
    assert words([(5, 1 << 3), (6, 0), (6, 1 << 9)]) == [fails, clean, fails]   # word 5 restored


def test_masked_to_one_unit(P):
    from nanogpu.agent import cumask
    from nanogpu.probe.selftest_valu import GROUPS

    mask = cumask.mask_words(list(range(5 * 8, 6 * 8)), 256)             # unit 5
    r, f = _sweep_all(P, list(GROUPS), mask=mask, cus=8)
    assert f["cus_seen"] == 8 and f["cus_uncovered"] == 0 and f["failed"] == {} and len(r["records"]) % 8 == 0
    assert sorted({rec[0] for rec in r["records"]}) == list(range(8))     # one CU per XCD
    ours = {(rec[0], (rec[1] >> 8) & 0xFF) for rec in r["records"]}
    # which CUs the unit is: what the census kernel reports from a stream with the same mask
    unit = {(xcc, (hw_id >> 8) & 0xFF) for xcc, hw_id in P.cu_census(0, mask, 512, 64)}
    assert len(unit) == 8 and ours == unit


def test_deep_selftest_with_valu_and_paths_and_the_metric(P):
    from nanogpu.agent.metrics import render
    from nanogpu.probe import selftest as S
    from nanogpu.topology.model import synthetic_mi355x

    rep = S.deep_selftest(P, 0, valu="all", paths="all")
    assert rep.ok, rep.describe_failure()
    assert len(rep.valu["checked"]) == 13 and rep.valu["failed"] == {} and rep.valu["reg_slots"] >= 448 and rep.valu["ms"] > 0
    assert len(rep.paths["checked"]) == 9 and rep.sweep["cus_seen"] == 256
    stats = {"reports": {0: rep.to_dict()}, "at": {0: time.time()}, "runs": {(0, "pass"): 1}}
    assert 'nanogpu_selftest_valu_checked{device="0"} 13' in render(synthetic_mi355x(1), None, None, "/nonexistent", stats)


def test_cost_of_the_valu_launch(P):
    """No threshold: the window in which a new grant could share CUs with the test is reported."""
    from nanogpu.probe.selftest_valu import GROUPS

    plain, valu = [], []
    for _ in range(11):                                   # interleaved pairs in one process
        plain.append(P.cu_sweep(0, [], 4, SEED)["ms"])
        valu.append(P.cu_sweep_valu(0, [], 4, SEED, list(GROUPS))["ms"])
    facts = {"sweep_ms": statistics.median(plain), "valu_ms": statistics.median(valu),
             "sweep_plus_valu_ms": statistics.median(a + b for a, b in zip(plain, valu)), "pairs": len(plain)}
    print("valu cost", facts)
    record("selftest_valu_cost", facts)
