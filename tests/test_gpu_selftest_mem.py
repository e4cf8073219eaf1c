"""Memory part of the deep self-test on a real MI355X: the kernel's instructions give what the twin
computes, a clean device passes on every CU, and every table word, every group's injected fault and
every mask is seen. Nothing here corrupts anything but data the kernel owns or the host's own upload."""
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
    from nanogpu.probe.selftest_mem import fold_mem

    mask = list(mask)
    r = P.cu_sweep_mem(0, mask, rounds, SEED, groups, inject, corrupt)
    records = list(r["records"])
    for more in (rounds * 2, rounds * 4):
        if fold_mem(records, r["groups"], cus)["cus_uncovered"] == 0:
            break
        records += list(P.cu_sweep_mem(0, mask, more, SEED, groups, inject, corrupt)["records"])
    r["records"] = records
    return r, fold_mem(records, r["groups"], cus)


@pytest.fixture(scope="module")
def clean(P):
    from nanogpu.probe.selftest_mem import GROUPS

    return _sweep_all(P, list(GROUPS))


def _groups():
    from nanogpu.probe.selftest_mem import GROUPS

    return list(GROUPS)


@pytest.mark.parametrize("group", ["gload", "l1", "gstore", "buffer", "lds", "ldstr", "ldsdma", "atomic"])
def test_every_lane_word_is_the_twins(P, group):
    from nanogpu.probe import selftest_mem as V

    got = [int(w) for w in P.mem_lanes(group)]
    want = V.group_lanes(group)
    K = V.GROUP_WORDS[group]
    assert len(got) == len(want) == 4 * K * 64
    diff = [(i // (K * 64), (i // 64) % K, i % 64, hex(a), hex(b)) for i, (a, b) in enumerate(zip(got, want)) if a != b]
    print(group, "differing (wave, k, lane, device, twin):", len(diff), diff[:8])
    assert not diff, (group, len(diff), diff[:4])


def test_clean_sweep_covers_every_cu(P, clean):
    r, f = clean
    print({k: r[k] for k in ("table_words", "slice_bytes", "num_regs", "scratch_bytes", "ms")}, f["cus_seen"])
    assert f["cus_seen"] == 256 and f["cus_uncovered"] == 0 and f["failed"] == {} and f["simds_seen_min"] == 4
    assert all(rec[2] == 0 and rec[4] == 0 and rec[5] == rec[6] == rec[7] == -1 for rec in r["records"])
    assert all(rec[3] == 0xF for rec in r["records"])
    assert r["scratch_bytes"] == 0 and r["table_words"] == 8192 and r["slice_bytes"] <= 8192
    assert r["checked"] == list(r["groups"]) == _groups() and len(r["groups"]) == 8


@pytest.mark.parametrize("group", ["gload", "l1", "gstore", "buffer", "lds", "ldstr", "ldsdma", "atomic"])
@pytest.mark.parametrize("end", ["first", "last"])
def test_injection_fails_exactly_that_cu_group_index_and_wave(P, clean, group, end):
    """The value the index is compared with is flipped on wave index % 4 of one CU; no held data is touched."""
    from nanogpu.probe import selftest as S
    from nanogpu.probe import selftest_common as C
    from nanogpu.probe import selftest_mem as V

    rec = clean[0]["records"][len(clean[0]["records"]) // 3]
    cu = (rec[0], C.cu_key(rec[1]))
    index = 0 if end == "first" else V.group_indices(group) - 1
    r, f = _sweep_all(P, _groups(), inject=cu + (group, index))
    assert f["failed"] == {group: [list(cu)]}, f["failed"]
    assert f["cus_seen"] == 256
    c = f["cus"][0]
    assert (c["bad_group"], c["bad_index"], c["bad_wave"], c["waves"]) == (group, index, index % 4, 1 << (index % 4))
    rep = S.DeepReport(device=0, ok=False, mem={"checked": _groups(), "failed": f["failed"], "cus": f["cus"]})
    assert S.fenceable(rep) and S.failed_cus(rep) == {cu}
    assert f"first in {group} at index {index}, wave {index % 4}" in rep.describe_failure()


def _twin_failure(group, word, mask):
    """(fail bits, lowest bad index, its wave) the twin gives for `group` with table word `word` XORed with `mask`."""
    from nanogpu.probe import selftest_mem as V

    K = V.GROUP_WORDS[group]
    good = list(V.group_lanes(group))
    t = V.table()
    held = t.load(4 * word, 4)
    t.store(4 * word, 4, held ^ mask)
    V._CACHE.pop(group)
    try:
        bad = list(V.group_lanes(group))
    finally:
        t.store(4 * word, 4, held)
        V._CACHE.pop(group)
    assert V.group_lanes(group) == good
    where = [(i // (K * 64), (i // 64) % K, i % 64) for i, (a, b) in enumerate(zip(good, bad)) if a != b]
    assert where, (group, word)
    if group == "l1":
        return sum(1 << w for w in {w for w, _k, _l in where}), word, min(w for w, _k, _l in where)
    index, wave = min((k * 64 + lane, w) for w, k, lane in where)
    return sum(1 << w for w in {w for w, _k, _l in where}), index, wave


def test_corrupt_expected_fails_every_record_at_that_word(P):
    from nanogpu.probe import selftest_mem as V

    groups = _groups()
    cases = [("l1", 4097, 1 << 30), ("gload", V.gload_chunk(0, 1, 5, 18) // 4, 1 << 7), ("gload", V.gload_chunk(1, 3, 63, 25) // 4 + 3, 1 << 31),
             ("ldsdma", V.dma_src(2, 7, 1) // 4 + 2, 1)]
    for group, word, mask in cases:
        fail, index, wave = _twin_failure(group, word, mask)
        r = P.cu_sweep_mem(0, [], 1, SEED, [group], None, (group, word, mask))
        g = groups.index(group)
        assert r["records"] and all(rec[2:] == (fail, 0xF, 1 << g, g, index, wave) for rec in r["records"]), (group, word, r["records"][0])
    # with every group selected the word fails in every group that reads it; the first one is reported
    r = P.cu_sweep_mem(0, [], 1, SEED, groups, None, ("l1", 4097, 1 << 30))
    assert r["records"] and all(rec[2] == 0xF and rec[4] >> 1 & 1 and rec[5] in (0, 1) for rec in r["records"])
    if all(rec[5] == 1 for rec in r["records"]):
        assert all(rec[6] == 4097 and rec[7] == 0 for rec in r["records"])
    for bad in (("gstore", 0, 1), ("l1", 8192, 1)):
        with pytest.raises(ValueError):
            P.cu_sweep_mem(0, [], 1, SEED, groups, None, bad)


def test_every_word_of_the_table_can_fail_the_sweep(P):
    """All 8,192 words, 1,024 a call, through `l1`, which every wave reads whole; the time is printed."""
    from nanogpu.probe.selftest_common import mix32

    t0 = time.perf_counter()
    for first in range(0, 8192, 1024):
        r = P.mem_sensitivity(0, "l1", [(w, 1 << (mix32(w) & 31)) for w in range(first, first + 1024)])
        assert r["records"] >= 256 and len(r["words"]) == 1024
        for k, (a, o) in enumerate(r["words"]):
            w = first + k
            assert tuple(a) == (0xF, 1 << 1, 1, w) == tuple(o), (w, a, o)   # every wave of every record, this group, this word
    print(f"table sensitivity: 8192 sweeps in {time.perf_counter() - t0:.2f} s")


def test_a_flipped_word_is_restored_before_the_next_flip(P):
    """A word left corrupted would hide behind the next one's failure. A zero XOR of the word flipped before is
    clean on every record: the XOR starts from the host's word each time, and the host's table was not written. A
    zero XOR of another word is clean only if the word flipped before was put back; the words around both must
    still fail."""
    def words(flips):
        return [tuple(tuple(half) for half in w) for w in P.mem_sensitivity(0, "l1", flips)["words"]]

    bad5, bad6, clean = ((0xF, 2, 1, 5),) * 2, ((0xF, 2, 1, 6),) * 2, ((0, 0, -1, -1),) * 2
    assert words([(5, 1 << 3), (5, 0), (6, 1 << 9)]) == [bad5, clean, bad6]
    assert words([(5, 1 << 3), (6, 0), (6, 1 << 9)]) == [bad5, clean, bad6]   # word 5 restored


def test_masked_to_one_unit(P):
    from nanogpu.agent import cumask

    mask = cumask.mask_words(list(range(5 * 8, 6 * 8)), 256)             # unit 5
    r, f = _sweep_all(P, _groups(), mask=mask, cus=8)
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

    rep = S.deep_selftest(P, 0, mem="all", scalar="all", valu="all", paths="all")
    assert rep.ok, rep.describe_failure()
    assert len(rep.mem["checked"]) == 8 and rep.mem["failed"] == {} and rep.mem["table_words"] == 8192 and rep.mem["ms"] > 0
    assert len(rep.scalar["checked"]) == 9 and len(rep.valu["checked"]) == 13 and len(rep.paths["checked"]) == 9
    assert rep.sweep["cus_seen"] == 256
    stats = {"reports": {0: rep.to_dict()}, "at": {0: time.time()}, "runs": {(0, "pass"): 1}}
    assert 'nanogpu_selftest_mem_checked{device="0"} 8' in render(synthetic_mi355x(1), None, None, "/nonexistent", stats)


def test_cost_of_the_mem_launch(P):
    """No threshold: the window in which a new grant could share CUs with the test is reported."""
    plain, mem, last = [], [], {}
    for _ in range(11):                                   # interleaved pairs in one process
        plain.append(P.cu_sweep(0, [], 4, SEED)["ms"])
        last = P.cu_sweep_mem(0, [], 4, SEED, _groups())
        mem.append(last["ms"])
    facts = {"sweep_ms": statistics.median(plain), "mem_ms": statistics.median(mem),
             "sweep_plus_mem_ms": statistics.median(a + b for a, b in zip(plain, mem)), "pairs": len(plain)}
    print("mem cost", facts)
    record("selftest_mem_cost", facts)
    record("selftest_mem_regs", {"num_regs": last["num_regs"], "scratch_bytes": last["scratch_bytes"], "slice_bytes": last["slice_bytes"]})
