"""XCD check of the deep self-test on a real MI355X: what one XCD wrote is read on every other, by a hand-off
across a kernel boundary, by release, ticket and acquire inside one kernel, and by memory-side atomics; every
hook fails exactly what it names. Nothing here touches anything but memory the check allocated itself."""
import statistics
import time

import pytest

pytestmark = pytest.mark.gpu

SEED = 0x1234ABCD
ALL_PAIRS = {(w, r) for w in range(8) for r in range(8)}


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


def _mask(bits):
    from nanogpu.agent import cumask

    return cumask.mask_words(list(bits), 256)


UNIT = range(40, 48)      # one CU-mask unit: 8 CUs, one per XCD
THREE = range(40, 43)     # three CUs on three XCDs


def _run(P, mask=(), rounds=4, groups=("handoff", "ticket", "atomic"), inject=None, corrupt=None):
    from nanogpu.probe.selftest_xcd import fold_xcd

    r = P.xcd_check(0, list(mask), rounds, SEED, list(groups), inject, corrupt)
    return r, fold_xcd(r)


@pytest.fixture(scope="module")
def whole(P):
    return _run(P)


@pytest.fixture(scope="module")
def unit(P):
    return _run(P, _mask(UNIT), 1)


def _pairs(r, group):
    return {tuple(p) for p in r["pairs"][group]}


def _lasts(r):
    """{ticket group: [ticket sections of its last arrivers]}"""
    out = {}
    for b, rec in enumerate(r["records"]):
        if rec[2][3]:
            out.setdefault(b // 8, []).append(rec[2])
    return out


def _assert_clean(r, f, n):
    from nanogpu.probe import selftest_xcd as X

    assert r["blocks"] == n == len(r["records"]) and r["scratch_bytes"] == 0
    assert f["ok"] and f["kinds"] == {} and f["failed"] == {"handoff": [], "ticket": [], "atomic": []}, (f["kinds"], f["failed"], f["first"])
    assert [int(w) for w in r["atomic_words"]] == X.atomic_expected(SEED, n) == [int(w) for w in r["atomic_expected"]]
    assert list(r["atomic_bad"]) == [] and int(r["atomic_words"][X.COUNTER]) == 4 * n
    lasts = _lasts(r)
    for g in range(X.ticket_groups(n)):                      # one last arriver a group, and it verified all the others
        assert len(lasts.get(g, [])) == 1, (g, lasts.get(g))
        assert lasts[g][0][5] == X.group_size(n, g) - 1 and lasts[g][0][4] == X.group_size(n, g) - 1
    assert f["ticket_groups_bad"] == []
    for rec in r["records"]:
        assert rec[0][2] == 0 and rec[1][2] == 0 and rec[2][2] == 0 and rec[3][2:] == (0, 0)
        assert rec[1][6:] == (None,) * 6 and rec[2][8:14] == (None,) * 6
        assert rec[2][14] in (0, 0xFFFFFFFF)                  # the fold of the words read before the ticket: each before or after


def test_whole_device_is_clean_and_every_ordered_pair_is_verified(whole):
    r, f = whole
    print({k: r[k] for k in ("blocks", "bytes", "num_regs", "scratch_bytes", "ms", "ms_kernels")})
    print("pairs seen", f["pairs_seen"], "uncovered", f["pairs_uncovered"])
    _assert_clean(r, f, 1024)
    assert _pairs(r, "handoff") == ALL_PAIRS and f["pairs_seen"]["handoff"] == 64 and f["pairs_uncovered"] == [] and f["xcds"] == 8


def test_one_unit_verifies_all_56_foreign_pairs(unit):
    r, f = unit
    print("unit placement: writers", [rec[0][0] for rec in r["records"]], "readers", [rec[1][0] for rec in r["records"]])
    _assert_clean(r, f, 8)
    assert {p for p in _pairs(r, "handoff") if p[0] != p[1]} == {p for p in ALL_PAIRS if p[0] != p[1]}
    assert f["pairs_uncovered"] == [] and f["xcds"] == 8


def test_three_cus_one_ticket_group_of_three(P):
    r, f = _run(P, _mask(THREE), 1)
    _assert_clean(r, f, 3)
    xs = {rec[0][0] for rec in r["records"]}
    assert len(xs) == 3 and f["xcds"] == 3
    assert _pairs(r, "handoff") == {(w, rd) for w in xs for rd in xs}
    last = _lasts(r)[0][0]
    assert last[5] == 2 and last[6] and not last[6] & ~sum(1 << x for x in xs)      # both partners verified, on XCDs of the mask


def test_nine_workgroups_ticket_groups_of_eight_and_of_one(P):
    r, f = _run(P, _mask(THREE), 3)
    _assert_clean(r, f, 9)
    lasts = _lasts(r)
    assert lasts[1][0][5] == 0 and lasts[1][0][4] == 0 and r["records"][8][2][3] == 1     # alone: last at once, nothing to verify
    assert lasts[0][0][5] == 7


def test_inject_handoff_fails_exactly_that_pair(P):
    from nanogpu.probe import selftest_xcd as X

    r, f = _run(P, inject=("handoff", 3, 5))
    assert f["failed"] == {"handoff": [[3, 5]], "ticket": [], "atomic": []} and f["kinds"] == {"handoff": ["data"]}
    first = f["first"]["handoff"]
    assert first["word"] == 0 and first["writer"][0] == 3 and first["reader"][0] == 5 and first["expected"] ^ first["observed"] == 1
    assert first["observed"] == X.hand_word(SEED, first["block"], 0)
    readers5 = [rec[1] for rec in r["records"] if rec[1][0] == 5]
    assert readers5 and all(rd[2] == 1 and rd[4] == 1 << 3 and rd[9] == 0 for rd in readers5)      # every reader on XCD 5, word 0
    assert all(rec[1][2] == 0 for rec in r["records"] if rec[1][0] != 5)
    assert _pairs(r, "handoff") == ALL_PAIRS - {(3, 5)} and list(r["atomic_bad"]) == []


def test_inject_ticket_fails_exactly_that_groups_last_arriver(P):
    from nanogpu.probe import selftest_xcd as X

    r, f = _run(P, inject=("ticket", 17))
    assert f["kinds"] == {"ticket": ["data"]} and f["failed"]["handoff"] == [] and f["failed"]["atomic"] == [] and len(f["failed"]["ticket"]) == 1
    bad = [(b, rec[2]) for b, rec in enumerate(r["records"]) if rec[2][2]]
    assert len(bad) == 1 and bad[0][0] // 8 == 17 and bad[0][1][3] == 1 and bad[0][1][5] == 6     # the last arriver; six of seven verified
    b, sec = bad[0]
    partner = 17 * 8 + (1 if b % 8 == 0 else 0)
    assert sec[8] == partner and sec[11] == 0 and sec[12] ^ sec[13] == 1 and sec[13] == X.ticket_word(SEED, partner, 0, 1)
    assert sec[9] == r["records"][partner][2][0] and sec[10] == r["records"][partner][2][1]            # the writer's CU
    assert f["failed"]["ticket"] == [[sec[9], sec[0]]]


@pytest.mark.parametrize("word", [0, 1, 7, 8, 167])
def test_inject_atomic_fails_exactly_that_word(P, word):
    r, f = _run(P, _mask(UNIT), 1, inject=("atomic", word))
    assert list(r["atomic_bad"]) == [word] and f["kinds"] == {"atomic": ["words"]} and not f["ok"]
    assert f["failed"] == {"handoff": [], "ticket": [], "atomic": []}
    assert int(r["atomic_expected"][word]) ^ int(r["atomic_words"][word]) == 1


def test_corrupt_byte_is_reported_by_every_reader_with_writer_cu_and_word(P):
    from nanogpu.probe import selftest_xcd as X

    word, byte, xor = 1234, 2, 0x40
    r, f = _run(P, _mask(UNIT), 1, corrupt=(3, 4 * word + byte, xor))
    wx, whw = r["records"][3][0][0], r["records"][3][0][1]
    want = X.hand_word(SEED, 3, word)
    counts = {}
    for rec in r["records"]:
        counts[rec[0][0]] = counts.get(rec[0][0], 0) + 1
    readers = [rec[1] for rec in r["records"]]
    hit = [rd for rd in readers if rd[2]]
    assert hit and all(rd[2] == 1 and rd[4] == 1 << wx and rd[6:] == (3, wx, whw, word, want, want ^ xor << 16) for rd in hit)
    if counts[wx] == 1:                                       # block 3 is its XCD's only slice: every reader reads it
        assert len(hit) == 8
    assert f["kinds"] == {"handoff": ["data"]} and f["failed"]["handoff"] == [list(p) for p in sorted({(wx, rd[0]) for rd in hit})]
    assert f["first"]["handoff"]["writer"] == [wx, (whw >> 8) & 0xFF] and f["first"]["handoff"]["word"] == word
    assert list(r["atomic_bad"]) == [] and f["failed"]["ticket"] == []
    for bad in ((8, 0, 1), (0, 16384, 1), (0, 0, 256)):
        with pytest.raises(ValueError):
            P.xcd_check(0, _mask(UNIT), 1, SEED, ["handoff"], None, bad)


def test_every_word_of_a_slice_can_fail_the_handoff(P):
    """All 4,096 words of block 0's slice on the one-unit shape, one run a word on one session; the time is printed."""
    from nanogpu.probe.selftest_common import mix32

    t0 = time.perf_counter()
    r = P.xcd_sensitivity(0, [(w, 1 << (mix32(w) & 31)) for w in range(4096)], _mask(UNIT), 1, SEED)
    print(f"slice sensitivity: 4096 runs in {time.perf_counter() - t0:.2f} s ({r['seconds']:.2f} s in the loop)")
    assert r["records"] == 8 and len(r["words"]) == 4096
    whole_and = 0
    for w, (a, o) in enumerate(r["words"]):
        # some reader failed at exactly this word of block 0, with one writer XCD, and no reader saw anything else
        assert o[0] == 1 and o[1] in [1 << k for k in range(8)] and (o[2], o[3]) == (0, w), (w, a, o)
        whole_and += tuple(a) == tuple(o)
    print("runs in which every one of the 8 readers read block 0:", whole_and)
    assert whole_and > 0


def test_a_flipped_word_is_restored_before_the_next_flip(P):
    def words(flips):
        return [tuple(o) for _a, o in P.xcd_sensitivity(0, flips, _mask(UNIT), 1, SEED)["words"]]

    for flips in ([(5, 1 << 3), (5, 0), (6, 1 << 9)], [(5, 1 << 3), (6, 0), (6, 1 << 9)]):
        got = words(flips)
        assert got[0][0] == 1 and got[0][2:] == (0, 5) and got[2][0] == 1 and got[2][2:] == (0, 6)
        assert got[1] == (0, 0, -1, -1)                       # a zero XOR is clean: the flip before it did not stay


def test_deep_selftest_with_the_xcd_check_and_the_metric(P):
    from nanogpu.agent.metrics import render
    from nanogpu.probe import selftest as S
    from nanogpu.topology.model import synthetic_mi355x

    rep = S.deep_selftest(P, 0, xcd="all", mem="all")
    assert rep.ok, rep.describe_failure()
    assert rep.xcd["checked"] == ["handoff", "ticket", "atomic"] and rep.xcd["ok"] and rep.xcd["pairs_seen"]["handoff"] == 64
    assert rep.xcd["pairs_verified"] == 64 and rep.xcd["ms"] > 0 and len(rep.mem["checked"]) == 8
    stats = {"reports": {0: rep.to_dict()}, "at": {0: time.time()}, "runs": {(0, "pass"): 1}}
    text = render(synthetic_mi355x(1), None, None, "/nonexistent", stats)
    assert 'nanogpu_selftest_xcd_checked{device="0"} 3' in text and 'nanogpu_selftest_xcd_pairs_verified{device="0"} 64' in text
    assert 'nanogpu_selftest_xcd_failed_pairs{device="0",group="ticket"} 0' in text


def test_ticket_last_arrivers_read_foreign_xcds_and_the_cost(P, whole):
    """On the idle whole device the last arrivers of the 128 ticket groups sit where dispatch put them. The exact
    conditions (one last arriver a group, every partner verified) are test_whole_device's; here the placement is
    recorded, and that every XCD was the writer of a foreign pair verified through a ticket. The cost has no
    threshold: it is the window in which a new grant could share CUs with the check."""
    r, f = whole
    foreign = {p for p in _pairs(r, "ticket") if p[0] != p[1]}
    last_xccs = [sec[0] for secs in _lasts(r).values() for sec in secs]
    placement = {"ticket_pairs": len(_pairs(r, "ticket")), "ticket_foreign_pairs": len(foreign),
                 "foreign_writers": sorted({w for w, _r in foreign}), "last_arrivers_per_xcd": [last_xccs.count(x) for x in range(8)],
                 "group_xcds_min": min(len({r["records"][b][2][0] for b in range(8 * g, 8 * g + 8)}) for g in range(128))}
    print("ticket placement", placement)
    record("selftest_xcd_ticket_placement", placement)
    plain, xcd, last = [], [], {}
    for _ in range(11):                                   # interleaved pairs in one process
        plain.append(P.cu_sweep(0, [], 4, SEED)["ms"])
        last = P.xcd_check(0, [], 4, SEED)
        xcd.append(last)
    facts = {"sweep_ms": statistics.median(plain), "xcd_ms": statistics.median(x["ms"] for x in xcd),
             "sweep_plus_xcd_ms": statistics.median(a + x["ms"] for a, x in zip(plain, xcd)), "pairs": len(plain),
             **{f"{k}_ms": statistics.median(x["ms_kernels"][k] for x in xcd) for k in ("write", "read", "ticket", "atomic")}}
    print("xcd cost", facts)
    record("selftest_xcd_cost", facts)
    record("selftest_xcd_regs", {"num_regs": list(last["num_regs"]), "scratch_bytes": last["scratch_bytes"], "bytes": last["bytes"]})
    assert placement["foreign_writers"] == list(range(8))
