"""XCD check of the deep self-test, without a GPU: the host header's stand-alone program against the Python twin,
hand-derived values, the bounds of every access, folding, deep_selftest over a fake probe, the agent's flag, where
the check runs, the unchanged outputs with the check off, and the metrics."""
import asyncio
import json
import subprocess
import sys
from pathlib import Path

import pytest

from nanogpu.agent.metrics import render as render_metrics
from nanogpu.agent.node import NodeAgent, build_parser
from nanogpu.k8s import podutil as pu
from nanogpu.k8s.fake_apiserver import FakeKubeStore, InProcKube
from nanogpu.probe import selftest as S
from nanogpu.probe import selftest_common as C
from nanogpu.probe import selftest_xcd as X
from nanogpu.topology.model import synthetic_mi355x

GIB = 1 << 30
M32 = 0xFFFFFFFF
ROOT = Path(__file__).resolve().parent.parent
SEED = 0x1234ABCD
NO_FIRST = (None,) * 6


def _hw(key):
    return key << 8


# ----------------------------------------------------------------------------- host program and twin
@pytest.mark.parametrize("kind", ["plain", "asan"])
def test_host_program_agrees_with_the_twin(kind):
    sys.path.insert(0, str(ROOT / "native"))
    import build  # native/build.py

    assert "xcd" in build.SELFTEST_HOST_TARGETS and f"xcd-{kind}" in build.SELFTEST_HOST_CHOICES
    exe = build.build_selftest_host(kind, target="xcd")
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr          # the program asserts the bounds and the header's conditions itself
    host = json.loads(r.stdout)
    assert host == X.twin_summary(host["seed"]) and host["seed"] == SEED
    assert host["dir_words"] == X.DIR_WORDS == 22272 and host["record_words"] == 36 and host["atom_words"] == 168


def test_spot_values_by_hand():
    assert X.hand_word(0, 0, 0) == C.mix32(0) == 0 and X.hand_word(SEED, 3, 17) == C.mix32(((3 << 12) | 17) ^ SEED)
    assert X.ticket_word(0, 0, 0, 0) == C.mix32(0x7E1C4E70) ^ 0x9E3779B1
    assert all(X.ticket_word(SEED, b, i, 0) ^ X.ticket_word(SEED, b, i, 1) == M32 for b in (0, 9, 1023) for i in (0, 511, 1023))
    # no two words of a slice, and no two slices' first words, are equal: an aliased address line shows
    assert len({X.hand_word(SEED, 5, i) for i in range(X.SLICE_WORDS)}) == X.SLICE_WORDS
    assert len({X.hand_word(SEED, b, 0) for b in range(X.MAX_BLOCKS)}) == X.MAX_BLOCKS
    one = X.atomic_expected(SEED, 1)
    assert one[X.ADD32] == X.atom_const(SEED, 0, 0) and one[X.ADD64] == X.atom_add64(SEED, 0) and one[X.XOR] == X.atom_const(SEED, 0, 3)
    assert one[X.COUNTER] == 4 and one[X.OR_MAP] == 1 and one[X.SEEN_MAP] == 0xF and sum(one[X.OR_MAP + 1:X.SEEN_MAP]) == 0
    three = X.atomic_expected(SEED, 3)
    lows = [X.atom_add64(SEED, b) & M32 for b in range(3)]
    assert all(v >> 31 for v in lows) and three[X.ADD64] >> 32 == sum(X.atom_add64(SEED, b) >> 32 for b in range(3)) + (sum(lows) >> 32)
    assert sum(lows) >> 32 >= 1                                                  # a carry crossed bit 32
    assert three[X.COUNTER] == 12 and three[X.OR_MAP] == 0b111 and three[X.SEEN_MAP] == 0xFFF
    assert three[X.UMAX] == max(X.atom_const(SEED, b, 4) for b in range(3)) and three[X.UMIN] == min(X.atom_const(SEED, b, 6) for b in range(3))
    signed = [X.atom_const(SEED, b, 5) for b in range(64)]
    assert any(v >> 31 for v in signed) and not all(v >> 31 for v in signed)     # signed and unsigned max differ somewhere
    full = X.atomic_expected(SEED, 1024)
    assert full[X.COUNTER] == 4096 and all(w == M32 for w in full[X.OR_MAP:]) and len(full) == X.ATOM_WORDS
    nine = X.atomic_expected(SEED, 9)
    assert nine[X.OR_MAP] == 0x1FF and nine[X.SEEN_MAP] == M32 and nine[X.SEEN_MAP + 1] == 0xF and nine[X.SEEN_MAP + 2] == 0
    assert X.atom_word_name(1) == "add64" and X.atom_word_name(8) == "or bitmap word 0" and X.atom_word_name(167) == "counter bitmap word 127"


@pytest.mark.parametrize("n", [1, 3, 8, 9, 256, 1024])
def test_bounds_of_every_access_a_legal_directory_can_produce(n):
    """The twin's layout: every region apart, every position, block and slice inside, for full and for empty XCDs."""
    regions = [X.COUNT_AT, X.READERS_AT, X.TICKET_AT, X.ATOM_AT, X.LIST_AT, X.WRITER_AT, X.MEMBER_AT, X.DIR_WORDS]
    assert regions == sorted(regions) and X.ATOM_AT + X.ATOM_WORDS * X.LINE_WORDS == X.LIST_AT
    assert X.TICKET_AT + X.ticket_groups(n) * X.LINE_WORDS <= X.ATOM_AT
    for placement in (lambda b: b % 8, lambda b: 5, lambda b: 5 if b % 2 else 2):
        counts = [sum(1 for b in range(n) if placement(b) == x) for x in range(8)]
        for q in (0, 1, n - 1):
            for x in range(8):
                pos = X.pick_position(n, counts[x], q)
                assert (pos is None) == (counts[x] == 0)
                if pos is not None:
                    assert 0 <= pos < counts[x] <= n and X.LIST_AT <= X.LIST_AT + x * X.MAX_BLOCKS + pos < X.WRITER_AT
    for bad in (n + 1, 1 << 31, M32):
        assert X.pick_position(n, bad, 0) is None
    assert (n - 1) * 4 * X.SLICE_WORDS + (3 * X.THREADS + X.THREADS - 1) * 16 + 16 == n * 4 * X.SLICE_WORDS
    assert sum(X.group_size(n, g) for g in range(X.ticket_groups(n))) == n and 1 <= X.group_size(n, X.ticket_groups(n) - 1) <= 8
    assert X.OR_MAP + (n - 1) // 32 < X.SEEN_MAP and X.SEEN_MAP + (4 * n - 1) // 32 < X.ATOM_WORDS


def test_parse_xcd():
    assert X.parse_xcd("all") == list(X.GROUPS) == ["handoff", "ticket", "atomic"] and X.parse_xcd("atomic, handoff") == ["handoff", "atomic"]
    assert X.parse_xcd(None) == X.parse_xcd("") == X.parse_xcd([]) == []
    with pytest.raises(ValueError, match=r"unknown XCD group\(s\) \['l2'\]: choose from handoff, ticket, atomic or 'all'"):
        X.parse_xcd("handoff,l2")


# ----------------------------------------------------------------------------- a simulated xcd_check
def _sim(n=16, groups=X.GROUPS, wplace=lambda b: b % 8, rplace=lambda b: (b + 3) % 8, bad_pairs=(), two_lasts=(), atomic_bad=(), seed=SEED):
    """What `xcd_check` returns for n workgroups placed by `wplace` (write and ticket kernels) and `rplace` (read
    kernel). `bad_pairs`: (writer xcc, reader xcc) whose word 17 reads wrong; `two_lasts`: ticket groups with two
    last arrivers; `atomic_bad`: indices of atomic words unlike the host's."""
    groups = [g for g in X.GROUPS if g in groups]
    lists = {x: [b for b in range(n) if wplace(b) == x] for x in range(8)}
    readers = {}
    records = []
    for b in range(n):
        write = (wplace(b), _hw(b // 8), 0, lists[wplace(b)].index(b))
        read = tick = atom = None
        if "handoff" in groups:
            y = rplace(b)
            q = readers[y] = readers.get(y, -1) + 1
            have = [x for x in range(8) if lists[x]]
            failed = [w for w in have if (w, y) in bad_pairs]
            first = NO_FIRST
            if failed:
                block = min(lists[w][q % len(lists[w])] for w in failed)
                first = (block, wplace(block), _hw(block // 8), 17, X.hand_word(seed, block, 17), X.hand_word(seed, block, 17) ^ 4)
            read = (y, _hw(32 + b // 8), 1 if failed else 0, sum(1 << w for w in have if w not in failed), sum(1 << w for w in failed), q) + first
        if "ticket" in groups:
            g, size = b // 8, X.group_size(n, b // 8)
            last = b % 8 == size - 1 or (g in two_lasts and b % 8 == 0)
            partners = [8 * g + j for j in range(size) if j != b % 8] if last else []
            tick = (wplace(b), _hw(b // 8), 0, int(last), b % 8, len(partners), sum({1 << wplace(p) for p in partners}), 0) + NO_FIRST + (0,)
        if "atomic" in groups:
            atom = (wplace(b), _hw(b // 8), 0, 0)
        records.append((write, read, tick, atom))
    want = X.atomic_expected(seed, n) if "atomic" in groups else []
    got = [w ^ (1 if i in atomic_bad else 0) for i, w in enumerate(want)]
    return {"records": records, "groups": list(X.GROUPS), "checked": groups, "atomic_words": got, "atomic_expected": want,
            "atomic_bad": sorted(atomic_bad) if "atomic" in groups else [], "pairs": {}, "blocks": n, "bytes": n * 20480 + 2 * 4 * X.DIR_WORDS,
            "num_regs": [16, 61, 29, 6], "scratch_bytes": 0, "ms_kernels": {"write": 0.02, "read": 0.06, "ticket": 0.05, "atomic": 0.05}, "ms": 0.2}


# ----------------------------------------------------------------------------- folding
def test_fold_a_clean_run():
    f = X.fold_xcd(_sim(64))
    assert f["ok"] and f["kinds"] == {} and f["failed"] == {"handoff": [], "ticket": [], "atomic": []} and f["first"] == {}
    assert f["pairs_seen"] == {"handoff": 64, "ticket": 7, "atomic": 0} and f["pairs_verified"] == 64 and f["pairs_uncovered"] == []
    assert f["ticket_groups_bad"] == [] and f["atomic_bad"] == [] and f["xcds"] == 8 and f["blocks"] == 64
    assert X.clauses(f) == [] and X.notes(f) == []
    f = X.fold_xcd(_sim(9, groups=["ticket"]))                           # groups of eight and of one
    assert f["ok"] and f["checked"] == ["ticket"] and f["ticket_groups_bad"] == [] and f["pairs_seen"] == {"ticket": 7}


def test_fold_exactly_one_failing_pair():
    f = X.fold_xcd(_sim(64, bad_pairs={(3, 5)}))
    assert not f["ok"] and f["failed"] == {"handoff": [[3, 5]], "ticket": [], "atomic": []} and f["kinds"] == {"handoff": ["data"]}
    first = f["first"]["handoff"]
    assert first["writer"] == [3, 0] and first["reader"][0] == 5 and (first["block"], first["word"]) == (3, 17)
    assert first["expected"] ^ first["observed"] == 4 and f["pairs_seen"]["handoff"] == 63 and f["pairs_uncovered"] == []
    assert X.clauses(f) == [f"XCD hand-off 3->5 wrong at word 17 of the slice of CU (xcc 3, key 0x0), read on CU (xcc 5, key {first['reader'][1]:#x})"]


def test_fold_one_writer_xcd_failing_towards_all_readers():
    f = X.fold_xcd(_sim(64, bad_pairs={(2, r) for r in range(8)}))
    assert f["failed"]["handoff"] == [[2, r] for r in range(8)] and f["pairs_seen"]["handoff"] == 56 and not f["ok"]
    assert X.clauses(f)[0].startswith("XCD hand-off 2->") and X.clauses(f)[0].endswith(", 8 pairs failed")


def test_fold_an_uncovered_pair_is_a_note_and_leaves_ok_true():
    # the read launch puts nothing on XCD 7, so no pair towards 7 is seen; writers 0..7 and readers 0..6 appear
    f = X.fold_xcd(_sim(64, rplace=lambda b: b % 7))
    assert f["ok"] and f["pairs_seen"]["handoff"] == 56 and f["pairs_uncovered"] == []     # XCD 7 is no reader in the records
    # a reader whose record shows fewer writer XCDs verified than wrote: that pair is uncovered
    res = _sim(64)
    recs = [list(r) for r in res["records"]]
    for r in recs:
        if r[1][0] == 5:
            r[1] = r[1][:3] + (r[1][3] & ~(1 << 3),) + r[1][4:]
    res["records"] = [tuple(r) for r in recs]
    f = X.fold_xcd(res)
    assert f["ok"] and f["pairs_uncovered"] == [[3, 5]] and f["pairs_seen"]["handoff"] == 63
    assert X.notes(f) == ["1 ordered pairs of XCDs not verified by the hand-off"]
    one = X.fold_xcd(_sim(8, wplace=lambda b: 2, rplace=lambda b: 2))
    assert one["ok"] and one["xcds"] == 1 and "nothing crosses XCDs" in X.notes(one)[0]


def test_fold_a_garbled_record():
    for where, section in ((1, (9, 0, 0, 0xFF, 0, 0) + NO_FIRST), (1, (1, 0, 0x20, 0xFF, 0, 0) + NO_FIRST), (1, (1, 0, 0, 0x1FF, 0, 0) + NO_FIRST),
                           (1, (1, 0, 1, 0xFE, 1, 0) + (5000, 0, 0, 17, 1, 2)), (2, (1, 0, 0, 2, 0, 0, 0, 0) + NO_FIRST + (0,)),
                           (3, (1, 0, 0x10, 0))):
        res = _sim(16)
        rec = list(res["records"][4])
        rec[where] = section
        res["records"][4] = tuple(rec)
        f = X.fold_xcd(res)
        group = X.GROUPS[where - 1]
        assert not f["ok"] and "record" in f["kinds"][group], (where, section, f["kinds"])


def test_fold_a_failing_write_kernel_fails_the_groups_that_read_what_it_left():
    for section, kind in (((3, 0, 2, None), "dir"), ((8, 0, 0, 0), "record"), ((3, 0, 1, 0), "record")):
        res = _sim(16)
        res["records"][5] = (section,) + res["records"][5][1:]
        f = X.fold_xcd(res)
        assert not f["ok"] and f["kinds"] == {"handoff": [kind], "ticket": [kind]}, (section, f["kinds"])
        res = _sim(16, groups=["atomic"])
        res["records"][5] = (section,) + res["records"][5][1:]
        assert X.fold_xcd(res)["ok"]


def test_fold_a_ticket_group_with_two_last_arrivers_or_none():
    f = X.fold_xcd(_sim(24, two_lasts={1}))
    assert not f["ok"] and f["ticket_groups_bad"] == [1] and f["kinds"] == {"ticket": ["last"]}
    assert X.clauses(f) == ["XCD ticket hand-off last in groups [1]"]
    res = _sim(24)
    res["records"][7] = res["records"][7][:2] + ((7, 0, 0, 0, 6, 0, 0, 0) + NO_FIRST + (0,),) + res["records"][7][3:]   # group 0 has none
    assert X.fold_xcd(res)["ticket_groups_bad"] == [0]


def test_fold_atomic_words():
    f = X.fold_xcd(_sim(16, atomic_bad={1, 40}))
    assert not f["ok"] and f["atomic_bad"] == [1, 40] and f["kinds"] == {"atomic": ["words"]} and f["failed"]["atomic"] == []
    assert X.clauses(f) == ["XCD atomics words wrong at add64 and 1 more"]
    res = _sim(16)
    res["records"][2] = res["records"][2][:3] + ((2, 0, 0x10, 3),)
    f = X.fold_xcd(res)
    assert f["kinds"] == {"atomic": ["dup"]} and X.clauses(f) == ["XCD atomics dup wrong"]


# ----------------------------------------------------------------------------- deep_selftest over a fake probe
class _FakeProbe:
    """256 CUs; `xcd[dev]` = keywords of `_sim` that make device dev's XCD check fail."""

    def __init__(self, n=2, xcd=None, cus=256):
        self.n, self.cus, self.xcd = n, cus, xcd or {}
        self.calls = []                  # ("sweep" | "mem" | "xcd" | "hbm", dev, mask, rounds[, names])

    def device_count(self):
        return self.n

    def device_props(self, dev):
        return {"cus": self.cus}

    def mem_info(self, dev):
        return 200 * GIB, 288 * GIB

    def _keys(self, mask):
        return [(i % 8, i // 8) for i in range(self.cus) if not mask or (mask[i // 32] >> (i % 32)) & 1]

    def cu_sweep(self, dev, mask, rounds, seed, inject=None):
        self.calls.append(("sweep", dev, list(mask), rounds))
        return {"records": [(x, _hw(k), 0, 0xF, -1) for x, k in self._keys(mask)], "lds_bytes": 163840, "ms": 0.25}

    def cu_sweep_mem(self, dev, mask, rounds, seed, groups, inject=None, corrupt_expected=None):
        self.calls.append(("mem", dev, list(mask), rounds, list(groups)))
        return {"records": [(x, _hw(k), 0, 0xF, 0, -1, -1, -1) for x, k in self._keys(mask)], "groups": list(groups),
                "checked": list(groups), "table_words": 8192, "slice_bytes": 8192, "num_regs": 128, "scratch_bytes": 0, "ms": 0.4}

    def xcd_check(self, dev, mask, rounds, seed, groups, inject=None, corrupt=None):
        self.calls.append(("xcd", dev, list(mask), rounds, list(groups)))
        keys = self._keys(mask)
        place = lambda b: keys[b % len(keys)][0]
        return _sim(rounds * len(keys), groups, wplace=place, rplace=place, seed=seed, **self.xcd.get(dev, {}))

    def hbm_pattern_check(self, dev, nbytes, seed, passes=2, corrupt=(), verify_seed=None, cu_mask=None):
        self.calls.append(("hbm", dev, list(cu_mask or []), passes))
        return {"bytes": nbytes, "errors": 0, "first": [], "fill_gbs": 5000.0, "verify_gbs": 6000.0}

    def kinds(self):
        return [c[0] for c in self.calls]


class _OldProbe(_FakeProbe):
    xcd_check = property()        # hasattr() is False


def test_the_check_runs_once_after_the_coverage_loop_before_hbm_on_the_sweeps_mask():
    P = _FakeProbe()
    rep = S.deep_selftest(P, 0, hbm_bytes=1 << 20, mem="l1", xcd="all", seed=1)
    assert rep.ok and P.kinds() == ["sweep", "mem", "xcd", "hbm"] and P.calls[2][2:] == ([], 4, list(X.GROUPS))
    assert rep.xcd["checked"] == list(X.GROUPS) and rep.xcd["pairs_verified"] == 64 and rep.xcd["ms"] == 0.2 and rep.xcd["bytes"] > 0
    assert rep.to_dict()["xcd"]["ms_kernels"]["read"] == 0.06 and rep.notes == []
    P = _FakeProbe()
    rep = S.deep_selftest(P, 0, cu_mask_bits=list(range(40, 48)), xcd="atomic,handoff", rounds=16, seed=1)
    assert P.kinds() == ["sweep", "xcd"] and P.calls[0][2] == P.calls[1][2] != [] and P.calls[1][3:] == (4, ["handoff", "atomic"])   # rounds capped
    assert rep.ok and rep.xcd["blocks"] == 32 and rep.xcd["pairs_seen"] == {"handoff": 64, "atomic": 0}

    class Shy(_FakeProbe):                 # the coverage loop runs three times; the check still runs once, after it
        def cu_sweep(self, dev, mask, rounds, seed, inject=None):
            out = super().cu_sweep(dev, mask, rounds, seed)
            if rounds < 16:
                out["records"] = out["records"][1:]
            return out

    P = Shy()
    assert S.deep_selftest(P, 0, xcd="ticket", seed=1).ok and P.kinds() == ["sweep", "sweep", "sweep", "xcd"]


def test_ok_fenceable_and_describe_failure():
    P = _FakeProbe(xcd={0: {"bad_pairs": {(3, 5)}}})
    rep = S.deep_selftest(P, 0, xcd="all", seed=1)
    assert not rep.ok and not S.fenceable(rep) and S.failed_cus(rep) == set() and rep.sweep["failed"] == []
    assert rep.xcd["failed"]["handoff"] == [[3, 5]]
    text = rep.describe_failure()
    assert text.startswith("XCD hand-off 3->5 wrong at word 17 of the slice of CU (xcc 3, key 0x") and ", read on CU (xcc 5, key 0x" in text
    assert S.deep_selftest(P, 1, xcd="all", seed=1).ok and S.deep_selftest(P, 0, xcd="ticket,atomic", seed=1).ok
    assert S.would_fence(P, 0, rep, 4)["units"] == [] and "not a CU's to fence" in S.would_fence(P, 0, rep, 4)["reason"]
    rep = S.deep_selftest(_FakeProbe(xcd={0: {"atomic_bad": {7}}}), 0, xcd="all", seed=1)
    assert not rep.ok and rep.describe_failure() == "XCD atomics words wrong at counter"
    rep = S.deep_selftest(_FakeProbe(xcd={0: {"two_lasts": {0}}}), 0, xcd="all", seed=1)
    assert not rep.ok and not S.fenceable(rep) and "XCD ticket hand-off last in groups [0]" in rep.describe_failure()
    # localise_failure's unit sweeps do not carry the check: it is no part of the selection
    P = _FakeProbe()
    S.localise_failure(P, 0, S.DeepReport(device=0), range(2), 8)
    assert "xcd" not in P.kinds()
    with pytest.raises(TypeError):
        S.Selection.parse(xcd="all")


def test_notes_for_an_older_probe_a_single_xcd_and_uncovered_pairs():
    P = _OldProbe()
    assert not hasattr(P, "xcd_check")
    rep = S.deep_selftest(P, 0, xcd="all", seed=1)
    assert rep.ok and rep.xcd is None and "xcd" not in rep.to_dict() and rep.notes == [X.NOTE_MISSING]
    rep = S.deep_selftest(_FakeProbe(), 0, cu_mask_bits=[40, 48, 56], xcd="all", seed=1)       # three CUs of XCD 0
    assert rep.ok and rep.xcd["xcds"] == 1 and any("nothing crosses XCDs" in n for n in rep.notes)


def test_with_the_check_off_every_output_is_what_it_was(monkeypatch, capsys):
    """Compared with the same calls made before `xcd=` is passed, not with a copied constant."""
    def strip(d):
        return {k: v for k, v in d.items() if k != "seconds"}

    before = S.deep_selftest(_FakeProbe(), 0, hbm_bytes=1 << 20, mem="all", seed=1)
    for off in (None, "", []):
        P = _FakeProbe()
        rep = S.deep_selftest(P, 0, hbm_bytes=1 << 20, mem="all", seed=1, xcd=off)
        assert strip(rep.to_dict()) == strip(before.to_dict()) and "xcd" not in rep.to_dict() and "xcd" not in P.kinds()
        assert rep.xcd is None and repr(rep).replace(repr(rep.seconds), "") == repr(before).replace(repr(before.seconds), "")
    on = S.deep_selftest(_FakeProbe(), 0, hbm_bytes=1 << 20, mem="all", seed=1, xcd="all").to_dict()
    assert strip({k: v for k, v in on.items() if k != "xcd"}) == strip(before.to_dict())
    # both help texts: the parsers with the two flags taken out again
    monkeypatch.setenv("COLUMNS", "100")
    with pytest.raises(SystemExit):
        S.main(["--help"])
    help_cmd = capsys.readouterr().out
    agent_parser = build_parser()
    help_agent = agent_parser.format_help()
    assert "xcd" not in help_cmd and "xcd" not in help_agent
    hidden = [a for a in agent_parser._actions if "--selftest-xcd" in a.option_strings]
    assert len(hidden) == 1
    agent_parser._remove_action(hidden[0])
    assert agent_parser.format_help() == help_agent
    # the command's printed report
    from nanogpu import native

    monkeypatch.setattr(native, "probe", lambda required=False: _FakeProbe())
    monkeypatch.setattr(S.time, "perf_counter", lambda: 0.0)
    assert S.main(["--hbm-mib", "64", "--mem", "all"]) == 0
    plain = capsys.readouterr().out
    assert S.main(["--hbm-mib", "64", "--mem", "all", "--xcd", ""]) == 0
    assert capsys.readouterr().out == plain
    assert S.main(["--hbm-mib", "64", "--mem", "all", "--xcd", "all"]) == 0
    with_check = capsys.readouterr().out.splitlines()
    line = "  XCD check handoff, ticket, atomic: 64 ordered pair(s) of XCDs verified, 0.200 ms: all clean"
    assert line in with_check and [x for x in with_check if x != line] == plain.splitlines()
    assert S.main(["--hbm-mib", "64", "--xcd", "atomic", "--json"]) == 0
    assert json.loads(capsys.readouterr().out)["xcd"]["checked"] == ["atomic"]
    with pytest.raises(SystemExit) as e:
        S.main(["--xcd", "handoff,nope"])
    assert e.value.code == 2 and "unknown XCD group(s) ['nope']" in capsys.readouterr().err


# ----------------------------------------------------------------------------- agent
def _agent(n=2, **kw):
    store = FakeKubeStore()
    topo = synthetic_mi355x(n)
    store.add_node(pu.make_node("n0", n, topo.to_json()))
    return NodeAgent(InProcKube(store), "n0", topo, device_plugin=False, health_period_s=0, **kw), store


def test_the_agents_flag_parses_and_implies_deep(capsys):
    ap = build_parser()
    a = ap.parse_args(["--node-name", "n", "--selftest-xcd", "atomic,handoff"])
    assert a.selftest and a.selftest_deep and a.selftest_xcd == ["handoff", "atomic"]
    assert ap.parse_args(["--selftest-xcd", "all"]).selftest_xcd == list(X.GROUPS)
    d = ap.parse_args(["--node-name", "n", "--selftest-deep"])
    assert d.selftest_xcd == [] and not ap.parse_args(["--node-name", "n"]).selftest_deep
    for bad, wording in (("handoff,l2", "--selftest-xcd: unknown XCD group(s) ['l2']: choose from handoff, ticket, atomic or 'all'"),
                         ("", "--selftest-xcd: name at least one group, or 'all'")):
        with pytest.raises(SystemExit) as e:
            ap.parse_args(["--selftest-xcd", bad])
        assert e.value.code == 2 and wording in " ".join(capsys.readouterr().err.split())
    agent = NodeAgent(None, "n", synthetic_mi355x(1), device_plugin=False, selftest_xcd="ticket")
    assert agent.selftest_deep and agent.selftest_xcd == ["ticket"]
    plain = NodeAgent(None, "n", synthetic_mi355x(1), device_plugin=False)
    assert plain.selftest_xcd == [] and not plain.selftest_deep


def test_a_granted_device_gets_the_check_and_no_hbm_check():
    from nanogpu.agent.plugin import NanoGpuPlugin

    async def main():
        store = FakeKubeStore()
        topo = synthetic_mi355x(2)
        store.add_node(pu.make_node("n0", 2, topo.to_json()))
        api = InProcKube(store)
        agent = NodeAgent(api, "n0", topo, device_plugin=False, health_period_s=0, selftest_hbm_mib=64, selftest_xcd="all")
        agent.plugin = NanoGpuPlugin(topo, api, "n0")
        dc = agent.plugin.cus[0]
        dc.used[("pod", "c")] = [0, 1, 2, 3]                      # a tenant holds four units of device 0
        bits, hbm = agent.deep_plan(0)
        assert not hbm and len(bits) == 256 - 32
        P = _FakeProbe(2)
        assert await agent.selftest(P) == []
        by_dev = {d: [c for c in P.calls if c[1] == d] for d in (0, 1)}
        assert [c[0] for c in by_dev[0]] == ["sweep", "xcd"] and [c[0] for c in by_dev[1]] == ["sweep", "xcd", "hbm"]
        assert by_dev[0][1][2] == by_dev[0][0][2] != [] and by_dev[1][1][2] == []          # the free units' mask; the whole idle device
        assert agent.selftest_stats["reports"][0]["xcd"]["ok"] and agent.selftest_stats["reports"][0]["hbm"] is None

    asyncio.run(main())


def test_the_fence_modes_call_order():
    from nanogpu.agent.plugin import NanoGpuPlugin

    async def run(P, **kw):
        store = FakeKubeStore()
        topo = synthetic_mi355x(1)
        store.add_node(pu.make_node("n0", 1, topo.to_json()))
        api = InProcKube(store)
        agent = NodeAgent(api, "n0", topo, device_plugin=False, health_period_s=0, selftest_fence=1, selftest_xcd="all", **kw)
        agent.plugin = NanoGpuPlugin(topo, api, "n0")
        failed = await agent.selftest(P)
        return agent, failed

    async def main():
        # a clean chip: the sweep alone, then the run that judges memory, with the check before the HBM check
        P = _FakeProbe(1)
        agent, failed = await run(P, selftest_hbm_mib=64)
        assert failed == [] and P.kinds() == ["sweep", "sweep", "xcd", "hbm"]
        # a chip whose check fails is not fenced: the failure names no CU
        P = _FakeProbe(1, xcd={0: {"bad_pairs": {(1, 2)}}})
        agent, failed = await run(P, selftest_hbm_mib=64)
        assert failed == [0] and P.kinds() == ["sweep", "sweep", "xcd", "hbm"] and agent.topo.devices[0].fenced == []
        assert not agent.topo.devices[0].healthy
        # a chip with a failing CU is judged on its CUs first: first sweep, 32 units alone, then the verification with the check
        class BadCu(_FakeProbe):
            def cu_sweep(self, dev, mask, rounds, seed, inject=None):
                out = super().cu_sweep(dev, mask, rounds, seed)
                out["records"] = [(x, h, 1 if (x, h >> 8) == (3, 17) else 0, s, b) for x, h, _f, s, b in out["records"]]
                return out

        P = BadCu(1)
        agent, failed = await run(P, selftest_hbm_mib=64)
        assert failed == [] and agent.topo.devices[0].fenced == [17]
        assert P.kinds() == ["sweep"] * 34 + ["xcd", "hbm"] and P.calls[-2][2] == P.calls[-3][2] != []

    asyncio.run(main())


def test_the_metrics_lines():
    async def main():
        agent, _ = _agent(2, selftest_xcd="all", selftest_hbm_mib=64)
        await agent.start()
        P = _FakeProbe(2, xcd={1: {"bad_pairs": {(2, r) for r in range(8)}}})
        assert await agent.selftest(P) == [1]
        assert [d.healthy for d in agent.topo.devices] == [True, False]
        lines = render_metrics(agent.topo, None, None, "/nonexistent", agent.selftest_stats).splitlines()
        for line in ('nanogpu_selftest_xcd_checked{device="0"} 3', 'nanogpu_selftest_xcd_checked{device="1"} 3',
                     'nanogpu_selftest_xcd_failed_pairs{device="0",group="handoff"} 0', 'nanogpu_selftest_xcd_failed_pairs{device="1",group="handoff"} 8',
                     'nanogpu_selftest_xcd_failed_pairs{device="1",group="ticket"} 0', 'nanogpu_selftest_xcd_failed_pairs{device="1",group="atomic"} 0',
                     'nanogpu_selftest_xcd_pairs_verified{device="0"} 64', 'nanogpu_selftest_xcd_pairs_verified{device="1"} 57',   # 56 by hand-off, and 2->7 through a ticket
                    
                     "# TYPE nanogpu_selftest_xcd_failed_pairs gauge"):
            assert line in lines, line
        plain, _ = _agent(2, selftest_deep=True)
        await plain.start()
        Q = _FakeProbe(2, xcd={1: {"bad_pairs": {(2, 3)}}})
        assert await plain.selftest(Q) == [] and "xcd" not in Q.kinds()                     # without the flag the check does not run
        assert "xcd" not in plain.selftest_stats["reports"][0]
        assert "nanogpu_selftest_xcd" not in render_metrics(plain.topo, None, None, "/nonexistent", plain.selftest_stats)
        for a in (agent, plain):
            await a.stop()

    asyncio.run(main())


def test_the_documents_name_the_flags_and_the_metrics():
    text = (ROOT / "docs" / "REFERENCE.md").read_text()
    for name in ("--selftest-xcd", "--xcd all|LIST", "nanogpu_selftest_xcd_checked", "nanogpu_selftest_xcd_failed_pairs", "nanogpu_selftest_xcd_pairs_verified"):
        assert name in text, name
    readme = (ROOT / "README.md").read_text()
    for name in ("--selftest-xcd", "selftest_xcd_host.h", "probe_xcd.inc", "selftest_xcd.py"):
        assert name in readme, name
