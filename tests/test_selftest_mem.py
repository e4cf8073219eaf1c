"""Memory part of the deep self-test, without a GPU: the host header's stand-alone program against
the Python twin, the twin's own conditions and hand-derived values, parsing, folding,
deep_selftest over a fake probe, fencing, the hidden flags, the unchanged help texts and the metric."""
import asyncio
import dataclasses
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
from nanogpu.probe import selftest_mem as V
from nanogpu.topology.model import synthetic_mi355x

GIB = 1 << 30
M32 = 0xFFFFFFFF
ROOT = Path(__file__).resolve().parent.parent
ALL = [(x, k) for x in range(8) for k in range(32)]


def _hw(key, simd=0):
    return (key << 8) | (simd << 4)


def _rec(x, k, fail=0, gbits=0, group=-1, index=-1, wave=-1):
    return (x, _hw(k), fail, 0xF, gbits, group, index, wave)


def _bad(x, k, group, index, wave):
    g = V.GROUPS.index(group)
    return _rec(x, k, fail=1 << wave, gbits=1 << g, group=g, index=index, wave=wave)


def _clean(keys=ALL):
    return [_rec(x, k) for x, k in keys]


# ----------------------------------------------------------------------------- host program and twin
@pytest.mark.parametrize("kind", ["plain", "asan"])
def test_host_program_agrees_with_the_twin(kind):
    sys.path.insert(0, str(ROOT / "native"))
    import build  # native/build.py

    exe = build.build_selftest_host(kind, target="mem")
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr          # the program asserts the header's conditions itself, bounds included
    host = json.loads(r.stdout)
    twin = V.twin_summary()
    assert list(host["groups"]) == list(V.GROUPS)
    for g in V.GROUPS:
        assert host["groups"][g] == twin["groups"][g], g         # [words a lane, checksum over [wave][k][lane]]
    assert host["table_checksum"] == twin["table_checksum"] and host["table_words"] == V.MEM_WORDS == 8192
    assert host["slice_bytes"] == V.SLICE_BYTES <= 8192 and host["record_words"] == V.RECORD_WORDS == 8


def test_twin_conditions_hold():
    for g in V.GROUPS:
        words = V.group_lanes(g)
        assert len(words) == 4 * 64 * V.GROUP_WORDS[g] and V.uncovered_bits(words) == 0, g   # no bit position is constant
    t = [V.table_word(i) for i in range(V.MEM_WORDS)]
    assert all(t[i] != t[i ^ (1 << b)] for i in range(V.MEM_WORDS) for b in range(13))       # every address line matters
    # store maps are injective, and the upper chunks of the st64 forms meet no lower one
    for wave in range(4):
        for f in range(7):
            assert len({V.gstore_chunk(wave, lane, f) for lane in range(64)}) == 64
            assert all(V.gstore_sub(lane, f) + V.GSTORE_BYTES[f] <= 16 for lane in range(64))
    for m in range(3):
        chunks = {V.lds_chunk(m, lane) for lane in range(64)}
        assert len(chunks) == 64 and max(chunks) + 16 <= V.LDS_UPPER and 2 * V.LDS_UPPER <= V.LDS_WAVE_BYTES
    assert {(V.lds_chunk(2, lane) // 4) % 32 for lane in range(32)} == {0}                    # a half-wave on one bank
    for f in range(26):                                                                       # map 1: a 128-byte line a lane
        assert len({V.gload_chunk(1, 2, lane, f) // 128 for lane in range(64)}) == 64
    # every byte offset and both signs in the sub-dword loads
    assert {f[2] for f in V.GLOAD_FORMS[:8]} == {0, 1, 2, 3} and {f[2] for f in V.GLOAD_FORMS[8:12]} == {0, 2}
    g = V.group_lanes("gload")
    for k in (4, 5, 6, 7, 10, 11):
        for wave in range(4):
            lanes = g[(wave * 88 + k) * 64:(wave * 88 + k + 1) * 64]
            assert any(v >> 31 for v in lanes) and not all(v >> 31 for v in lanes), (k, wave)
    # every buffer instruction has lanes in range and out of range, up to the boundary on both sides
    for w, n in enumerate(V.BUF_BYTES):
        for m in range(3):
            inside = [V.buffer_lane(*V.buf_operands(w, m, lane), n, V.BUF_RECORDS) for lane in range(64)]
            assert inside == [True] * 32 + [False] * 32
            assert sum(V.buf_operands(w, m, 31)) + V.buf_stride(w) == V.BUF_RECORDS
            vo, _so, imm = V.buf_operands(w, m, 32)
            assert vo + imm == V.BUF_RECORDS
            assert all(0 <= sum(V.buf_operands(w, m, lane)) and sum(V.buf_operands(w, m, lane)) + n <= V.WAVE_BYTES for lane in range(64))
    # min and max pick each side, cmpswap succeeds and fails, inc and dec wrap and do not
    for m in range(2):
        for wave in range(4):
            for i, (op, bits) in enumerate(V.ATOMICS):
                rows = [V.atom_operands(m, wave, lane, i) for lane in range(64)]
                after = [V.atomic(op, bits, a, v, c) for a, v, c in rows]
                if op in ("smin", "umin", "smax", "umax"):
                    assert {x == a for x, (a, _v, _c) in zip(after, rows)} == {True, False}, (op, bits)
                if op == "cmpswap":
                    assert {x == v for x, (_a, v, _c) in zip(after, rows)} == {True, False}
                if op == "inc":
                    assert 0 in after and any(x == a + 1 for x, (a, _v, _c) in zip(after, rows))
                if op == "dec":
                    assert any(x == v and a == 0 for x, (a, v, _c) in zip(after, rows)) and any(x == v and a > v for x, (a, v, _c) in zip(after, rows))
                    assert any(x == a - 1 for x, (a, _v, _c) in zip(after, rows))
            b, c = V.contended(m, wave)
            assert b + 64 * c < 1 << 32 and c & 1
    # l1: each pass reads every chunk of the table once, in another order
    for p in range(2):
        assert sorted(V.l1_chunk(p, s, lane) for s in range(32) for lane in range(64)) == list(range(2048))
    assert [V.l1_chunk(0, 0, lane) for lane in range(64)] != [V.l1_chunk(1, 0, lane) for lane in range(64)]


def test_spot_values_by_hand_loads_and_stores():
    mem = V.Memory(16, [0x8091A2B3, 0x7F6E5D4C, 0x11223344, 0xFFEEDDCC])
    # bytes in memory order: b3 a2 91 80 4c 5d 6e 7f ...
    assert V.load_ext(mem, 0, 1, False) == 0xB3 and V.load_ext(mem, 0, 1, True) == 0xFFFFFFB3           # sbyte sign-extends
    assert V.load_ext(mem, 4, 1, True) == 0x4C and V.load_ext(mem, 3, 1, True) == 0xFFFFFF80
    assert V.load_ext(mem, 2, 2, False) == 0x8091 and V.load_ext(mem, 2, 2, True) == 0xFFFF8091
    assert V.load_ext(mem, 6, 2, True) == 0x7F6E
    assert V.load_d16(mem, 0, 1, True) == 0xFFB3 and V.load_d16(mem, 0, 1, False) == 0x00B3 and V.load_d16(mem, 2, 2, False) == 0x8091
    assert mem.words(0, 3) == [0x8091A2B3, 0x7F6E5D4C, 0x11223344] and mem.words(8, 2) == [0x11223344, 0xFFEEDDCC]
    mem.store(5, 1, 0xABCDEF12)                                  # a byte store writes the low byte and nothing else
    assert mem.words(4, 1) == [0x7F6E124C]
    mem.store(10, 2, 0xABCD9876)                                 # a short store the low half
    assert mem.words(8, 1) == [0x98763344]
    mem.store(0, 12, 0x0C0C0C0C_0B0B0B0B_0A0A0A0A)               # dwordx3: the fourth word stays
    assert mem.words(0, 4) == [0x0A0A0A0A, 0x0B0B0B0B, 0x0C0C0C0C, 0xFFEEDDCC]
    for corner in (lambda: mem.load(2, 4), lambda: mem.load(4, 12), lambda: mem.store(1, 2, 0), lambda: V.lds_dma_dest(0, 1, 12),
                   lambda: V.lds_dma_dest(0, 1, 2)):
        with pytest.raises(ValueError, match="left out"):
            corner()
    # the group's words: gstore form 2 (short_d16_hi) on wave 1, lane 9 stores bits 31:16 of its register at byte 2 * ((9 + 3) & 7) = 8
    g = V.group_lanes("gstore")
    chunk = V.gstore_chunk(1, 9, 2)
    want = (V.val(V.T_GSTORE_BG, 1, 0, 2, chunk // 4 + 2) & 0xFFFF0000) | (V.val(V.T_GSTORE, 1, 9, 2, 0) >> 16)
    assert V.gstore_sub(9, 2) == 8 and g[(1 * 28 + 4 * 2 + 2) * 64 + 9] == want
    assert g[(1 * 28 + 4 * 2 + 3) * 64 + 9] == V.val(V.T_GSTORE_BG, 1, 0, 2, chunk // 4 + 3)             # the neighbouring word is background
    # gload: word k = 0 is the unsigned byte at byte 0 of chunk (wave * 64 + lane) of the table
    assert V.group_lanes("gload")[(2 * 88 + 0) * 64 + 5] == V.table_word(4 * (2 * 64 + 5)) & 0xFF
    assert V.group_lanes("l1")[(3 * 256 + 7) * 64 + 11] == V.table_word(4 * (1 * 64 + 11) + 3)           # pass 0, step 1, word 3


def test_spot_values_by_hand_buffer_lds_and_transpose():
    assert V.buffer_lane(1020, 0, 0, 4, 1024) and not V.buffer_lane(1024, 0, 0, 4, 1024)                 # the last dword in range, the first out
    assert V.buffer_lane(896, 64, 48, 16, 1024) and not V.buffer_lane(976, 64, 48, 16, 1024)
    for vo, so, imm, n in ((1016, 0, 0, 16), (960, 64, 0, 4), (1023, 0, 0, 2)):                          # partly out; only soffset decides
        with pytest.raises(ValueError, match="left out"):
            V.buffer_lane(vo, so, imm, n, 1024)
    g = V.group_lanes("buffer")
    assert all(g[(0 * 108 + k) * 64 + lane] == 0 for k in range(36) for lane in (32, 47, 63))            # out-of-range loads read 0
    assert g[(0 * 108 + 2) * 64 + 31] == V.val(V.T_BUF_BG, 0, 0, 0, 1020 // 4)                            # dword, offen, lane 31: the last word in range
    k = 36 + 4 * (3 * 2 + 0)                                                                              # the dword store, offen
    assert g[(0 * 108 + k + 3) * 64 + 31] == V.val(V.T_BUF, 0, 31, 6, 0)                                  # lane 31 wrote the chunk's last word
    assert g[(0 * 108 + k + 0) * 64 + 32] == V.val(V.T_BUF_BG, 0, 0, 1 + 6, 1024 // 4)                    # lane 32's store was dropped
    # the transposed read, on a 4 x 16 block whose element (row, col) is 16 row + col, rows 32 bytes apart
    mem = V.Memory(V.LDS_WAVE_BYTES)
    for row in range(16):
        for col in range(16):
            mem.store(32 * row + 2 * col, 2, 16 * row + col)
    got = V.tr_b16(mem, [V.ldstr_addr(0, lane) for lane in range(64)])
    assert got[0] == [0 | 16 << 16, 32 | 48 << 16]               # lane 0: column 0 of rows 0..3
    assert got[5] == [5 | 21 << 16, 37 | 53 << 16]               # lane 5: column 5
    assert got[16 + 15] == [79 | 95 << 16, 111 | 127 << 16]      # group 1, lane 15: column 15 of rows 4..7
    assert V.ldstr_addr(1, 23) == 5 * 48 + 24                    # lane 23 = 16 + 4 * 1 + 3 supplies row 5, columns 12..15
    with pytest.raises(ValueError, match="left out"):
        V.tr_b16(mem, [0] * 63)
    # ds_read2st64_b32 offset1:16 reaches 16 * 64 * 4 = 4096 bytes on
    lanes = V.group_lanes("lds")
    k = V.GROUP_WORDS["lds"] * 0 + 20                           # map 0: read forms 0..9 take 20 words; form 10 follows
    assert lanes[(0 * 222 + k + 1) * 64 + 3] == V.val(V.T_LDS_BG, 0, 0, 0, (16 * 3 + 4096) // 4)


def test_spot_values_by_hand_atomics():
    assert V.atomic("add", 32, M32, 2) == 1 and V.atomic("sub", 32, 1, 2) == M32
    assert V.atomic("smin", 32, M32, 1) == M32 and V.atomic("umin", 32, M32, 1) == 1           # -1 < 1 signed
    assert V.atomic("smax", 32, M32, 1) == 1 and V.atomic("umax", 32, M32, 1) == M32
    assert (V.atomic("and", 32, 0xC, 0xA), V.atomic("or", 32, 0xC, 0xA), V.atomic("xor", 32, 0xC, 0xA)) == (8, 0xE, 6)
    assert V.atomic("inc", 32, 5, 5) == 0 and V.atomic("inc", 32, 4, 5) == 5 and V.atomic("inc", 32, 9, 5) == 0     # wraps at the operand
    assert V.atomic("dec", 32, 0, 5) == 5 and V.atomic("dec", 32, 9, 5) == 5 and V.atomic("dec", 32, 3, 5) == 2
    assert V.atomic("swap", 64, 1, 1 << 40) == 1 << 40
    assert V.atomic("cmpswap", 32, 7, 9, cmp=7) == 9 and V.atomic("cmpswap", 32, 7, 9, cmp=6) == 7
    assert V.atomic("add", 64, (1 << 64) - 1, 2) == 1 and V.atomic("umax", 64, 1 << 63, 5) == 1 << 63
    g = V.group_lanes("atomic")
    b, c = V.contended(1, 2)
    k = 46 + 42                                                   # LDS, after the 17 operations
    assert [g[(2 * 92 + k + j) * 64 + 9] for j in range(4)] == [1, M32, M32, b + 64 * c]
    a, v, _cmp = V.atom_operands(0, 3, 4, 0)
    assert g[(3 * 92 + 0) * 64 + 4] == a and g[(3 * 92 + 1) * 64 + 4] == (a + v) & M32               # add returns a and leaves a + v


def test_parse_mem():
    assert V.parse_mem(None) == V.parse_mem("") == V.parse_mem([]) == []
    assert V.parse_mem("all") == list(V.GROUPS) and len(V.GROUPS) == 8
    assert V.parse_mem("atomic, gload,lds") == ["gload", "lds", "atomic"] == V.parse_mem(["lds", "atomic", "gload"])   # bit order
    with pytest.raises(ValueError, match="unknown memory group"):
        V.parse_mem("gload,flat")


# ----------------------------------------------------------------------------- fold_mem
def test_fold_clean_and_uncovered_is_no_failure():
    f = V.fold_mem(_clean(), V.GROUPS, 256)
    assert f["failed"] == {} and f["cus"] == [] and f["cus_seen"] == 256 and f["cus_uncovered"] == 0 and f["simds_seen_min"] == 4
    f = V.fold_mem(_clean(ALL[:250]), V.GROUPS, set(ALL))
    assert f["failed"] == {} and f["cus_uncovered"] == 6 and f["uncovered"] == [list(k) for k in ALL[250:]]


@pytest.mark.parametrize("group", V.GROUPS)
def test_fold_one_failing_cu_per_group(group):
    last = V.group_indices(group) - 1
    f = V.fold_mem(_clean() + [_bad(5, 9, group, last, 2)] + _clean([(5, 9)]), V.GROUPS, 256)
    assert f["failed"] == {group: [[5, 9]]}                                # a clean revisit clears nothing
    assert f["cus"] == [{"xcc": 5, "cu_key": 9, "kinds": [group], "waves": 0b100, "bad_group": group, "bad_index": last, "bad_wave": 2}]


def test_fold_two_groups_and_two_visits():
    g0, g7 = 1 << 0, 1 << 7
    f = V.fold_mem(_clean() + [_rec(2, 3, fail=0b1010, gbits=g0 | g7, group=0, index=77, wave=1), _bad(2, 3, "gload", 12, 0)], V.GROUPS, 256)
    assert f["failed"] == {"gload": [[2, 3]], "atomic": [[2, 3]]}
    assert (f["cus"][0]["bad_group"], f["cus"][0]["bad_index"], f["cus"][0]["bad_wave"], f["cus"][0]["waves"]) == ("gload", 12, 0, 0b1011)


def test_fold_garbled_record():
    for bad in (_rec(4, 4, fail=0x10, gbits=1, group=0, index=0, wave=0), _rec(4, 4, fail=1), _rec(4, 4, gbits=1),
                _rec(4, 4, fail=1, gbits=1 << 8, group=8, index=0, wave=0), _rec(4, 4, fail=1, gbits=2, group=0, index=0, wave=0),
                _rec(4, 4, fail=1, gbits=3, group=1, index=0, wave=0), _rec(4, 4, fail=1, gbits=1, group=0, index=88 * 64, wave=0),
                _rec(4, 4, fail=2, gbits=1, group=0, index=0, wave=0), _rec(4, 4, index=3)):
        assert "record" in V.fold_mem(_clean() + [bad], V.GROUPS, 256)["failed"], bad


# ----------------------------------------------------------------------------- deep_selftest over a fake probe
class _FakeProbe:
    """256 CUs; `bad[dev]` = [(xcc, key, group, index, wave)]: that CU fails that group when it is selected."""

    def __init__(self, n=2, bad=None, cus=256):
        self.n, self.cus, self.bad = n, cus, bad or {}
        self.calls = []                  # ("sweep" | "scalar" | "mem", dev, mask, rounds[, names])

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

    def cu_sweep_scalar(self, dev, mask, rounds, seed, groups, inject=None, corrupt_expected=None):
        self.calls.append(("scalar", dev, list(mask), rounds, list(groups)))
        return {"records": [(x, _hw(k), 0, 0xF, 0, -1, -1, -1) for x, k in self._keys(mask)], "groups": list(groups),
                "checked": list(groups), "sreg_slots": 88, "num_regs": 16, "scratch_bytes": 0, "ms": 0.3}

    def cu_sweep_mem(self, dev, mask, rounds, seed, groups, inject=None, corrupt_expected=None):
        self.calls.append(("mem", dev, list(mask), rounds, list(groups)))
        keys = self._keys(mask)
        recs = _clean(keys)
        for x, k, group, index, wave in self.bad.get(dev, ()):
            if group in groups and (x, k) in keys:
                recs.append(_bad(x, k, group, index, wave))
        return {"records": recs, "groups": list(V.GROUPS), "checked": list(groups), "table_words": 8192, "slice_bytes": 8192,
                "num_regs": 128, "scratch_bytes": 0, "ms": 0.4}

    def hbm_pattern_check(self, dev, nbytes, seed, passes=2, corrupt=(), verify_seed=None, cu_mask=None):
        return {"bytes": nbytes, "errors": 0, "first": [], "fill_gbs": 5000.0, "verify_gbs": 6000.0}

    def mem_calls(self):
        return [c for c in self.calls if c[0] == "mem"]


class _OldProbe(_FakeProbe):
    cu_sweep_mem = property()        # hasattr() is False


def test_the_mem_launch_follows_each_sweep_launch_on_the_same_mask():
    P = _FakeProbe()
    rep = S.deep_selftest(P, 0, mem="all", seed=1)
    assert rep.ok and rep.mem["checked"] == list(V.GROUPS) and rep.mem["failed"] == {} and rep.mem["table_words"] == 8192
    assert [c[0] for c in P.calls] == ["sweep", "mem"] and P.calls[0][2:4] == P.calls[1][2:4]
    assert set(rep.to_dict()["mem"]) == {"checked", "failed", "cus", "table_words", "ms"}
    P = _FakeProbe()
    S.deep_selftest(P, 0, cu_mask_bits=list(range(40, 48)), scalar="add", mem="l1,atomic", seed=1)
    assert [c[0] for c in P.calls] == ["sweep", "scalar", "mem"] and P.calls[2][4] == ["l1", "atomic"]   # after the scalar launch
    assert P.calls[0][2] == P.calls[1][2] == P.calls[2][2] != []
    assert S.PARTS[-1] is V.PART

    class Shy(_FakeProbe):                 # the first two launches miss a CU: the coverage loop runs three times
        def cu_sweep(self, dev, mask, rounds, seed, inject=None):
            out = super().cu_sweep(dev, mask, rounds, seed)
            if rounds < 16:
                out["records"] = out["records"][1:]
            return out

    P = Shy()
    rep = S.deep_selftest(P, 0, mem="lds", seed=1)
    assert [c[0] for c in P.calls] == ["sweep", "mem"] * 3 and [c[3] for c in P.calls] == [4, 4, 8, 8, 16, 16] and rep.ok


@pytest.mark.parametrize("group", V.GROUPS)
def test_ok_is_false_exactly_when_a_group_failed(group):
    bad = _FakeProbe(bad={0: [(3, 17, group, 5, 1)]})
    rep = S.deep_selftest(bad, 0, mem="all", seed=1)
    assert not rep.ok and rep.mem["failed"] == {group: [[3, 17]]} and rep.sweep["failed"] == []
    assert S.failed_cus(rep) == {(3, 17)} and S.fenceable(rep)
    assert f"memory pipeline {group} on CU (xcc 3, key 0x11), first in {group} at index 5, wave 1" in rep.describe_failure()
    others = [g for g in V.GROUPS if g != group]
    assert S.deep_selftest(bad, 0, mem=others, seed=1).ok                  # the bad group is not asked for
    assert S.deep_selftest(bad, 1, mem="all", seed=1).ok                   # nor is the other device bad


def test_a_garbled_mem_record_is_not_fenceable():
    class Garbled(_FakeProbe):
        def cu_sweep_mem(self, *a, **kw):
            out = super().cu_sweep_mem(*a, **kw)
            out["records"].append(_rec(0, 0, fail=0x10))
            return out

    rep = S.deep_selftest(Garbled(), 0, mem="all", seed=1)
    assert not rep.ok and "record" in rep.mem["failed"] and not S.fenceable(rep)


def test_without_mem_nothing_changes():
    P = _FakeProbe()
    rep = S.deep_selftest(P, 0, seed=1)
    assert rep.ok and rep.mem is None and P.mem_calls() == [] and [c[0] for c in P.calls] == ["sweep"]
    assert sorted(rep.to_dict()) == sorted(["device", "ok", "seconds", "sweep", "hbm", "error", "masked", "seed", "notes", "paths"])
    for spec in (None, "", []):
        assert S.deep_selftest(P, 0, mem=spec, scalar="all", seed=1).mem is None
    assert P.mem_calls() == []
    assert "mem" not in S.deep_selftest(P, 0, scalar="all", seed=1).to_dict()
    assert "mem" not in repr(S.DeepReport(device=0, mem={"checked": []}))    # repr=False, default None
    assert S.DeepReport(device=0).mem is None


def test_an_older_probe_gets_a_note():
    P = _OldProbe()
    assert not hasattr(P, "cu_sweep_mem")
    rep = S.deep_selftest(P, 0, mem="all", seed=1)
    assert rep.ok and rep.mem is None and "mem" not in rep.to_dict() and any("no cu_sweep_mem" in n for n in rep.notes)
    assert not S.deep_selftest(_FakeProbe(), 0, mem="all", seed=1).notes


def test_localise_failure_and_would_fence_pass_mem():
    P = _FakeProbe(bad={0: [(3, 17, "atomic", 0, 0)]})
    rep = S.deep_selftest(P, 0, mem="atomic", seed=1)
    P.calls.clear()
    loc = S.localise_failure(P, 0, rep, range(32), 8, mem=["atomic"])
    assert loc.bad_units == [17] and loc.unexplained == []
    assert len(P.mem_calls()) == 32 and all(c[4] == ["atomic"] for c in P.mem_calls())
    plan = S.would_fence(P, 0, rep, 1, mem=["atomic"])
    assert plan["units"] == [17] and [3, 17] in plan["cus"]["17"]
    assert S.would_fence(P, 0, rep, 1)["units"] == []                      # without the part nothing fails again


def test_the_agents_fence_run_carries_mem():
    from nanogpu.agent.plugin import NanoGpuPlugin

    async def main():
        store = FakeKubeStore()
        topo = synthetic_mi355x(1)
        store.add_node(pu.make_node("n0", 1, topo.to_json()))
        api = InProcKube(store)
        agent = NodeAgent(api, "n0", topo, device_plugin=False, health_period_s=0, selftest_hbm_mib=64,
                          selftest_fence=1, selftest_mem="ldstr,gload")
        agent.plugin = NanoGpuPlugin(topo, api, "n0")
        P = _FakeProbe(1, bad={0: [(3, 17, "ldstr", 255, 3)]})
        assert await agent.selftest(P) == []
        assert agent.topo.devices[0].healthy and agent.topo.devices[0].fenced == [17] and agent.plugin.cus[0].fenced == {17}
        rep = agent.selftest_stats["reports"][0]
        assert rep["mem"]["checked"] == ["gload", "ldstr"] and rep["mem"]["failed"] == {}
        assert any("first in ldstr at index 255, wave 3" in n for n in rep["notes"])
        # the first sweep, 32 units swept alone, the verification: each with its mem launch on the same mask
        sweeps = [c for c in P.calls if c[0] == "sweep"]
        assert len(P.mem_calls()) == len(sweeps) == 34 and all(c[4] == ["gload", "ldstr"] for c in P.mem_calls())
        assert [c[2] for c in P.mem_calls()] == [c[2] for c in sweeps]

    asyncio.run(main())


# ----------------------------------------------------------------------------- flags, help, docs, metrics
def _agent(n=2, **kw):
    store = FakeKubeStore()
    topo = synthetic_mi355x(n)
    store.add_node(pu.make_node("n0", n, topo.to_json()))
    return NodeAgent(InProcKube(store), "n0", topo, device_plugin=False, health_period_s=0, **kw), store


def test_flags_parse_and_imply_deep(capsys):
    ap = build_parser()
    a = ap.parse_args(["--node-name", "n", "--selftest-mem", "atomic,gload"])
    assert a.selftest and a.selftest_deep and a.selftest_mem == ["gload", "atomic"]
    assert ap.parse_args(["--selftest-mem", "all"]).selftest_mem == list(V.GROUPS)
    assert ap.parse_args(["--node-name", "n", "--selftest-deep"]).selftest_mem == []        # the default is off
    for bad, wording in (("gload,flat", "--selftest-mem: unknown memory group(s) ['flat']: choose from gload, l1, gstore, buffer, lds, ldstr, "
                                        "ldsdma, atomic or 'all'"),
                         ("", "--selftest-mem: name at least one group, or 'all'")):
        with pytest.raises(SystemExit) as e:
            ap.parse_args(["--selftest-mem", bad])
        assert e.value.code == 2 and wording in " ".join(capsys.readouterr().err.split())
    agent = NodeAgent(None, "n", synthetic_mi355x(1), device_plugin=False, selftest_mem="l1")
    assert agent.selftest_deep and agent.selftest_parts.mem == ["l1"]
    assert not NodeAgent(None, "n", synthetic_mi355x(1), device_plugin=False).selftest_parts.mem
    with pytest.raises(SystemExit) as e:
        S.main(["--mem", "gload,nope"])
    assert e.value.code == 2 and "unknown memory group(s) ['nope']" in capsys.readouterr().err


def test_the_command_runs_the_part(monkeypatch, capsys):
    from nanogpu import native

    P = _FakeProbe(bad={0: [(1, 2, "buffer", 70, 2)]})
    monkeypatch.setattr(native, "probe", lambda required=False: P)
    assert S.main(["--hbm-mib", "64", "--mem", "all"]) == 1
    out = capsys.readouterr().out
    assert "memory pipeline gload, l1, gstore, buffer, lds, ldstr, ldsdma, atomic (8192 table words, 0.400 ms): buffer failed on 1 CU(s)" in out
    assert "first in buffer at index 70, wave 2" in out
    assert S.main(["--hbm-mib", "64", "--mem", "gload", "--json"]) == 0
    assert json.loads(capsys.readouterr().out)["mem"]["checked"] == ["gload"]


def test_both_help_texts_are_those_of_parsers_without_the_part(monkeypatch, capsys):
    """The part is not listed: --help of the command and of the agent are byte for byte what they are without it."""
    assert V.PART.listed is False and all(p.listed for p in S.PARTS[:-1])
    monkeypatch.setenv("COLUMNS", "100")

    def texts():
        with pytest.raises(SystemExit):
            S.main(["--help"])
        return capsys.readouterr().out, build_parser().format_help()

    with_part = texts()
    without_parts = S.PARTS[:-1]
    monkeypatch.setattr(S, "PARTS", without_parts)
    without = texts()
    assert with_part == without and "--mem" not in with_part[0] and "selftest-mem" not in with_part[1]
    assert "--scalar" in with_part[0] and "--selftest-scalar" in with_part[1]
    # a listed part would show: the flag is hidden by `listed`, not by accident
    monkeypatch.setattr(S, "PARTS", without_parts + (dataclasses.replace(V.PART, listed=True),))
    shown = texts()
    assert "--mem all|LIST" in shown[0] and "--selftest-mem all|LIST" in shown[1]


def test_the_reference_names_both_flags():
    text = (ROOT / "docs" / "REFERENCE.md").read_text()
    assert "--selftest-mem" in text and "--mem all|LIST" in text and "nanogpu_selftest_mem_checked" in text
    readme = (ROOT / "README.md").read_text()
    assert "--selftest-mem" in readme and "selftest_mem_host.h" in readme


def test_agent_marks_the_device_unhealthy_and_renders_the_metric():
    async def main():
        agent, _ = _agent(2, selftest_mem="all", selftest_hbm_mib=64)
        await agent.start()
        P = _FakeProbe(2, bad={1: [(3, 17, "l1", 4097, 1)]})
        assert await agent.selftest(P) == [1]
        assert [d.healthy for d in agent.topo.devices] == [True, False]
        assert agent.selftest_stats["reports"][1]["mem"]["failed"] == {"l1": [[3, 17]]}
        text = render_metrics(agent.topo, None, None, "/nonexistent", agent.selftest_stats)
        for line in ('nanogpu_selftest_mem_checked{device="0"} 8', 'nanogpu_selftest_mem_checked{device="1"} 8',
                     "# TYPE nanogpu_selftest_mem_checked gauge"):
            assert line in text.splitlines(), line
        plain, _ = _agent(2, selftest_deep=True)
        await plain.start()
        Q = _FakeProbe(2, bad={1: [(3, 17, "l1", 4097, 1)]})
        assert await plain.selftest(Q) == [] and Q.mem_calls() == []              # without the flag: today's kernels only
        assert "mem" not in plain.selftest_stats["reports"][0]
        assert "nanogpu_selftest_mem" not in render_metrics(plain.topo, None, None, "/nonexistent", plain.selftest_stats)
        for a in (agent, plain):
            await a.stop()

    asyncio.run(main())
