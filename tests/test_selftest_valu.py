"""Vector-ALU part of the deep self-test, without a GPU: the host header's stand-alone program
against the Python twin, the twin's own conditions and hand-derived values, parsing, folding,
deep_selftest over a fake probe, the agent's flag and the metric."""
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
from nanogpu.probe import selftest_valu as V
from nanogpu.topology.model import synthetic_mi355x

GIB = 1 << 30
ALL = [(x, k) for x in range(8) for k in range(32)]
HASH = 0x1234ABCD


def _hw(key, simd=0):
    return (key << 8) | (simd << 4)


def _rec(x, k, fail=0, gbits=0, slot=-1, thread=-1, ahash=HASH):
    return (x, _hw(k), fail, 0xF, gbits, slot, thread, ahash)


def _clean(keys=ALL):
    return [_rec(x, k) for x, k in keys]


# ----------------------------------------------------------------------------- host program and twin
@pytest.mark.parametrize("kind", ["plain", "asan"])
def test_host_program_agrees_with_the_twin(kind):
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "native"))
    import build  # native/build.py

    exe = build.build_selftest_host(kind, target="valu")
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    host = json.loads(r.stdout)
    twin = V.twin_summary()
    assert list(host["groups"]) == list(V.EXACT_GROUPS)
    for g in V.EXACT_GROUPS:
        assert host["groups"][g] == twin["groups"][g], g
    assert host["approx_checksum"] == twin["approx_checksum"]
    assert host["reg_slots"] == V.REG_SLOTS >= 448 and host["record_words"] == V.RECORD_WORDS


def test_twin_conditions_hold():
    for g in V.EXACT_GROUPS:
        words, c = V.group_expected(g)
        assert len(words) == 128 and c.abnormal == 0, g           # every operand and result finite, normal, nonzero
        assert V.uncovered_bits(words, 0) == 0 and V.uncovered_bits(words, 1) == 0, g   # no listed exception
        if g in V.FP_GROUPS:
            assert min(c.eff_add, c.eff_sub, c.round_up, c.round_down) > 0, g
    for g in ("int32", "int64"):
        c = V.group_expected(g)[1]
        assert min(c.carry31, c.carry63, c.borrow63) > 0, g
    c = V.group_expected("cvt")[1]
    assert all(n > 0 for n in c.tie_up + c.tie_down) and c.round_up > 0 and c.round_down > 0
    xl = V.group_expected("xlane")[0]
    for w in range(2):
        assert len({xl[2 * lane + w] for lane in range(64)}) == 64


def test_spot_values_by_hand():
    c = V.Conds()
    # fma32: 1/8 * 1 + 1 = 1.125; (1/8 + ulp)(2 - ulp) - 1 is just below -0.75 in magnitude... rounds to -0.75
    assert V.fma(0x3E000000, 0x3F800000, 0x3F800000, V.F32, c) == 0x3F900000
    assert V.fma(0x3E000001, 0x3FFFFFFF, 0xBF800000, V.F32, c) == 0xBF400000
    # fma64: 0.125 * 1.5 + 1 = 1.1875
    assert V.fma(0x3FC0000000000000, 0x3FF8000000000000, 0x3FF0000000000000, V.F64, c) == 0x3FF3000000000000
    # f16: 0.125 * (1 + 2^-10) + 1 = 1.125 + 2^-13: below half an ulp (2^-11) of 1.125, rounds down
    assert V.fma(0x3000, 0x3C01, 0x3C00, V.F16, c) == 0x3C80
    # bf16 tie, derived by hand: 1 + 2^-8 lies between 1 and 1 + 2^-7, goes to the even 1; 1 + 3 * 2^-8 goes up
    assert V._cvt(0x3F808000, V.BF16, 0, c) == 0x3F80 and V._cvt(0x3F818000, V.BF16, 0, c) == 0x3F82
    assert c.tie_down[0] == 1 and c.tie_up[0] == 1
    # fp8 (e4m3, bias 7) without saturation: 3.7 = 1.85 x 2, 1.85 is between 1.75 and 1.875, nearer 1.875 -> 0x47
    assert V._cvt(V.float_bits(3.7), V.E4M3, 2, c) == 0x47 and V._cvt(V.float_bits(-1.0625), V.E4M3, 2, c) == 0xB8
    assert V._cvt(V.float_bits(1.375), V.E5M2, 3, c) == 0x3E                        # tie to the even 1.5
    assert V._cvt(0x3F801000, V.F16, 1, c) == 0x3C00 and V._cvt(0x3F803000, V.F16, 1, c) == 0x3C02
    # v_perm selector: bytes 0..3 are the second operand's, 4..7 the first's
    assert V.perm(0x44332211, 0x88776655, 0x07040300) == 0x44118855
    assert V.bfe_u(0xABCD1234, 4, 8) == 0x23 and V.bfe_i(0xABCD1234, 16, 4) == 0xFFFFFFFD
    assert V.round_rne(V.Fraction(0x40000040), V.F32, c)[0] == 0x4E800000           # 31 bits, tie to even
    assert V.ordered_key(0x3F800000) == 0xBF800000 and V.ordered_key(0x80000000) + 1 == V.ordered_key(0)
    assert c.abnormal == 0
    assert V.operand("fma32", 0, 0, 0) == C.mix32(0x5A17C0DE) and V.f32_win(0xFFFFFFFF, -3) == 0xBE7FFFFF


def test_spot_values_by_hand_of_the_other_groups():
    """One step of each remaining group, every expected value worked out on paper (in the comments)."""
    c = V.Conds()
    # pkfma32: the pair (1/8 * 1 + 1, 1/8 * -2 + 1.5) = (1.125, 1.25); the elements do not mix
    assert V.pkfma32([0x3E000000, 0x3E000000], [0x3F800000, 0xC0000000], [0x3F800000, 0x3FC00000], c) == [0x3F900000, 0x3FA00000]
    assert V.pkfma32([0x3E000000, 0x3F800000], [0x3F800000, 0x3F800000], [0x3F800000, 0xBF000000], c) == [0x3F900000, 0x3F000000]   # 1 * 1 - 0.5
    # addmul32 where the fused result differs: a = x = 1 + 2^-12, so a * x = 1 + 2^-11 + 2^-24; 2^-24 is half an
    # ulp of 1 and the kept mantissa is even, so the product rounds down to 1 + 2^-11. Minus 1: separately rounded
    # 2^-11 exactly, fused 2^-11 + 2^-24 = 2^-11 (1 + 2^-13), which f32 holds.
    a = x = 0x3F800800
    assert V.mul32(a, x, c) == 0x3F801000
    assert V.add32(V.mul32(a, x, c), 0xBF800000, c) == 0x3A000000
    assert V.fma(a, x, 0xBF800000, V.F32, c) == 0x3A000400
    # int32, x = y = 2^32 - 1, a = 1, b = 0, k = 1: lo = x * a = 2^32 - 1, hi = mulhi(y, 0) = 0,
    # (a ^ y)(b ^ x) = (2^32 - 2)(2^32 - 1) = 2^64 - 3 * 2^32 + 2 = 0xfffffffd_00000002 (mod 2^64),
    # t = that + 0xffffffff = 0xfffffffe_00000001; 0xffffffff_ffffffff + t: the low words carry across bit 31,
    # the high words across bit 63, leaving 0xfffffffe_00000000; minus 1 borrows across bit 31: 0xfffffffd_ffffffff
    ci = V.Conds()
    assert V.int32_step(0xFFFFFFFF, 0xFFFFFFFF, 1, 0, 1, ci) == (0xFFFFFFFF, 0xFFFFFFFD)
    assert (ci.carry31, ci.carry63, ci.borrow63) == (2, 1, 0)
    # a borrow across bit 63: state 0, a = b = 0 gives t = (0 ^ 0)(0 ^ 0) + 0 = 0; 0 - 1 = 2^64 - 1
    assert V.int32_step(0, 0, 0, 0, 1, ci) == (0xFFFFFFFF, 0xFFFFFFFF) and ci.borrow63 == 1
    # int64, x = 2^63 - 1, k1 = 1: the sum 2^63 carries across bit 31, not 63. Shifts: left 0, logical right 63
    # (sh = 63 << 8 | 60 << 16): 2^63 ^ 1; minus k2 = 1: 2^63, negative as a signed value; arithmetic right 60
    # fills with ones: 0xffffffff_fffffff8; 2^63 << 7 is 0 modulo 2^64, so that is the result
    c64 = V.Conds()
    assert V.int64_step(0x7FFFFFFFFFFFFFFF, 1, 1, (63 << 8) | (60 << 16), c64) == 0xFFFFFFFFFFFFFFF8
    assert (c64.carry31, c64.carry63, c64.borrow63) == (1, 0, 0)
    # the logical right shift of the same value fills with zeros: x = 2^63, no add, left 0 ^ right 60 = 2^63 | 8,
    # minus 0, arithmetic right 0 ^ (x << 7 = 8 << 7 = 0x400): 0x80000000_00000408
    assert V.int64_step(0x8000000000000000, 0, 0, 60 << 8, c64) == 0x8000000000000408
    # dot: bytes, low first, (4, 3, 2, 1) . (8, 7, 6, 5) = 32 + 21 + 12 + 5 = 70, plus 10
    assert V.udot4(0x01020304, 0x05060708, 10) == 80
    assert V.udot4(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF) == (4 * 255 * 255 - 1) & 0xFFFFFFFF      # wraps past 2^32
    # signed: (4, 3, 2, -1) . (8, 7, -2, 5) = 32 + 21 - 4 - 5 = 44; four times -128 * 127 = -65024 = 0xffff0200
    assert V.sdot4(0xFF020304, 0x05FE0708, 0) == 44
    assert V.sdot4(0x80808080, 0x7F7F7F7F, 0) == 0xFFFF0200
    # xlane on x[l] = l, operands 0, row_ror:1, read lane 5 (rotl(5, 13) = 40960):
    # lane 0 reads lane 15 of its row (rotation right, wrapping inside the row) and lane 32:
    #   (15 ^ 32 << 7) + 40960 = (15 ^ 4096) + 40960 = 4111 + 40960 = 45071
    # lane 16 reads lane 31 (its own row, not lane 15) and lane 48: (31 ^ 6144) + 40960 = 6175 + 40960 = 47135
    # lane 33 reads lane 32 and lane 1: (32 ^ 128) + 40960 = 160 + 40960 = 41120
    out = V.xlane_step(list(range(64)), 1, 5, [0] * 64)
    assert (out[0], out[16], out[33]) == (45071, 47135, 41120)
    # row_ror:3 at lane 2 reads lane 15 (2 - 3 mod 16) and lane 34, and the operand is added:
    # 34 << 7 = 4352 = 0x1100, 15 ^ 0x1100 = 0x110f = 4367; 4367 + 40960 + 7 = 45334
    assert V.xlane_step(list(range(64)), 3, 5, [7] * 64)[2] == 45334
    assert c.abnormal == 0
    assert V.reg_word(3, 200, 5, 1) == V.reg_word(3, 200, 5, 0) ^ 0xFFFFFFFF != V.reg_word(3, 201, 5, 1)


def test_approx_inputs_and_ranges():
    r = V.approx_ranges()
    assert len(r) == 5 * 64 * 2 and all(r[i + 1] - r[i] == 16 for i in range(0, len(r), 2))
    for op in V.APPROX_OPS:
        for lane in range(64):
            x = V.bits_float(V.approx_input(op, lane))
            lo, hi = {"exp2": (-20, 20), "log2": (2, 2 ** 20)}.get(op, (2.0 ** -20, 2.0 ** 20))
            assert lo <= x <= hi and x != 0
            assert V.approx_ulp_distance(op, lane, V.approx_libm(op, x)) == 0
    assert V.approx_ulp_distance("sqrt", 0, V.bits_float(V.float_bits(V.approx_libm("sqrt", V.bits_float(V.approx_input("sqrt", 0)))) + 3)) == 3


def test_parse_valu():
    assert V.parse_valu(None) == V.parse_valu("") == V.parse_valu([]) == []
    assert V.parse_valu("all") == list(V.GROUPS) and len(V.GROUPS) == 13
    assert V.parse_valu("regs, fma32,cvt") == ["fma32", "cvt", "regs"] == V.parse_valu(["regs", "cvt", "fma32"])   # bit order
    with pytest.raises(ValueError, match="unknown vector-ALU group"):
        V.parse_valu("fma32,fma33")


# ----------------------------------------------------------------------------- fold_valu
def test_fold_clean_and_uncovered_is_no_failure():
    f = V.fold_valu(_clean(), V.GROUPS, 256)
    assert f["failed"] == {} and f["cus"] == [] and f["cus_seen"] == 256 and f["cus_uncovered"] == 0
    assert f["simds_seen_min"] == 4 and f["approx_hash"] == HASH
    f = V.fold_valu(_clean(ALL[:250]), V.GROUPS, set(ALL))
    assert f["failed"] == {} and f["cus_uncovered"] == 6 and f["uncovered"] == [list(k) for k in ALL[250:]]


def test_fold_one_group_on_waves_1_and_3_survives_a_clean_revisit():
    cvt = 1 << V.GROUPS.index("cvt")
    f = V.fold_valu(_clean() + [_rec(5, 9, fail=0b1010, gbits=cvt)] + _clean([(5, 9)]), V.GROUPS, 256)
    assert f["failed"] == {"cvt": [[5, 9]]}
    assert f["cus"] == [{"xcc": 5, "cu_key": 9, "kinds": ["cvt"], "waves": 0b1010, "bad_slot": -1, "bad_wave": -1, "bad_lane": -1}]


def test_fold_regs_reports_first_slot_and_lane():
    recs = _clean() + [_rec(2, 3, fail=0x40, slot=300, thread=2 << 6 | 17), _rec(2, 3, fail=0x10, slot=255, thread=63)]
    f = V.fold_valu(recs, V.GROUPS, 256)
    assert f["failed"] == {"regs": [[2, 3]]}
    assert f["cus"][0] == {"xcc": 2, "cu_key": 3, "kinds": ["regs"], "waves": 0b101, "bad_slot": 255, "bad_wave": 0, "bad_lane": 63}


def test_fold_approx_majority():
    one = [r for r in _clean() if (r[0], C.cu_key(r[1])) != (7, 31)] + [_rec(7, 31, ahash=HASH ^ 4)]
    assert V.fold_valu(one, V.GROUPS, 256)["failed"] == {"approx": [[7, 31]]}       # a minority of 1 in 256
    eight = [(x, 0) for x in range(8)]
    tie = [_rec(x, 0, ahash=HASH ^ (x & 1)) for x, _ in eight]
    f = V.fold_valu(tie, V.GROUPS, 8)
    assert f["failed"] == {"approx": [[x, 0] for x in range(8)]} and f["approx_hash"] is None   # 4-4: all fail
    assert V.fold_valu([_rec(0, 0, ahash=77)], V.GROUPS, 1)["failed"] == {}          # one CU: a trivial majority
    assert V.fold_valu([_rec(0, 0, fail=0x200, ahash=77)], V.GROUPS, 1)["failed"] == {"approx": [[0, 0]]}   # the bound guards it
    wave = V.fold_valu(_clean() + [_rec(1, 1, fail=0x4000)], V.GROUPS, 256)          # wave 2 unlike wave 0
    assert wave["failed"] == {"approx": [[1, 1]]} and wave["cus"][0]["waves"] == 0b100


def test_fold_garbled_record():
    f = V.fold_valu(_clean() + [_rec(4, 4, fail=0x10000)], V.GROUPS, 256)
    assert f["failed"] == {"record": [[4, 4]]}
    assert V.fold_valu(_clean() + [_rec(4, 4, fail=1, gbits=0)], V.GROUPS, 256)["failed"] == {"record": [[4, 4]]}
    assert "record" in V.fold_valu(_clean() + [_rec(4, 4, fail=1, gbits=1 << 12)], V.GROUPS, 256)["failed"]


# ----------------------------------------------------------------------------- deep_selftest over a fake probe
class _FakeProbe:
    """256 CUs; `bad[dev]` = [(xcc, key, kind, slot, thread)]: that CU fails that kind when it is selected."""

    def __init__(self, n=2, bad=None, cus=256):
        self.n, self.cus, self.bad = n, cus, bad or {}
        self.sweeps, self.valu_sweeps = [], []

    def device_count(self):
        return self.n

    def device_props(self, dev):
        return {"cus": self.cus}

    def mem_info(self, dev):
        return 200 * GIB, 288 * GIB

    def _keys(self, mask):
        return [(i % 8, i // 8) for i in range(self.cus) if not mask or (mask[i // 32] >> (i % 32)) & 1]

    def cu_sweep(self, dev, mask, rounds, seed, inject=None):
        self.sweeps.append((dev, list(mask), rounds))
        return {"records": [(x, _hw(k), 0, 0xF, -1) for x, k in self._keys(mask)], "lds_bytes": 163840, "ms": 0.25}

    def cu_sweep_valu(self, dev, mask, rounds, seed, groups, inject=None, corrupt_expected=None):
        self.valu_sweeps.append((dev, list(mask), rounds, list(groups)))
        keys = self._keys(mask)
        recs = _clean(keys)
        for x, k, kind, slot, thread in self.bad.get(dev, ()):
            if kind in groups and (x, k) in keys:
                if kind == "regs":
                    recs.append(_rec(x, k, fail=0x10 << (thread >> 6), slot=slot, thread=thread))
                else:
                    recs.append(_rec(x, k, fail=1, gbits=1 << V.GROUPS.index(kind)))
        return {"records": recs, "groups": list(V.GROUPS), "checked": list(groups), "reg_slots": 448, "regs_per_lane": 512,
                "scratch_bytes": 0, "ms": 0.5}

    def hbm_pattern_check(self, dev, nbytes, seed, passes=2, corrupt=(), verify_seed=None, cu_mask=None):
        return {"bytes": nbytes, "errors": 0, "first": [], "fill_gbs": 5000.0, "verify_gbs": 6000.0}


class _OldProbe(_FakeProbe):
    cu_sweep_valu = property()        # hasattr() is False


def test_deep_selftest_with_valu():
    P = _FakeProbe()
    rep = S.deep_selftest(P, 0, valu="all", seed=1)
    assert rep.ok and rep.valu["checked"] == list(V.GROUPS) and rep.valu["failed"] == {} and rep.valu["reg_slots"] == 448
    assert len(P.sweeps) == 1 and [v[3] for v in P.valu_sweeps] == [list(V.GROUPS)] and P.valu_sweeps[0][1] == P.sweeps[0][1]
    assert set(rep.to_dict()["valu"]) == {"checked", "failed", "cus", "reg_slots", "ms"}
    bad = _FakeProbe(bad={0: [(3, 17, "regs", 255, 1 << 6 | 5)]})
    rep = S.deep_selftest(bad, 0, valu="all", seed=1)
    assert not rep.ok and rep.valu["failed"] == {"regs": [[3, 17]]} and rep.sweep["failed"] == []
    assert S.failed_cus(rep) == {(3, 17)} and S.fenceable(rep)
    text = rep.describe_failure()
    assert "regs" in text and "xcc 3" in text and "slot 255" in text and "wave 1 lane 5" in text
    assert S.deep_selftest(bad, 0, valu="fma32,cvt", seed=1).ok                     # the bad kind is not asked for
    rep = S.deep_selftest(_FakeProbe(bad={0: [(1, 2, "cvt", -1, -1)]}), 0, valu="cvt", seed=1)
    assert not rep.ok and "cvt" in rep.describe_failure() and S.fenceable(rep)


def test_a_garbled_valu_record_is_not_fenceable():
    class Garbled(_FakeProbe):
        def cu_sweep_valu(self, *a, **kw):
            out = super().cu_sweep_valu(*a, **kw)
            out["records"].append(_rec(0, 0, fail=0x10000))
            return out

    rep = S.deep_selftest(Garbled(), 0, valu="all", seed=1)
    assert not rep.ok and "record" in rep.valu["failed"] and not S.fenceable(rep)


def test_without_valu_nothing_changes():
    P = _FakeProbe()
    rep = S.deep_selftest(P, 0, seed=1)
    assert rep.ok and rep.valu is None and P.valu_sweeps == []
    assert sorted(rep.to_dict()) == sorted(["device", "ok", "seconds", "sweep", "hbm", "error", "masked", "seed", "notes", "paths"])
    for spec in (None, "", []):
        assert S.deep_selftest(P, 0, valu=spec, seed=1).valu is None
    assert P.valu_sweeps == []


def test_an_older_probe_gets_a_note():
    P = _OldProbe()
    assert not hasattr(P, "cu_sweep_valu")
    rep = S.deep_selftest(P, 0, valu="all", seed=1)
    assert rep.ok and rep.valu is None and any("no cu_sweep_valu" in n for n in rep.notes)
    assert not S.deep_selftest(_FakeProbe(), 0, valu="all", seed=1).notes


def test_localise_failure_passes_valu():
    P = _FakeProbe(bad={0: [(3, 17, "regs", 0, 0)]})
    rep = S.deep_selftest(P, 0, valu="regs", seed=1)
    P.valu_sweeps.clear()
    loc = S.localise_failure(P, 0, rep, range(32), 8, valu=["regs"])
    assert loc.bad_units == [17] and loc.unexplained == []
    assert len(P.valu_sweeps) == 32 and all(v[3] == ["regs"] for v in P.valu_sweeps)
    plan = S.would_fence(P, 0, rep, 1, valu=["regs"])
    assert plan["units"] == [17] and [3, 17] in plan["cus"]["17"]


def test_the_agents_fence_run_carries_valu():
    """--selftest-fence with --selftest-valu: a CU with a bad register file is localised with the valu part,
    its unit fenced, and the verification without the unit passes: as for a matrix-path failure."""
    from nanogpu.agent.plugin import NanoGpuPlugin

    async def main():
        store = FakeKubeStore()
        topo = synthetic_mi355x(1)
        store.add_node(pu.make_node("n0", 1, topo.to_json()))
        api = InProcKube(store)
        agent = NodeAgent(api, "n0", topo, device_plugin=False, health_period_s=0, selftest_hbm_mib=64,
                          selftest_fence=1, selftest_valu="regs,fma32")
        agent.plugin = NanoGpuPlugin(topo, api, "n0")
        P = _FakeProbe(1, bad={0: [(3, 17, "regs", 447, 2 << 6 | 9)]})
        assert await agent.selftest(P) == []
        assert agent.selftest_failed == set() and agent.topo.devices[0].healthy
        assert agent.topo.devices[0].fenced == [17] and agent.plugin.cus[0].fenced == {17}
        assert agent.selftest_stats["runs"] == {(0, "fenced"): 1}
        rep = agent.selftest_stats["reports"][0]
        assert rep["valu"]["checked"] == ["fma32", "regs"] and rep["valu"]["failed"] == {}
        assert any("slot 447" in n and "wave 2 lane 9" in n for n in rep["notes"])
        # the first sweep, 32 units swept alone, the verification: each with its valu launch on the same mask
        assert len(P.valu_sweeps) == len(P.sweeps) == 34 and all(v[3] == ["fma32", "regs"] for v in P.valu_sweeps)
        assert [v[1] for v in P.valu_sweeps] == [s[1] for s in P.sweeps]
        last = [i for i in range(256) if (P.valu_sweeps[-1][1][i // 32] >> (i % 32)) & 1]
        assert last == [b for b in range(256) if b // 8 != 17]
        # without the valu flag the same probe passes: the fault is in a unit only --selftest-valu tests
        plain = NodeAgent(api, "n0", synthetic_mi355x(1), device_plugin=False, health_period_s=0, selftest_fence=1)
        plain.plugin = NanoGpuPlugin(plain.topo, api, "n0")
        Q = _FakeProbe(1, bad={0: [(3, 17, "regs", 447, 9)]})
        assert await plain.selftest(Q) == [] and Q.valu_sweeps == [] and plain.topo.devices[0].fenced == []

    asyncio.run(main())


def test_cli_rejects_an_unknown_group():
    with pytest.raises(SystemExit) as e:
        S.main(["--valu", "fma32,nope"])
    assert e.value.code == 2


# ----------------------------------------------------------------------------- agent, flag, metrics
def _agent(n=2, **kw):
    store = FakeKubeStore()
    topo = synthetic_mi355x(n)
    store.add_node(pu.make_node("n0", n, topo.to_json()))
    return NodeAgent(InProcKube(store), "n0", topo, device_plugin=False, health_period_s=0, **kw), store


def test_flag_parses_and_implies_deep(capsys):
    ap = build_parser()
    a = ap.parse_args(["--node-name", "n", "--selftest-valu", "regs,fma32"])
    assert a.selftest and a.selftest_deep and a.selftest_valu == ["fma32", "regs"]
    assert ap.parse_args(["--selftest-valu", "all"]).selftest_valu == list(V.GROUPS)
    assert ap.parse_args(["--node-name", "n", "--selftest-deep"]).selftest_valu == []     # the default is off
    for bad in ("fma32,fma33", ""):
        with pytest.raises(SystemExit) as e:
            ap.parse_args(["--selftest-valu", bad])
        assert e.value.code == 2
    assert "unknown vector-ALU group" in capsys.readouterr().err
    assert NodeAgent(None, "n", synthetic_mi355x(1), device_plugin=False, selftest_valu="regs").selftest_deep
    assert not NodeAgent(None, "n", synthetic_mi355x(1), device_plugin=False).selftest_parts.valu


def test_agent_marks_the_device_unhealthy_and_renders_the_metric():
    async def main():
        agent, _ = _agent(2, selftest_valu="all", selftest_hbm_mib=64)
        await agent.start()
        P = _FakeProbe(2, bad={1: [(3, 17, "regs", 447, 3 << 6 | 1)]})
        assert await agent.selftest(P) == [1]
        assert [d.healthy for d in agent.topo.devices] == [True, False]
        assert agent.selftest_stats["reports"][1]["valu"]["failed"] == {"regs": [[3, 17]]}
        text = render_metrics(agent.topo, None, None, "/nonexistent", agent.selftest_stats)
        for line in ('nanogpu_selftest_valu_checked{device="0"} 13', 'nanogpu_selftest_valu_checked{device="1"} 13',
                     "# TYPE nanogpu_selftest_valu_checked gauge"):
            assert line in text.splitlines(), line
        plain, _ = _agent(2, selftest_deep=True)
        await plain.start()
        Q = _FakeProbe(2, bad={1: [(3, 17, "regs", 447, 1)]})
        assert await plain.selftest(Q) == [] and Q.valu_sweeps == []                  # without the flag: today's kernels only
        assert "valu" not in plain.selftest_stats["reports"][0]
        assert "nanogpu_selftest_valu" not in render_metrics(plain.topo, None, None, "/nonexistent", plain.selftest_stats)
        for a in (agent, plain):
            await a.stop()

    asyncio.run(main())
