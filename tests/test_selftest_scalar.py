"""Scalar part of the deep self-test, without a GPU: the host header's stand-alone program against
the Python twin, the twin's own conditions and hand-derived values, parsing, folding,
deep_selftest over a fake probe, fencing, the agent's flag and the metric."""
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
from nanogpu.probe import selftest_scalar as V
from nanogpu.topology.model import synthetic_mi355x

GIB = 1 << 30
M32 = 0xFFFFFFFF
ALL = [(x, k) for x in range(8) for k in range(32)]


def _hw(key, simd=0):
    return (key << 8) | (simd << 4)


def _rec(x, k, fail=0, gbits=0, index=-1, wave=-1, which=-1):
    return (x, _hw(k), fail, 0xF, gbits, index, wave, which)


def _clean(keys=ALL):
    return [_rec(x, k) for x, k in keys]


# ----------------------------------------------------------------------------- host program and twin
@pytest.mark.parametrize("kind", ["plain", "asan"])
def test_host_program_agrees_with_the_twin(kind):
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "native"))
    import build  # native/build.py

    exe = build.build_selftest_host(kind, target="scalar")
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr          # the program asserts the header's conditions itself
    host = json.loads(r.stdout)
    twin = V.twin_summary()
    assert list(host["groups"]) == list(V.EXACT_GROUPS)
    for g in V.EXACT_GROUPS:
        assert host["groups"][g] == twin["groups"][g], g
    assert host["smem_checksum"] == twin["smem_checksum"] and host["smem_words"] == V.SMEM_WORDS == 4096
    assert host["sreg_slots"] == V.SREG_SLOTS == 88 and host["record_words"] == V.RECORD_WORDS


def test_twin_conditions_hold():
    scc: dict[str, list[int]] = {}
    for g in V.EXACT_GROUPS:
        words, c = V.group_expected(g)
        assert len(words) == 32 and V.uncovered_bits(words) == 0, g       # every bit is 0 in some word and 1 in another
        for name, (zero, one) in c.scc.items():
            scc[name] = [scc.get(name, [0, 0])[0] + zero, scc.get(name, [0, 0])[1] + one]
    assert len(scc) == 80 and all(zero > 0 and one > 0 for zero, one in scc.values()), \
        {n: v for n, v in scc.items() if 0 in v}                          # every SCC consumed as 0 and as 1
    c = V.group_expected("add")[1]
    for taken in (0, 1):                                                   # across bit 31 and out of bit 63, both ways
        assert min(c.carry31[taken], c.carry63[taken], c.borrow31[taken], c.borrow63[taken]) > 0
    assert c.overflow_pos > 0 and c.overflow_neg > 0
    assert {V.shift_amount32(s, 0x12345678) for s in range(8)} >= {0, 1, 31}
    assert {V.shift_amount64(s, 0x12345678) for s in range(8)} >= {0, 31, 32, 63}
    c = V.group_expected("cmp")[1]
    assert c.equal_operands > 0
    for name in list(V.CMP32) + list(V.CMP64):                             # true and false, through the select and the branch
        assert all(min(c.scc[f"{how}_{name}"]) > 0 for how in ("sel", "br")), name
    for u in range(0, 1 << 32, 0x01010101 * 3 + 7):                        # extracts stay inside the operand
        f32, f64 = V.bfe_field32(u), V.bfe_field64(u)
        assert f32 >> 16 >= 1 and (f32 & 31) + (f32 >> 16) <= 32 and f64 >> 16 >= 1 and (f64 & 63) + (f64 >> 16) <= 64
    table = [V.smem_word(i) for i in range(V.SMEM_WORDS)]
    assert all(table[i] != table[i ^ (1 << b)] for i in range(V.SMEM_WORDS) for b in range(12))   # every address line matters
    for wave in range(4):
        for p in range(2):
            assert len({V.sreg_word(i, 0x5EED5EED ^ wave, p) for i in range(V.SREG_SLOTS)}) == V.SREG_SLOTS


def test_spot_values_by_hand_add_mul_shift():
    # s_add_u32: 0xffffffff + 1 wraps to 0 and carries; s_addc_u32 adds the carry in
    assert V.s_add_u32(M32, 1) == (0, 1) and V.s_add_u32(5, 6, cin=1) == (12, 0)
    # s_sub_u32: 0 - 1 borrows; s_subb_u32: 5 - 5 - 1 borrows too
    assert V.s_sub_u32(0, 1) == (M32, 1) and V.s_sub_u32(5, 5, bin_=1) == (M32, 1)
    # the pair: 0x0_ffffffff + 1: the low carry enters the high word, no carry out of bit 63
    assert V.add64(0xFFFFFFFF, 1) == (0x100000000, 0) and V.add64((1 << 64) - 1, 1) == (0, 1)
    assert V.sub64(0x100000000, 1) == (0xFFFFFFFF, 0) and V.sub64(0, 1) == ((1 << 64) - 1, 1)
    # signed overflow: 2^31 - 1 + 1 and -2^31 - 1 do not fit; -1 + 1 does
    assert V.s_add_i32(0x7FFFFFFF, 1) == (0x80000000, 1) and V.s_sub_i32(0x80000000, 1) == (0x7FFFFFFF, 1)
    assert V.s_add_i32(M32, 1) == (0, 0)
    # -1 is the signed minimum of (-1, 1) and S0, so SCC = 1; unsigned 0xffffffff is the maximum
    assert V.s_min_i32(M32, 1) == (M32, 1) and V.s_min_u32(M32, 1) == (1, 0)
    assert V.s_max_i32(M32, 1) == (1, 0) and V.s_max_u32(M32, 1) == (M32, 1)
    # |3 - (-5)| = 8; |-7| = 7; |0| = 0 with SCC 0
    assert V.s_absdiff_i32(3, 0xFFFFFFFB) == (8, 1) and V.s_abs_i32(0xFFFFFFF9) == (7, 1) and V.s_abs_i32(0) == (0, 0)
    # (2^32 - 1)^2 = 2^64 - 2^33 + 1: low word 1, high word 2^32 - 2; signed (-1)(-1) = 1: high word 0
    assert V.s_mul_i32(M32, M32) == 1 and V.s_mul_hi_u32(M32, M32) == 0xFFFFFFFE and V.s_mul_hi_i32(M32, M32) == 0
    assert V.s_mul_hi_i32(0x80000000, 2) == M32                           # -2^31 * 2 = -2^32: high word -1
    # (0x1fffffff << 3) + 8 = 2^32 - 8 + 8: wraps to 0 with a carry
    assert V.s_lshl_add_u32(3, 0x1FFFFFFF, 8) == (0, 1) and V.s_lshl_add_u32(1, 3, 4) == (10, 0)
    assert V.s_lshl(1, 31) == (0x80000000, 1) and V.s_lshl(2, 31) == (0, 0)            # the bit leaves: D = 0, SCC = 0
    assert V.s_lshr(0x80000000, 31) == (1, 1) and V.s_ashr(0x80000000, 31) == (M32, 1)  # zeros fill | the sign fills
    assert V.s_lshl(3, 63, 64) == (1 << 63, 1) and V.s_ashr(1 << 63, 63, 64) == ((1 << 64) - 1, 1)
    assert V.s_lshr(1 << 63, 32, 64) == (1 << 31, 1)
    # s_bfm: 4 ones at bit 8; 33 ones at bit 4
    assert V.s_bfm(4, 8) == 0xF00 and V.s_bfm(33, 4, 64) == 0x1FFFFFFFF0
    for corner in (lambda: V.s_lshl(1, 32), lambda: V.s_min_i32(4, 4), lambda: V.s_abs_i32(0x80000000),
                   lambda: V.s_lshl_add_u32(1, 0x80000000, 0)):
        with pytest.raises(ValueError, match="left out"):
            corner()


def test_spot_values_by_hand_logic_bits_cmp():
    # each of the eight on (0b1100, 0b1010), in 4 bits of 32: and 1000, or 1110, xor 0110, andn2 0100, orn2 ...11111101
    assert [V.s_logic(n, 0xC, 0xA)[0] for n in V.LOGIC] == [0x8, 0xE, 0x6, M32 ^ 0x8, M32 ^ 0xE, M32 ^ 0x6, 0x4, M32 ^ 0x2]
    assert V.s_logic("nand", M32, M32) == (0, 0) and V.s_logic("orn2", 0, (1 << 64) - 1, 64) == (0, 0)   # SCC = D != 0
    assert V.s_not(0, 64) == ((1 << 64) - 1, 1) and V.s_not(M32) == (0, 0)
    # 0xabcd1234: bits 4..11 are 0x23; bits 16..19 are 0xd = 1101b, signed -3
    assert V.s_bfe(0xABCD1234, 4 | 8 << 16) == (0x23, 1) and V.s_bfe(0xABCD1234, 16 | 4 << 16, 32, True) == (0xFFFFFFFD, 1)
    assert V.s_bfe(0xF << 40, 40 | 4 << 16, 64, True) == ((1 << 64) - 1, 1) and V.s_bfe(0xF << 40, 44 | 4 << 16, 64) == (0, 0)
    assert V.s_brev(1) == 0x80000000 and V.s_brev(2, 64) == 1 << 62
    assert V.s_bcnt(0xFFFFFFF0, 0) == (4, 1) and V.s_bcnt(0xF0000000F0, 1, 64) == (8, 1) and V.s_bcnt(0, 1) == (0, 0)
    assert V.s_ff(0x0000FFFF, 0) == 16 and V.s_ff(1 << 32, 1, 64) == 32
    # leading zeros of 0x00ff0000: 8. Signed: 0xff00ffff has 8 leading sign bits, 0x7fffffff one
    assert V.s_flbit(0x00FF0000) == 8 and V.s_flbit(0xFF00FFFF, 32, True) == 8 and V.s_flbit(0x7FFFFFFF, 32, True) == 1
    assert V.s_flbit(1, 64) == 63 and V.s_flbit((1 << 64) - 2, 64, True) == 63
    assert V.s_bitset(0xFF, 3, 0) == 0xF7 and V.s_bitset(0, 31, 1) == 0x80000000
    assert V.s_sext(0x1280, 8) == 0xFFFFFF80 and V.s_sext(0x12347FFF, 16) == 0x7FFF
    assert [V.s_pack(k, 0x11112222, 0x33334444) for k in ("ll", "lh", "hh")] == [0x44442222, 0x33332222, 0x33331111]
    # -1 > 1 is false signed, true unsigned; the bit number of s_bitcmp is S1[4:0]: 36 names bit 4
    assert V.s_cmp("gt_i32", M32, 1, 7, 8) == 8 and V.s_cmp("gt_u32", M32, 1, 7, 8) == 7
    assert V.s_cmp("bitcmp0_b32", 0x10, 4, 7, 8) == 8 and V.s_cmp("bitcmp1_b32", 0x10, 36, 7, 8, "br") == 7
    assert V.s_cmp("eq_u64", 1 << 32, 2 << 32, 7, 8) == 8 and V.s_cmp("le_i32", 5, 5, 7, 8) == 7
    with pytest.raises(ValueError, match="left out"):
        V.s_bfe(1, 30 | 4 << 16)                    # runs past the top bit
    with pytest.raises(ValueError, match="left out"):
        V.s_ff(M32, 0)                              # no zero to find


def test_spot_values_by_hand_vcc_fold_operand_and_patterns():
    # fold: rotl(h ^ d, 7) + c + 0x9e3779b9
    assert V.fold(0, 0, 0) == 0x9E3779B9 and V.fold(1, 0, 1) == 0x9E3779B9 + 129
    assert V.operand("add", 0, 0, 0) == C.mix32(0x5CA1A2B3) and V.operand("mul", 1, 2, 3) == C.mix32(0x5CA1A2B3 ^ 1 << 24 ^ 1 << 16 ^ 2 << 8 ^ 3)
    # vcc with thr = 0: no lane is below, mask = 0, count 0, the search finds the guard bit 63; m = 0: w = v ^ k with
    # k = 0 is v, never below 0, so mask2 = 0: the word folds (0, 0), (0, 63), v0 ^ h, (0, 0), (0, 0)
    h0, u0 = 0x1234, 0x77
    h = V.fold(V.fold(V.fold(h0, 0, 0), 0, 63), V.vcc_lane_value(u0, 0) ^ h0, 0)
    assert V.vcc_step(h0, u0, 0, 0, 0) == V.fold(V.fold(h, 0, 0), 0, 0)
    # thr = 2^32 - 1 and no lane value equal to it: all 64 lanes, the first at 0
    assert M32 not in [V.vcc_lane_value(u0, lane) for lane in range(64)]
    h = V.fold(V.fold(V.fold(h0, M32, 64), M32, 0), V.vcc_lane_value(u0, 0) ^ h0, 0)
    assert V.vcc_step(h0, u0, M32, 0, 0) == V.fold(V.fold(h, 0, 0), 0, 0)
    assert V.sreg_word(0, 1) == 0x9E3779B1 ^ 0x7F4A7C15 and V.sreg_word(3, 77, 1) == V.sreg_word(3, 77) ^ M32
    assert V.sreg_word(87, 2) == ((2 * (0x9E3779B1 + 174)) & M32) ^ ((0x7F4A7C15 + 87 * 0x01000193) & M32)
    assert V.smem_word(5) == C.mix32(5 ^ V.SMEM_SALT)


def test_parse_scalar():
    assert V.parse_scalar(None) == V.parse_scalar("") == V.parse_scalar([]) == []
    assert V.parse_scalar("all") == list(V.GROUPS) and len(V.GROUPS) == 9 and V.EXACT_GROUPS == V.GROUPS[:7]
    assert V.parse_scalar("sregs, add,cmp") == ["add", "cmp", "sregs"] == V.parse_scalar(["sregs", "cmp", "add"])   # bit order
    with pytest.raises(ValueError, match="unknown scalar group"):
        V.parse_scalar("add,sub")


# ----------------------------------------------------------------------------- fold_scalar
def test_fold_clean_and_uncovered_is_no_failure():
    f = V.fold_scalar(_clean(), V.GROUPS, 256)
    assert f["failed"] == {} and f["cus"] == [] and f["cus_seen"] == 256 and f["cus_uncovered"] == 0 and f["simds_seen_min"] == 4
    f = V.fold_scalar(_clean(ALL[:250]), V.GROUPS, set(ALL))
    assert f["failed"] == {} and f["cus_uncovered"] == 6 and f["uncovered"] == [list(k) for k in ALL[250:]]


def test_fold_one_failing_cu_per_kind():
    cmp_bit = 1 << V.GROUPS.index("cmp")
    f = V.fold_scalar(_clean() + [_rec(5, 9, fail=0b1010, gbits=cmp_bit)] + _clean([(5, 9)]), V.GROUPS, 256)
    assert f["failed"] == {"cmp": [[5, 9]]}                                # a clean revisit clears nothing
    assert f["cus"] == [{"xcc": 5, "cu_key": 9, "kinds": ["cmp"], "waves": 0b1010, "bad_slot": -1, "bad_slot_wave": -1,
                         "bad_word": -1, "bad_word_wave": -1}]
    f = V.fold_scalar(_clean() + [_rec(2, 3, fail=0x400, index=40, wave=2, which=0), _rec(2, 3, fail=0x100, index=17, wave=0, which=0)],
                      V.GROUPS, 256)
    assert f["failed"] == {"sregs": [[2, 3]]}
    assert (f["cus"][0]["bad_slot"], f["cus"][0]["bad_slot_wave"], f["cus"][0]["waves"], f["cus"][0]["bad_word"]) == (17, 0, 0b101, -1)
    f = V.fold_scalar(_clean() + [_rec(7, 31, fail=0x80, index=4095, wave=3, which=1)], V.GROUPS, 256)
    assert f["failed"] == {"smem": [[7, 31]]}
    assert (f["cus"][0]["bad_word"], f["cus"][0]["bad_word_wave"], f["cus"][0]["waves"], f["cus"][0]["bad_slot"]) == (4095, 3, 0b1000, -1)


def test_fold_garbled_record():
    for bad in (_rec(4, 4, fail=0x1000), _rec(4, 4, fail=1, gbits=0), _rec(4, 4, fail=1, gbits=1 << 8),
                _rec(4, 4, fail=0x100), _rec(4, 4, index=3, wave=0, which=0), _rec(4, 4, fail=0x10, index=3, wave=0, which=0)):
        assert "record" in V.fold_scalar(_clean() + [bad], V.GROUPS, 256)["failed"], bad


# ----------------------------------------------------------------------------- deep_selftest over a fake probe
class _FakeProbe:
    """256 CUs; `bad[dev]` = [(xcc, key, kind, index, wave)]: that CU fails that kind when it is selected."""

    def __init__(self, n=2, bad=None, cus=256):
        self.n, self.cus, self.bad = n, cus, bad or {}
        self.calls = []                  # ("sweep" | "valu" | "scalar", dev, mask, rounds[, names])

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

    def cu_sweep_valu(self, dev, mask, rounds, seed, groups, inject=None, corrupt_expected=None):
        self.calls.append(("valu", dev, list(mask), rounds, list(groups)))
        return {"records": [(x, _hw(k), 0, 0xF, 0, -1, -1, 7) for x, k in self._keys(mask)], "groups": list(groups),
                "checked": list(groups), "reg_slots": 448, "regs_per_lane": 512, "scratch_bytes": 0, "ms": 0.5}

    def cu_sweep_scalar(self, dev, mask, rounds, seed, groups, inject=None, corrupt_expected=None):
        self.calls.append(("scalar", dev, list(mask), rounds, list(groups)))
        keys = self._keys(mask)
        recs = _clean(keys)
        for x, k, kind, index, wave in self.bad.get(dev, ()):
            if kind in groups and (x, k) in keys:
                if kind in ("sregs", "smem"):
                    recs.append(_rec(x, k, fail=(0x100 if kind == "sregs" else 0x10) << wave, index=index, wave=wave,
                                     which=0 if kind == "sregs" else 1))
                else:
                    recs.append(_rec(x, k, fail=1, gbits=1 << V.GROUPS.index(kind)))
        return {"records": recs, "groups": list(V.GROUPS), "checked": list(groups), "sreg_slots": 88, "num_regs": 16,
                "scratch_bytes": 0, "ms": 0.3}

    def hbm_pattern_check(self, dev, nbytes, seed, passes=2, corrupt=(), verify_seed=None, cu_mask=None):
        return {"bytes": nbytes, "errors": 0, "first": [], "fill_gbs": 5000.0, "verify_gbs": 6000.0}

    def scalar_calls(self):
        return [c for c in self.calls if c[0] == "scalar"]


class _OldProbe(_FakeProbe):
    cu_sweep_scalar = property()        # hasattr() is False


def test_the_scalar_launch_follows_each_sweep_launch_on_the_same_mask():
    P = _FakeProbe()
    rep = S.deep_selftest(P, 0, scalar="all", seed=1)
    assert rep.ok and rep.scalar["checked"] == list(V.GROUPS) and rep.scalar["failed"] == {} and rep.scalar["sreg_slots"] == 88
    assert [c[0] for c in P.calls] == ["sweep", "scalar"] and P.calls[0][2:4] == P.calls[1][2:4]
    assert set(rep.to_dict()["scalar"]) == {"checked", "failed", "cus", "sreg_slots", "ms"}
    P = _FakeProbe()
    S.deep_selftest(P, 0, cu_mask_bits=list(range(40, 48)), valu="fma32", scalar="add,smem", seed=1)
    assert [c[0] for c in P.calls] == ["sweep", "valu", "scalar"] and P.calls[2][4] == ["add", "smem"]   # after the vector launch
    assert P.calls[0][2] == P.calls[1][2] == P.calls[2][2] != []

    class Shy(_FakeProbe):                 # the first two launches miss a CU: the coverage loop runs three times
        def cu_sweep(self, dev, mask, rounds, seed, inject=None):
            out = super().cu_sweep(dev, mask, rounds, seed)
            if rounds < 16:
                out["records"] = out["records"][1:]
            return out

    P = Shy()
    rep = S.deep_selftest(P, 0, scalar="cmp", seed=1)
    assert [c[0] for c in P.calls] == ["sweep", "scalar"] * 3 and [c[3] for c in P.calls] == [4, 4, 8, 8, 16, 16] and rep.ok


def test_ok_is_false_exactly_when_a_scalar_kind_failed():
    bad = _FakeProbe(bad={0: [(3, 17, "sregs", 87, 2)]})
    rep = S.deep_selftest(bad, 0, scalar="all", seed=1)
    assert not rep.ok and rep.scalar["failed"] == {"sregs": [[3, 17]]} and rep.sweep["failed"] == []
    assert S.failed_cus(rep) == {(3, 17)} and S.fenceable(rep)
    text = rep.describe_failure()
    assert "scalar unit sregs on CU (xcc 3, key 0x11), at slot 87, wave 2" in text
    assert S.deep_selftest(bad, 0, scalar="add,smem", seed=1).ok                   # the bad kind is not asked for
    rep = S.deep_selftest(_FakeProbe(bad={0: [(1, 2, "smem", 4095, 3)]}), 0, scalar="smem", seed=1)
    assert not rep.ok and "scalar unit smem on CU (xcc 1, key 0x2), at word 4095, wave 3" in rep.describe_failure() and S.fenceable(rep)
    rep = S.deep_selftest(_FakeProbe(bad={0: [(1, 2, "vcc", -1, -1)]}), 0, scalar="vcc", seed=1)
    assert not rep.ok and rep.scalar["failed"] == {"vcc": [[1, 2]]} and "scalar unit vcc" in rep.describe_failure()


def test_a_garbled_scalar_record_is_not_fenceable():
    class Garbled(_FakeProbe):
        def cu_sweep_scalar(self, *a, **kw):
            out = super().cu_sweep_scalar(*a, **kw)
            out["records"].append(_rec(0, 0, fail=0x1000))
            return out

    rep = S.deep_selftest(Garbled(), 0, scalar="all", seed=1)
    assert not rep.ok and "record" in rep.scalar["failed"] and not S.fenceable(rep)


def test_without_scalar_nothing_changes():
    P = _FakeProbe()
    rep = S.deep_selftest(P, 0, seed=1)
    assert rep.ok and rep.scalar is None and P.scalar_calls() == []
    assert sorted(rep.to_dict()) == sorted(["device", "ok", "seconds", "sweep", "hbm", "error", "masked", "seed", "notes", "paths"])
    for spec in (None, "", []):
        assert S.deep_selftest(P, 0, scalar=spec, valu="all", seed=1).scalar is None
    assert P.scalar_calls() == []
    assert sorted(S.deep_selftest(P, 0, valu="all", seed=1).to_dict()) == sorted(
        ["device", "ok", "seconds", "sweep", "hbm", "error", "masked", "seed", "notes", "paths", "valu"])


def test_an_older_probe_gets_a_note():
    P = _OldProbe()
    assert not hasattr(P, "cu_sweep_scalar")
    rep = S.deep_selftest(P, 0, scalar="all", seed=1)
    assert rep.ok and rep.scalar is None and "scalar" not in rep.to_dict() and any("no cu_sweep_scalar" in n for n in rep.notes)
    assert not S.deep_selftest(_FakeProbe(), 0, scalar="all", seed=1).notes


def test_localise_failure_and_would_fence_pass_scalar():
    P = _FakeProbe(bad={0: [(3, 17, "sregs", 0, 0)]})
    rep = S.deep_selftest(P, 0, scalar="sregs", seed=1)
    P.calls.clear()
    loc = S.localise_failure(P, 0, rep, range(32), 8, scalar=["sregs"])
    assert loc.bad_units == [17] and loc.unexplained == []
    assert len(P.scalar_calls()) == 32 and all(c[4] == ["sregs"] for c in P.scalar_calls())
    plan = S.would_fence(P, 0, rep, 1, scalar=["sregs"])
    assert plan["units"] == [17] and [3, 17] in plan["cus"]["17"]
    assert S.would_fence(P, 0, rep, 1)["units"] == []                      # without the part nothing fails again


def test_the_agents_fence_run_carries_scalar():
    from nanogpu.agent.plugin import NanoGpuPlugin

    async def main():
        store = FakeKubeStore()
        topo = synthetic_mi355x(1)
        store.add_node(pu.make_node("n0", 1, topo.to_json()))
        api = InProcKube(store)
        agent = NodeAgent(api, "n0", topo, device_plugin=False, health_period_s=0, selftest_hbm_mib=64,
                          selftest_fence=1, selftest_scalar="sregs,add")
        agent.plugin = NanoGpuPlugin(topo, api, "n0")
        P = _FakeProbe(1, bad={0: [(3, 17, "sregs", 87, 2)]})
        assert await agent.selftest(P) == []
        assert agent.topo.devices[0].healthy and agent.topo.devices[0].fenced == [17] and agent.plugin.cus[0].fenced == {17}
        rep = agent.selftest_stats["reports"][0]
        assert rep["scalar"]["checked"] == ["add", "sregs"] and rep["scalar"]["failed"] == {}
        assert any("at slot 87, wave 2" in n for n in rep["notes"])
        # the first sweep, 32 units swept alone, the verification: each with its scalar launch on the same mask
        sweeps = [c for c in P.calls if c[0] == "sweep"]
        assert len(P.scalar_calls()) == len(sweeps) == 34 and all(c[4] == ["add", "sregs"] for c in P.scalar_calls())
        assert [c[2] for c in P.scalar_calls()] == [c[2] for c in sweeps]

    asyncio.run(main())


def test_cli_rejects_an_unknown_group():
    with pytest.raises(SystemExit) as e:
        S.main(["--scalar", "add,nope"])
    assert e.value.code == 2


# ----------------------------------------------------------------------------- agent, flag, metrics
def _agent(n=2, **kw):
    store = FakeKubeStore()
    topo = synthetic_mi355x(n)
    store.add_node(pu.make_node("n0", n, topo.to_json()))
    return NodeAgent(InProcKube(store), "n0", topo, device_plugin=False, health_period_s=0, **kw), store


def test_flag_parses_and_implies_deep(capsys):
    ap = build_parser()
    a = ap.parse_args(["--node-name", "n", "--selftest-scalar", "sregs,add"])
    assert a.selftest and a.selftest_deep and a.selftest_scalar == ["add", "sregs"]
    assert ap.parse_args(["--selftest-scalar", "all"]).selftest_scalar == list(V.GROUPS)
    assert ap.parse_args(["--node-name", "n", "--selftest-deep"]).selftest_scalar == []     # the default is off
    for bad in ("add,sub", ""):
        with pytest.raises(SystemExit) as e:
            ap.parse_args(["--selftest-scalar", bad])
        assert e.value.code == 2
    assert "unknown scalar group" in capsys.readouterr().err
    agent = NodeAgent(None, "n", synthetic_mi355x(1), device_plugin=False, selftest_scalar="sregs")
    assert agent.selftest_deep and agent.selftest_parts.scalar == ["sregs"]
    assert not NodeAgent(None, "n", synthetic_mi355x(1), device_plugin=False).selftest_parts.scalar


def test_agent_marks_the_device_unhealthy_and_renders_the_metric():
    async def main():
        agent, _ = _agent(2, selftest_scalar="all", selftest_hbm_mib=64)
        await agent.start()
        P = _FakeProbe(2, bad={1: [(3, 17, "smem", 1024, 1)]})
        assert await agent.selftest(P) == [1]
        assert [d.healthy for d in agent.topo.devices] == [True, False]
        assert agent.selftest_stats["reports"][1]["scalar"]["failed"] == {"smem": [[3, 17]]}
        text = render_metrics(agent.topo, None, None, "/nonexistent", agent.selftest_stats)
        for line in ('nanogpu_selftest_scalar_checked{device="0"} 9', 'nanogpu_selftest_scalar_checked{device="1"} 9',
                     "# TYPE nanogpu_selftest_scalar_checked gauge"):
            assert line in text.splitlines(), line
        plain, _ = _agent(2, selftest_deep=True)
        await plain.start()
        Q = _FakeProbe(2, bad={1: [(3, 17, "smem", 1024, 1)]})
        assert await plain.selftest(Q) == [] and Q.scalar_calls() == []              # without the flag: today's kernels only
        assert "scalar" not in plain.selftest_stats["reports"][0]
        assert "nanogpu_selftest_scalar" not in render_metrics(plain.topo, None, None, "/nonexistent", plain.selftest_stats)
        for a in (agent, plain):
            await a.stop()

    asyncio.run(main())
