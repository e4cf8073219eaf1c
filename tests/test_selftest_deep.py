"""Deep self-test without a GPU: the folding of sweep records, the host twin of the HBM
pattern, and the node agent's start-up, periodic, metrics and flag paths over a fake probe."""
import asyncio
import subprocess
import sys
from pathlib import Path

import pytest

from nanogpu import types as T
from nanogpu.agent import cumask
from nanogpu.agent.metrics import render as render_metrics
from nanogpu.agent.node import NodeAgent, build_parser
from nanogpu.agent.plugin import Assignment, NanoGpuPlugin
from nanogpu.k8s import podutil as pu
from nanogpu.k8s.fake_apiserver import FakeKubeStore, InProcKube
from nanogpu.probe import selftest as S
from nanogpu.probe import selftest_common as C
from nanogpu.topology.model import NodeTopology, synthetic_mi355x

GIB = 1 << 30


def _hw(key: int, simd: int = 0) -> int:
    return (key << 8) | (simd << 4)


def _records(keys, simds=(0, 1, 2, 3)):
    simd_bits = sum(1 << s for s in simds)
    return [(x, _hw(k, simds[0]), 0, simd_bits, -1) for x, k in keys]


ALL = [(x, k) for x in range(8) for k in range(32)]


# ----------------------------------------------------------------------------- fold_sweep
def test_fold_full_coverage():
    rep = S.fold_sweep(_records(ALL) + _records(ALL[:40]), ALL)       # revisits fold into one CU
    assert rep["cus_seen"] == rep["cus_expected"] == 256
    assert rep["per_xcd"] == {x: 32 for x in range(8)}
    assert rep["failed"] == [] and rep["uncovered"] == [] and rep["cus_uncovered"] == 0
    assert rep["simds_seen_min"] == 4


def test_fold_one_failed_cu_with_kinds_decoded():
    recs = _records(ALL)
    recs.append((3, _hw(17), 0b00100, 0xF, -1))                       # wave 2's MFMA, one visit out of two
    recs.append((5, _hw(2), S.FAIL_LDS, 0xF, 40959))
    recs.append((5, _hw(2), S.FAIL_LDS | 1, 0xF, 12))                 # the lowest bad dword is kept
    rep = S.fold_sweep(recs, 256)
    assert rep["failed"] == [{"xcc": 3, "cu_key": 17, "kinds": ["mfma"], "lds_bad_off": -1},
                             {"xcc": 5, "cu_key": 2, "kinds": ["mfma", "lds"], "lds_bad_off": 12}]
    assert rep["cus_seen"] == 256 and rep["cus_uncovered"] == 0


def test_fold_missing_cu_is_uncovered_not_failed():
    rep = S.fold_sweep(_records([c for c in ALL if c != (6, 9)], simds=(1, 3)), ALL)
    assert rep["failed"] == []
    assert rep["uncovered"] == [[6, 9]] and rep["cus_uncovered"] == 1
    assert rep["cus_seen"] == 255 and rep["per_xcd"][6] == 31
    assert rep["simds_seen_min"] == 2
    by_count = S.fold_sweep(_records([c for c in ALL if c != (6, 9)]), 256)   # keys unknown: the count alone
    assert by_count["uncovered"] == [] and by_count["cus_uncovered"] == 1 and by_count["failed"] == []


def test_fold_masked_expectation():
    mine = [(x, k) for x in range(8) for k in range(8)]               # a 25 % grant: 8 CUs on each XCD
    rep = S.fold_sweep(_records(mine), mine)
    assert rep["cus_seen"] == rep["cus_expected"] == 64 and rep["uncovered"] == []
    assert rep["per_xcd"] == {x: 8 for x in range(8)}
    # a CU outside the expectation is seen and counted, and never "uncovered"
    rep = S.fold_sweep(_records(mine + [(0, 30)]), mine)
    assert rep["cus_seen"] == 65 and rep["cus_uncovered"] == 0


# ----------------------------------------------------------------------------- pattern twin
PINS = [((0, 0, 0, 0), 0x00000000), ((0, 3, 0x1234ABCD, 0), 0x00D1E6CC), ((4095, 1, 0x1234ABCD, 1), 0x72A42E3D),
        (((1 << 30), 2, 7, 0), 0x523A2A7C), (((1 << 32) + 5, 0, 0x1234ABCD, 0), 0x47FE4BAD),
        (((1 << 32) + 5, 0, 0x1234ABCD, 1), 0xB801B452), (((1 << 34) + 123456789, 3, 0xFFFFFFFF, 2), 0x71CA6542)]


def test_pattern_twin_pins():
    assert C.mix32(1) == 0x514E28B7                                   # murmur3's finaliser
    for args, want in PINS:
        assert S.pattern_word(*args) == want, args
    for i in (0, 77, (1 << 33) + 1):
        for k in range(4):
            assert S.pattern_word(i, k, 9, 1) == S.pattern_word(i, k, 9, 0) ^ 0xFFFFFFFF
            assert S.pattern_word(i, k, 9, 2) == S.pattern_word(i, k, 9, 0)
    # the value depends on the whole address: words 16 GiB apart share their low index bits only
    assert S.pattern_word(5, 1, 3) != S.pattern_word(5 + (1 << 30), 1, 3)
    assert S.pattern_at(16 * 4095 + 7, 0x1234ABCD, 1) == 0x72A42E3D


@pytest.mark.parametrize("off", [5, 4095 * 16 + 7, (1 << 36) + 12345])
def test_pattern_differs_across_every_address_line(off):
    """The aliasing claim, for every line: a word and the word at the address with bit b flipped
    differ, in both passes. Bits 2..33 flip the low half of the word index (mix32 is a bijection),
    bits 34..47 the high half (HI_MUL is odd)."""
    seed = 0x1234ABCD
    for b in range(2, 48):
        for p in (0, 1):
            assert S.pattern_at(off, seed, p) != S.pattern_at(off ^ (1 << b), seed, p), (off, b, p)


def test_native_header_agrees_with_the_twin():
    """The kernels take the pattern, the launch spans, the expected tile and the record decode from
    native/include/nanogpu/selftest_host.h; its stand-alone check pins the same values and
    checks the spans."""
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "native"))
    import build  # native/build.py

    exe = build.build_selftest_host("plain")
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    src = (Path(build.NATIVE) / "tests" / "selftest_host_main.cpp").read_text().lower()
    for _, want in PINS[1:]:
        assert f"0x{want:08x}u" in src


def test_host_program_passes_under_asan_and_ubsan():
    """The same stand-alone program, launch spans up to 304 GiB included, under ASan + UBSan."""
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "native"))
    import build  # native/build.py

    r = subprocess.run([str(build.build_selftest_host("asan"))], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "selftest host arithmetic ok" in r.stdout


# ----------------------------------------------------------------------------- fake probe
class _FakeDeepProbe:
    """Stands in for nanogpu._probe with the deep bindings. Mask bit i is CU (i % 8, i // 8), as
    measured on the chip. `bad_cus[dev]` = [(xcc, key, fail_bits, lds_off)], `hbm_errors[dev]`,
    `hidden[dev]` = CUs no workgroup ever lands on. The basic checks pass everywhere."""

    def __init__(self, n=8, cus=256, bad_cus=None, hbm_errors=None, hidden=None, free=200 * GIB, raises=()):
        self.n, self.cus, self.cur = n, cus, 0
        self.bad_cus, self.hbm_errors, self.hidden = bad_cus or {}, hbm_errors or {}, hidden or {}
        self.free, self.raises = free, set(raises)
        self.sweeps, self.hbm_calls, self.basic_calls = [], [], []

    def device_count(self):
        return self.n

    def device_props(self, dev):
        return {"cus": self.cus}

    def mem_info(self, dev):
        return self.free, 288 * GIB

    def copy_check(self, dev, n_floats):
        self.cur = dev
        self.basic_calls.append(dev)
        return True

    def gemm_tile(self, a, b):
        return [sum(a[r * 16 + k] * b[k * 32 + col] for k in range(16)) for r in range(32) for col in range(32)]

    def cu_sweep(self, dev, mask, rounds, seed, inject=None):
        if dev in self.raises:
            raise RuntimeError("hipErrorLaunchFailure")
        self.sweeps.append((dev, list(mask), rounds))
        bits = [i for i in range(self.cus) if not mask or (mask[i // 32] >> (i % 32)) & 1]
        keys = [(i % 8, i // 8) for i in bits if (i % 8, i // 8) not in self.hidden.get(dev, ())]
        recs = _records(keys)
        for x, k, fail, off in self.bad_cus.get(dev, ()):
            recs.append((x, _hw(k), fail, 0xF, off))
        return {"records": recs, "lds_bytes": 163840, "ms": 0.25}

    def hbm_pattern_check(self, dev, nbytes, seed, passes=2, corrupt=(), verify_seed=None):
        self.hbm_calls.append((dev, nbytes))
        e = self.hbm_errors.get(dev, 0)
        first = [(4096 * 16, 0x11, 0x10)] if e else []
        return {"bytes": nbytes, "errors": e, "first": first, "fill_gbs": 5000.0, "verify_gbs": 6000.0}


class _BasicProbe:
    """A probe from before the deep bindings: device 1's HBM copy is corrupt."""

    def __init__(self, n=2):
        self.n = n

    def device_count(self):
        return self.n

    def copy_check(self, dev, n_floats):
        return dev != 1

    gemm_tile = _FakeDeepProbe.gemm_tile


def _agent(n=8, plugin=False, **kw):
    store = FakeKubeStore()
    topo = synthetic_mi355x(n)
    store.add_node(pu.make_node("n0", n, topo.to_json()))
    api = InProcKube(store)
    agent = NodeAgent(api, "n0", topo, device_plugin=False, health_period_s=0, **kw)
    if plugin:
        agent.plugin = NanoGpuPlugin(topo, api, "n0")
    return agent, store


def _published_health(store):
    ann = store.get_node("n0")["metadata"]["annotations"][T.ANNOTATION_TOPOLOGY]
    return [d.healthy for d in NodeTopology.from_json(ann).devices]


# ----------------------------------------------------------------------------- deep_selftest
def test_deep_selftest_relaunches_for_coverage_and_stays_ok():
    P = _FakeDeepProbe(hidden={0: {(2, 5), (7, 31)}})
    rep = S.deep_selftest(P, 0, hbm_bytes=GIB + 7, seed=1)
    assert [r for _, _, r in P.sweeps] == [4, 8, 16]                  # doubled, three launches at most
    assert rep.ok and rep.sweep["cus_uncovered"] == 2 and rep.sweep["cus_seen"] == 254
    assert rep.sweep["launches"] == 3 and rep.sweep["lds_bytes"] == 163840
    assert P.hbm_calls == [(0, GIB)]                                  # whole 16-byte elements
    clean = _FakeDeepProbe()
    rep = S.deep_selftest(clean, 0)
    assert rep.ok and len(clean.sweeps) == 1 and rep.hbm is None and clean.hbm_calls == []


def test_deep_selftest_ok_iff_no_cu_failed_and_no_hbm_error():
    assert not S.deep_selftest(_FakeDeepProbe(bad_cus={0: [(3, 17, 0b0010, -1)]}), 0).ok
    assert not S.deep_selftest(_FakeDeepProbe(hbm_errors={0: 2}), 0, hbm_bytes=GIB).ok
    assert S.deep_selftest(_FakeDeepProbe(hbm_errors={0: 2}), 0).ok   # not asked to look at HBM
    rep = S.deep_selftest(_FakeDeepProbe(raises=[0]), 0)
    assert not rep.ok and "hipErrorLaunchFailure" in rep.error        # a HIP exception fails the device
    rep = S.deep_selftest(_FakeDeepProbe(bad_cus={0: [(5, 2, S.FAIL_LDS, 40959)]}), 0)
    assert "xcc 5" in rep.describe_failure() and "40959" in rep.describe_failure()


# ----------------------------------------------------------------------------- agent, start-up
def test_deep_startup_marks_exactly_the_failing_devices():
    async def main():
        agent, store = _agent(selftest_deep=True, selftest_hbm_mib=1024)
        await agent.start()
        P = _FakeDeepProbe(bad_cus={2: [(3, 17, 0b0001, -1)]}, hbm_errors={6: 3},
                           hidden={4: {(0, 0)}})                      # device 4: only a coverage shortfall
        assert await agent.selftest(P) == [2, 6]
        assert _published_health(store) == [True, True, False, True, True, True, False, True]
        assert agent.selftest_failed == {2, 6}
        assert P.basic_calls == []                                    # the deep test replaced the basic one
        assert sorted(P.hbm_calls) == [(i, 1024 << 20) for i in range(8)]
        assert agent.selftest_stats["reports"][4]["sweep"]["cus_uncovered"] == 1
        # the device-count guard is unchanged
        assert await agent.selftest(_FakeDeepProbe(4)) is None
        assert agent.selftest_failed == {2, 6}
        await agent.stop()

    asyncio.run(main())


def test_deep_falls_back_to_the_basic_test_on_an_older_probe(caplog):
    async def main():
        agent, store = _agent(2, selftest_deep=True)
        await agent.start()
        with caplog.at_level("WARNING"):
            assert await agent.selftest(_BasicProbe()) == [1]
            assert await agent.selftest(_BasicProbe()) == [1]
        assert sum("no cu_sweep" in r.getMessage() for r in caplog.records) == 1   # logged once
        assert agent.selftest_stats is None
        assert await agent.selftest_periodic(_BasicProbe()) is None   # nothing periodic without the deep kernels
        await agent.stop()

    asyncio.run(main())


def test_plain_selftest_does_not_run_the_deep_one():
    async def main():
        agent, _ = _agent(2)
        await agent.start()
        P = _FakeDeepProbe(2, bad_cus={0: [(0, 0, 1, -1)]})
        assert await agent.selftest(P) == []
        assert P.sweeps == [] and P.basic_calls == [0, 1] and agent.selftest_stats is None
        await agent.stop()

    asyncio.run(main())


def test_hbm_mib_zero_asks_for_free_less_two_gib():
    async def main():
        agent, _ = _agent(1, selftest_deep=True)                      # --selftest-hbm-mib 0
        await agent.start()
        P = _FakeDeepProbe(1, free=100 * GIB + 5)
        assert await agent.selftest(P) == []
        assert P.hbm_calls == [(0, 98 * GIB)]
        agent.selftest_hbm_mib = 512                                  # M > 0 caps it
        await agent.selftest(P)
        assert P.hbm_calls[-1] == (0, 512 << 20)
        tight = _FakeDeepProbe(1, free=GIB)                           # less than the headroom: no HBM check
        assert await agent.selftest(tight) == [] and tight.hbm_calls == []
        await agent.stop()

    asyncio.run(main())


# ----------------------------------------------------------------------------- agent, periodic
def test_periodic_sweeps_only_free_units_and_skips_what_tenants_hold():
    async def main():
        agent, store = _agent(4, plugin=True, selftest_deep=True, selftest_hbm_mib=64)
        await agent.start()
        dc = agent.plugin.cus[0]
        held = dc.grant("a", 25)
        agent.plugin.cus[1].grant("b", 100)                           # no free unit
        agent.plugin.grants[("uid", "c")] = Assignment("default/p", "c", [2], 100, 0, 0)   # whole device, no mask
        P = _FakeDeepProbe(4)
        assert await agent.selftest_periodic(P) == []
        swept = {dev: mask for dev, mask, _ in P.sweeps}
        assert sorted(swept) == [0, 3]                                # devices 1 and 2 are left alone
        free_bits = [u * 8 + k for u in dc.free_units() for k in range(8)]
        assert swept[0] == cumask.mask_words(free_bits)
        assert len(free_bits) == 192 and not set(free_bits) & set(held)
        assert swept[3] == []                                         # no grant: the whole chip
        assert P.hbm_calls == [(3, 64 << 20)]                         # HBM only where nobody has a grant
        assert agent.selftest_stats["reports"][0]["sweep"]["cus_expected"] == 192
        await agent.stop()

    asyncio.run(main())


def test_partitioned_device_is_swept_only_without_a_grant():
    async def main():
        store = FakeKubeStore()
        topo = synthetic_mi355x(1, "CPX")
        store.add_node(pu.make_node("n0", len(topo.devices), topo.to_json()))
        api = InProcKube(store)
        agent = NodeAgent(api, "n0", topo, device_plugin=False, health_period_s=0, selftest_deep=True,
                          selftest_hbm_mib=64)
        agent.plugin = NanoGpuPlugin(topo, api, "n0")
        agent.plugin.cus[1].grant("a", 50)
        assert agent.deep_plan(0) == (None, True)
        assert agent.deep_plan(1) is None

    asyncio.run(main())


def test_periodic_failure_is_sticky():
    async def main():
        agent, store = _agent(2, plugin=True, selftest_deep=True, selftest_hbm_mib=64)
        await agent.start()
        assert await agent.selftest_periodic(_FakeDeepProbe(2, hbm_errors={1: 1})) == [1]
        assert agent.selftest_failed == {1} and agent.plugin.health == [True, False]
        assert _published_health(store) == [True, False]
        assert await agent.selftest_periodic(_FakeDeepProbe(2, bad_cus={0: [(1, 1, S.FAIL_LDS, 7)]})) == [0]
        assert agent.selftest_failed == {0, 1}                        # only grows
        assert await agent.selftest_periodic(_FakeDeepProbe(2)) == [] # a later clean run clears nothing
        assert agent.selftest_failed == {0, 1} and agent.plugin.health == [False, False]
        assert _published_health(store) == [False, False]
        runs = agent.selftest_stats["runs"]
        assert runs == {(0, "pass"): 2, (0, "fail"): 1, (1, "fail"): 1, (1, "pass"): 2}
        await agent.stop()

    asyncio.run(main())


# ----------------------------------------------------------------------------- metrics
def test_metrics_families_appear_with_the_first_deep_run():
    async def main():
        agent, _ = _agent(2, plugin=True, selftest_deep=True, selftest_hbm_mib=64)
        await agent.start()
        before = render_metrics(agent.topo, agent.plugin, agent.render_minors(), "/nonexistent", agent.selftest_stats)
        assert "nanogpu_selftest" not in before
        assert before == render_metrics(agent.topo, agent.plugin, agent.render_minors(), "/nonexistent")
        P = _FakeDeepProbe(2, bad_cus={1: [(3, 17, 0b0001, -1)]}, hidden={0: {(0, 0), (0, 1)}})
        agent.plugin.cus[1].grant("a", 25)
        await agent.selftest_periodic(P)
        after = render_metrics(agent.topo, agent.plugin, agent.render_minors(), "/nonexistent", agent.selftest_stats)
        for line in ('nanogpu_selftest_cus_checked{device="0"} 254', 'nanogpu_selftest_cus_checked{device="1"} 192',
                     'nanogpu_selftest_cus_failed{device="0"} 0', 'nanogpu_selftest_cus_failed{device="1"} 1',
                     'nanogpu_selftest_cus_uncovered{device="0"} 2', 'nanogpu_selftest_cus_uncovered{device="1"} 0',
                     f'nanogpu_selftest_hbm_bytes_checked{{device="0"}} {64 << 20}',
                     'nanogpu_selftest_hbm_bytes_checked{device="1"} 0', 'nanogpu_selftest_hbm_errors{device="0"} 0',
                     'nanogpu_selftest_runs_total{device="0",result="pass"} 1',
                     'nanogpu_selftest_runs_total{device="1",result="fail"} 1',
                     "# TYPE nanogpu_selftest_runs_total counter"):
            assert line in after.splitlines(), line
        for fam in ("nanogpu_selftest_last_run_timestamp_seconds", "nanogpu_selftest_seconds"):
            assert f'{fam}{{device="1"}} ' in after
        # the old families: byte-identical to a render without a deep run (of the same state)
        plain = render_metrics(agent.topo, agent.plugin, agent.render_minors(), "/nonexistent")
        assert after.startswith(plain) and "nanogpu_selftest" not in plain
        assert all(l.startswith(("nanogpu_selftest", "# HELP nanogpu_selftest", "# TYPE nanogpu_selftest"))
                   for l in after[len(plain):].splitlines())
        await agent.stop()

    asyncio.run(main())


# ----------------------------------------------------------------------------- flags
def test_parser_deep_implies_selftest():
    ap = build_parser()
    a = ap.parse_args(["--node-name", "n", "--selftest-deep"])
    assert a.selftest and a.selftest_deep and a.selftest_hbm_mib == 0 and a.selftest_period == 0
    a = ap.parse_args(["--node-name", "n", "--selftest"])
    assert a.selftest and not a.selftest_deep
    a = ap.parse_args(["--node-name", "n"])
    assert not a.selftest and not a.selftest_deep
    a = ap.parse_args(["--selftest-deep", "--selftest-hbm-mib", "4096", "--selftest-period", "3600"])
    assert (a.selftest_hbm_mib, a.selftest_period) == (4096, 3600.0)
