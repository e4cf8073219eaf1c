"""Fencing a failing CU's mask unit without a GPU: the CU map's arithmetic with a fence, the
localisation of a failing sweep over units, the agent's flow, the plugin's answers on a fenced
device, the fence across an agent restart, and /metrics, over a fake probe that honours masks."""
import asyncio
import json

import pytest

from nanogpu import types as T
from nanogpu.agent import cumask
from nanogpu.agent.metrics import render as render_metrics
from nanogpu.agent.node import NodeAgent, build_parser, carry_fences
from nanogpu.agent.plugin import NanoGpuPlugin
from nanogpu.k8s import podutil as pu
from nanogpu.k8s.fake_apiserver import FakeKubeStore, InProcKube
from nanogpu.probe import selftest as S
from nanogpu.probe import selftest_paths as SP
from nanogpu.topology.model import NodeTopology, describe, from_host_json, synthetic_mi355x

GIB = 1 << 30


def _bits(mask, cus=256):
    return [i for i in range(cus) if not mask or (mask[i // 32] >> (i % 32)) & 1]


class _MaskProbe:
    """A probe whose sweeps honour `cu_mask`: mask bit b is CU (xcc = b % 8, key = b // 8), so
    unit u (bits 8u..8u+7) is the CUs with key u. `bad_cus[dev]` = [(xcc, key[, fail bits])] fail
    on every visit, `flaky[dev]` = [(xcc, key)] fail on their first visit only, `bad_paths[dev]` =
    [(xcc, key, path)] fail that matrix path on every visit, `hbm_errors[dev]` = a count."""

    def __init__(self, n=1, cus=256, bad_cus=None, flaky=None, bad_paths=None, hbm_errors=None, free=200 * GIB):
        self.n, self.cus, self.free = n, cus, free
        self.bad_cus, self.flaky = bad_cus or {}, {d: set(v) for d, v in (flaky or {}).items()}
        self.bad_paths, self.hbm_errors = bad_paths or {}, hbm_errors or {}
        self.sweeps, self.hbm_calls = [], []          # (dev, bits, rounds), (dev, bytes, bits or None)

    def device_count(self):
        return self.n

    def device_props(self, dev):
        return {"cus": self.cus}

    def mem_info(self, dev):
        return self.free, 288 * GIB

    def _records(self, dev, mask, rounds, paths=None):
        bits = _bits(mask, self.cus)
        self.sweeps.append((dev, bits, rounds))
        bad = {(c[0], c[1]): (c[2] if len(c) > 2 else 0b0001) for c in self.bad_cus.get(dev, ())}
        recs = []
        for b in bits:
            k = (b % 8, b // 8)
            fail = bad.get(k, 0)
            if k in self.flaky.get(dev, ()):
                self.flaky[dev].discard(k)
                fail |= 0b0001
            rec = (k[0], k[1] << 8, fail, 0xF, -1)
            if paths is not None:
                pf = sum(1 << SP.PATHS.index(p) for x, key, p in self.bad_paths.get(dev, ()) if (x, key) == k and p in paths)
                rec += (pf, 0b0001 if pf else 0)
            recs.append(rec)
        return recs

    def cu_sweep(self, dev, mask, rounds, seed, inject=None):
        return {"records": self._records(dev, mask, rounds), "lds_bytes": 163840, "ms": 0.25}

    def cu_sweep_paths(self, dev, mask, rounds, seed, paths, inject=None):
        return {"records": self._records(dev, mask, rounds, paths), "paths": list(SP.PATHS), "checked": list(paths),
                "lds_bytes": 163840, "ms": 0.25}

    def hbm_pattern_check(self, dev, nbytes, seed, passes=2, corrupt=(), verify_seed=None, cu_mask=None):
        self.hbm_calls.append((dev, nbytes, _bits(cu_mask, self.cus) if cu_mask else None))
        e = self.hbm_errors.get(dev, 0)
        return {"bytes": nbytes, "errors": e, "first": [(4096 * 16, 0x11, 0x10)] if e else [], "fill_gbs": 5000.0,
                "verify_gbs": 6000.0}


class _OldHbmProbe(_MaskProbe):
    """A probe from before hbm_pattern_check took a mask."""

    def hbm_pattern_check(self, dev, nbytes, seed, passes=2, corrupt=(), verify_seed=None):
        self.hbm_calls.append((dev, nbytes, None))
        return {"bytes": nbytes, "errors": 0, "first": [], "fill_gbs": 5000.0, "verify_gbs": 6000.0}


def _unit_bits(u):
    return list(range(8 * u, 8 * u + 8))


def _agent(n=1, topo=None, **kw):
    store = FakeKubeStore()
    topo = topo or synthetic_mi355x(n)
    store.add_node(pu.make_node("n0", len(topo.devices), topo.to_json()))
    api = InProcKube(store)
    agent = NodeAgent(api, "n0", topo, device_plugin=False, health_period_s=0, selftest_hbm_mib=64, **kw)
    agent.plugin = NanoGpuPlugin(topo, api, "n0")
    return agent, store


def _published(store):
    return NodeTopology.from_json(store.get_node("n0")["metadata"]["annotations"][T.ANNOTATION_TOPOLOGY])


# ----------------------------------------------------------------------------- DeviceCUs
@pytest.mark.parametrize("percent,units", [(1, 1), (3, 1), (25, 8), (50, 16), (100, 32)])
def test_an_empty_fence_changes_no_number(percent, units):
    d = cumask.DeviceCUs(256, 8)
    assert d.fenced == set() and d.short_grants == 0
    assert d.units_for(percent) == units == max(1, percent * 32 // 100)
    assert d.free_units() == list(range(32)) and d.usable_units() == list(range(32))
    assert d.grant("a", percent) == list(range(8 * units))
    assert d.free_units() == list(range(units, 32))
    assert d.grant("b", 100) is None and d.short_grants == 0      # no fence: a grant that does not fit is refused
    assert d.fenced_in_use() == []


def test_a_fence_of_one_unit():
    d = cumask.DeviceCUs(256, 8, fenced={5})
    assert len(d.usable_bits()) == 248 and not set(d.usable_bits()) & set(_unit_bits(5))
    assert 5 not in d.free_units() and len(d.free_units()) == 31
    assert [d.units_for(p) for p in (1, 3, 25, 50, 100, 150)] == [1, 1, 7, 15, 31, 31]
    grants = [d.grant(str(i), 25) for i in range(4)]
    assert [len(g) for g in grants] == [56] * 4                   # 7 + 7 + 7 + 7 units
    assert all(not set(g) & set(_unit_bits(5)) for g in grants)
    assert len({b for g in grants for b in g}) == 4 * 56 and d.short_grants == 0
    whole = cumask.DeviceCUs(256, 8, fenced={5})
    assert whole.grant("w", 100) == whole.usable_bits()


def test_a_grant_sized_before_the_fence_leaves_a_short_one():
    d = cumask.DeviceCUs(256, 8)
    for o in "abc":
        assert len(d.grant(o, 25)) == 64                          # 24 units held
    d.fence([30, 31])
    assert d.fenced == {30, 31} and d.units_for(25) == 7
    got = d.grant("d", 25)
    assert got == [b for u in range(24, 30) for b in _unit_bits(u)]   # 6 units, not None
    assert d.short_grants == 1 and d.fenced_in_use() == []
    assert d.grant("e", 3) is None and d.short_grants == 1        # nothing left: refused, and not counted
    assert d.grant("d", 25) == got and d.short_grants == 1        # idempotent


def test_restore_over_a_fence_keeps_the_units_and_is_listed():
    d = cumask.DeviceCUs(256, 8, fenced={5})
    d.restore("old", _unit_bits(4) + _unit_bits(5))
    d.restore("fine", _unit_bits(9))
    assert d.used["old"] == [4, 5] and d.fenced_in_use() == ["old"]
    assert 4 not in d.free_units() and 5 not in d.free_units()
    d.release("old")
    assert d.fenced_in_use() == [] and 5 not in d.free_units() and 4 in d.free_units()
    late = cumask.DeviceCUs(256, 8)
    late.grant("t", 25)
    late.fence([3])                                               # a grant from before the fence keeps its unit
    assert late.fenced_in_use() == ["t"] and late.bits("t") == list(range(64))


# ----------------------------------------------------------------------------- deep_selftest, masked HBM
def test_deep_selftest_passes_its_mask_to_the_hbm_check_only_when_it_has_one():
    P = _MaskProbe()
    rep = S.deep_selftest(P, 0, cu_mask_bits=_unit_bits(2) + _unit_bits(7), hbm_bytes=GIB, seed=1)
    assert rep.ok and P.hbm_calls == [(0, GIB, _unit_bits(2) + _unit_bits(7))]
    assert rep.cu_keys == sorted((x, k) for k in (2, 7) for x in range(8))
    assert "cu_keys" not in rep.to_dict()
    old = _OldHbmProbe()
    assert S.deep_selftest(old, 0, hbm_bytes=GIB, seed=1).ok and old.hbm_calls == [(0, GIB, None)]
    rep = S.deep_selftest(old, 0, cu_mask_bits=_unit_bits(2), hbm_bytes=GIB, seed=1)
    assert rep.ok and rep.hbm is None and old.hbm_calls == [(0, GIB, None)]     # skipped, not failed
    assert any("cu_mask" in n for n in rep.notes)
    assert S.hbm_check_takes_mask(P) and not S.hbm_check_takes_mask(old)
    # the capability is read from the signature: a probe that has the argument and refuses its value
    # fails the device, it is not taken for an older probe
    class Refusing(_MaskProbe):
        def hbm_pattern_check(self, dev, nbytes, seed, passes=2, corrupt=(), verify_seed=None, cu_mask=None):
            raise TypeError("hbm_pattern_check(): incompatible function arguments ... kwargs: cu_mask=[4294967296]")

    rep = S.deep_selftest(Refusing(), 0, cu_mask_bits=_unit_bits(2), hbm_bytes=GIB, seed=1)
    assert not rep.ok and "TypeError" in rep.error
    import dataclasses
    assert dataclasses.replace(S.deep_selftest(P, 0, cu_mask_bits=_unit_bits(2), seed=1)).cu_keys == [(x, 2) for x in range(8)]


# ----------------------------------------------------------------------------- localise_failure
def test_one_bad_cu_gives_exactly_its_unit():
    P = _MaskProbe(bad_cus={0: [(3, 17)]})
    rep = S.deep_selftest(P, 0, seed=1)
    assert not rep.ok and S.fenceable(rep) and S.failed_cus(rep) == {(3, 17)}
    P.sweeps.clear()
    loc = S.localise_failure(P, 0, rep, range(32), 8, paths=None, seed=1)
    assert loc.bad_units == [17] and loc.unexplained == []
    assert loc.unit_keys[17] == [(x, 17) for x in range(8)] and sorted(loc.unit_keys) == list(range(32))
    assert [bits for _, bits, _ in P.sweeps] == [_unit_bits(u) for u in range(32)]     # one masked sweep a unit
    assert P.hbm_calls == [] and loc.launches == {u: 1 for u in range(32)} and loc.seconds > 0


def test_two_bad_cus_in_one_unit_give_one_unit_and_a_path_failure_localises_too():
    P = _MaskProbe(bad_cus={0: [(3, 17), (6, 17, S.FAIL_LDS)]})
    loc = S.localise_failure(P, 0, S.deep_selftest(P, 0, seed=1), range(32), 8, paths=None, seed=1)
    assert loc.bad_units == [17] and loc.unexplained == []
    P = _MaskProbe(bad_paths={0: [(2, 9, "f16")]})
    assert S.deep_selftest(P, 0, seed=1).ok                       # the plain sweep does not see it
    rep = S.deep_selftest(P, 0, seed=1, paths=["f16", "i8"])
    assert not rep.ok and S.fenceable(rep) and S.failed_cus(rep) == {(2, 9)}
    loc = S.localise_failure(P, 0, rep, range(32), 8, paths=["f16", "i8"], seed=1)
    assert loc.bad_units == [9] and loc.unexplained == []
    assert S.localise_failure(P, 0, rep, range(32), 8, paths=["i8"], seed=1).bad_units == []   # the same paths, or nothing


def test_a_flaky_cu_gives_no_bad_unit_and_stays_unexplained():
    P = _MaskProbe(flaky={0: [(3, 17)]})
    rep = S.deep_selftest(P, 0, seed=1)
    assert not rep.ok
    loc = S.localise_failure(P, 0, rep, range(32), 8, paths=None, seed=1)
    assert loc.bad_units == [] and loc.unexplained == [(3, 17)]
    # a bad unit explains only its own CUs: a second failing CU outside the candidates stays unexplained
    P = _MaskProbe(bad_cus={0: [(3, 17), (1, 2)]})
    loc = S.localise_failure(P, 0, S.deep_selftest(P, 0, seed=1), range(8, 32), 8, paths=None, seed=1)
    assert loc.bad_units == [17] and loc.unexplained == [(1, 2)]


def test_what_is_fenceable():
    assert not S.fenceable(S.deep_selftest(_MaskProbe(), 0, seed=1))                       # nothing failed
    assert not S.fenceable(S.deep_selftest(_MaskProbe(bad_cus={0: [(3, 17)]}, hbm_errors={0: 1}), 0, hbm_bytes=GIB))
    assert not S.fenceable(S.deep_selftest(_MaskProbe(bad_cus={0: [(3, 17, 1 << 7)]}), 0))  # a garbled record
    assert S.fail_kinds(1 << 7) == ["record"]
    rep = S.deep_selftest(_MaskProbe(bad_cus={0: [(3, 17)]}), 0)
    rep.error = "RuntimeError: hipErrorLaunchFailure"
    assert not S.fenceable(rep)


# ----------------------------------------------------------------------------- agent
def test_one_bad_cu_is_fenced_and_the_device_stays_healthy():
    async def main():
        agent, store = _agent(selftest_fence=1)
        assert agent.selftest_deep
        P = _MaskProbe(bad_cus={0: [(3, 17)]})
        assert await agent.selftest(P) == []
        assert agent.selftest_failed == set() and agent.plugin.health == [True]
        assert agent.topo.devices[0].healthy and agent.topo.devices[0].fenced == [17]
        pub = _published(store)
        assert pub.devices[0].healthy and pub.devices[0].fenced == [17]
        assert agent.plugin.cus[0].fenced == {17}
        usable = [b for b in range(256) if b // 8 != 17]
        assert P.sweeps[-1][1] == usable                          # the verification: the plan less the fence
        assert P.hbm_calls == [(0, 64 << 20, usable)]             # HBM judged by the usable CUs only
        assert agent.selftest_stats["runs"] == {(0, "fenced"): 1}
        assert agent.selftest_stats["reports"][0]["sweep"]["cus_seen"] == 248
        assert agent.deep_plan(0) == (usable, True)
        # a later periodic run passes and never sweeps a fenced bit; a grant avoids the unit
        P.sweeps.clear()
        granted = agent.plugin.cus[0].grant("t", 25)
        assert await agent.selftest_periodic(P) == []
        assert P.sweeps and all(not set(bits) & set(_unit_bits(17)) for _, bits, _ in P.sweeps)
        assert all(not set(bits) & set(granted) for _, bits, _ in P.sweeps)
        assert len(granted) == 56 and not set(granted) & set(_unit_bits(17))
        assert agent.topo.devices[0].fenced == [17] and agent.plugin.health == [True]
        assert agent.selftest_stats["runs"] == {(0, "fenced"): 1, (0, "pass"): 1}

    asyncio.run(main())


def test_the_same_probe_without_the_flag_fails_the_device_as_before():
    async def main():
        agent, store = _agent(selftest_deep=True)
        P = _MaskProbe(bad_cus={0: [(3, 17)]})
        assert await agent.selftest(P) == [0]
        assert agent.plugin.health == [False] and not _published(store).devices[0].healthy
        assert agent.topo.devices[0].fenced == [] and agent.plugin.cus[0].fenced == set()
        assert len(P.sweeps) == 1 and P.sweeps[0][1] == list(range(256))      # one unmasked call, as before
        assert P.hbm_calls == [(0, 64 << 20, None)]
        assert agent.selftest_stats["runs"] == {(0, "fail"): 1}
        assert "fenced" not in store.get_node("n0")["metadata"]["annotations"][T.ANNOTATION_TOPOLOGY]

    asyncio.run(main())


def test_more_bad_units_than_allowed_fail_the_device():
    async def main():
        bad = {0: [(3, 17), (0, 2), (7, 30)]}
        agent, store = _agent(selftest_fence=2)
        assert await agent.selftest(_MaskProbe(bad_cus=bad)) == [0]
        assert agent.plugin.health == [False] and agent.topo.devices[0].fenced == []
        assert not _published(store).devices[0].healthy
        assert 0 in agent.localise_seconds                        # it was localised, then refused
        agent, _ = _agent(selftest_fence=3)
        assert await agent.selftest(_MaskProbe(bad_cus=bad)) == []
        assert agent.topo.devices[0].fenced == [2, 17, 30]
        # carried-over units count: one fenced at start, two new ones, two allowed
        topo = synthetic_mi355x(1)
        topo.devices[0].fenced = [30]
        agent, _ = _agent(topo=topo, selftest_fence=2)
        assert await agent.selftest(_MaskProbe(bad_cus={0: [(3, 17), (0, 2)]})) == [0]
        assert agent.topo.devices[0].fenced == [30]

    asyncio.run(main())


@pytest.mark.parametrize("probe", [dict(hbm_errors={0: 2}), dict(bad_cus={0: [(3, 17, 1 << 7)]})])
def test_hbm_errors_and_garbled_records_fail_the_device_without_a_localisation(probe):
    async def main():
        agent, store = _agent(selftest_fence=4)
        P = _MaskProbe(**probe)
        assert await agent.selftest(P) == [0]
        assert agent.plugin.health == [False] and agent.topo.devices[0].fenced == []
        assert all(len(bits) == 256 for _, bits, _ in P.sweeps)   # no unit was swept alone
        assert agent.localise_seconds == {}

    asyncio.run(main())


def test_a_flaky_cu_or_a_failed_verification_fails_the_device():
    async def main():
        agent, _ = _agent(selftest_fence=4)
        assert await agent.selftest(_MaskProbe(flaky={0: [(3, 17)]})) == [0]
        assert agent.plugin.health == [False] and agent.topo.devices[0].fenced == []
        # a bad CU and HBM errors: the verification's HBM check, run without the bad unit, fails it
        agent, _ = _agent(selftest_fence=4)
        P = _MaskProbe(bad_cus={0: [(3, 17)]}, hbm_errors={0: 2})
        assert await agent.selftest(P) == [0]
        assert agent.plugin.health == [False] and agent.topo.devices[0].fenced == []
        assert agent.plugin.cus[0].fenced == set() and P.hbm_calls[0][2] == [b for b in range(256) if b // 8 != 17]

    asyncio.run(main())


def test_a_partition_is_not_fenced():
    async def main():
        topo = synthetic_mi355x(1, "CPX")
        agent, store = _agent(topo=topo, selftest_fence=4)
        P = _MaskProbe(len(topo.devices), cus=32, bad_cus={1: [(3, 2)]})
        assert await agent.selftest(P) == [1]
        assert agent.plugin.health[1] is False and all(d.fenced == [] for d in agent.topo.devices)
        assert [d for d, _, _ in P.sweeps] == list(range(8))      # one call a device, as without the flag

    asyncio.run(main())


def test_a_grant_that_arrived_during_the_run_keeps_its_fenced_unit(caplog):
    async def main():
        agent, _ = _agent(selftest_fence=1)
        P = _MaskProbe(bad_cus={0: [(3, 1)]})
        failed = agent.run_selftest(P)                            # the executor's half: proposes only
        assert failed == [] and agent.plugin.cus[0].fenced == set() and agent.topo.devices[0].fenced == []
        held = agent.plugin.cus[0].grant("late", 25)              # takes units 0..7 meanwhile
        with caplog.at_level("WARNING"):
            assert agent._fence_locally() is True
        assert agent.plugin.cus[0].fenced == {1} and agent.plugin.cus[0].bits("late") == held
        assert agent.plugin.cus[0].fenced_in_use() == ["late"]
        assert any("hold fenced units" in r.getMessage() for r in caplog.records)
        assert agent.fence_metrics()["units_in_use"] == {0: 1}

    asyncio.run(main())


def test_a_whole_grant_that_arrived_during_the_run_is_logged_and_counted(caplog):
    async def main():
        agent, store = _agent(selftest_fence=1)
        assert agent.run_selftest(_MaskProbe(bad_cus={0: [(3, 1)]})) == []
        env, ann, _ = await _answer(agent.plugin, store, "whole", 100)      # answered before there is a fence
        assert "HSA_CU_MASK" not in env and ann == "full" and agent.plugin.cus[0].used == {}
        with caplog.at_level("WARNING"):
            agent._fence_locally()
        uid = pu.pod_uid(store.get_pod("default", "whole"))
        assert agent.whole_over_fence == {0: {(uid, "main"): {1}}}
        assert any("whole-device grants" in r.getMessage() and uid in r.getMessage() for r in caplog.records)
        assert agent.plugin.cus[0].fenced_in_use() == [] and agent.fence_metrics()["units_in_use"] == {0: 1}
        text = render_metrics(agent.topo, agent.plugin, agent.render_minors(), "/nonexistent", None, agent.fence_metrics())
        assert 'nanogpu_selftest_fenced_units_in_use{device="0"} 1' in text.splitlines()
        agent.plugin.release_pod(uid)                             # it ends with its pod
        assert agent.fence_metrics()["units_in_use"] == {0: 0} and agent.whole_over_fence == {0: {}}
        env, _, _ = await _answer(agent.plugin, store, "next", 100)         # a whole grant after the fence is masked
        assert env["HSA_CU_MASK"] == "0:0-7,16-255" and agent.fence_metrics()["units_in_use"] == {0: 0}

    asyncio.run(main())


def test_a_failed_fence_patch_neither_hides_a_failed_device_nor_loses_the_fence(caplog):
    async def main():
        agent, store = _agent(2, selftest_fence=1)
        real, calls = agent.api.patch_node, []

        async def patch_node(name, patch):                        # the fence's own patch fails once
            calls.append(patch)
            if len(calls) == 2:
                raise RuntimeError("503 from the API server")
            return await real(name, patch)

        agent.api.patch_node = patch_node
        P = _MaskProbe(2, bad_cus={0: [(3, 17)]}, hbm_errors={1: 2})
        with caplog.at_level("WARNING"):
            assert await agent.selftest(P) == [1]
        assert agent.plugin.health == [True, False]               # kubelet hears of device 1 in this run
        assert agent.plugin.cus[0].fenced == {17} and agent._fence_unpublished
        assert any("to be sent again" in r.getMessage() for r in caplog.records)
        assert [d.healthy for d in _published(store).devices] == [True, False]
        assert await agent.selftest_periodic(P) == [1]            # the next run sends it again
        assert not agent._fence_unpublished and _published(store).devices[0].fenced == [17]

    asyncio.run(main())


def test_parser_fence_implies_deep():
    ap = build_parser()
    a = ap.parse_args(["--node-name", "n", "--selftest-fence", "2"])
    assert a.selftest and a.selftest_deep and a.selftest_fence == 2 and not a.selftest_fence_reset
    a = ap.parse_args(["--node-name", "n"])
    assert a.selftest_fence == 0 and not a.selftest and not a.selftest_deep
    a = ap.parse_args(["--node-name", "n", "--selftest-fence", "0", "--selftest-fence-reset"])
    assert a.selftest_fence == 0 and not a.selftest_deep and a.selftest_fence_reset


# ----------------------------------------------------------------------------- plugin
def _placed(store, name, percent, devices="0"):
    store.create_pod(pu.make_pod(name, [("main", percent)]))
    store.patch_pod("default", name, {"metadata": {"annotations": {T.container_annotation("main"): devices}}})
    return store.get_pod("default", name)


async def _answer(plugin, store, name, percent, devices="0"):
    pod = _placed(store, name, percent, devices)
    r = await plugin._container_response(pod, pu.containers(pod)[0], percent)
    ann = store.get_pod("default", name)["metadata"]["annotations"][T.ANNOTATION_CU_MASK_FMT.format("main")]
    return dict(r.envs), ann, plugin.grants[(pu.pod_uid(pod), "main")]


def test_plugin_answers_on_a_fenced_and_on_an_unfenced_device():
    async def main():
        topo = synthetic_mi355x(2)
        topo.devices[0].fenced = [5]
        store = FakeKubeStore()
        store.add_node(pu.make_node("n0", 2, topo.to_json()))
        plugin = NanoGpuPlugin(topo, InProcKube(store), "n0")
        assert plugin.cus[0].fenced == {5} and plugin.cus[1].fenced == set()
        usable = plugin.cus[0].usable_bits()
        env, ann, a = await _answer(plugin, store, "whole", 100, "0")
        assert env["HSA_CU_MASK"] == "0:0-39,48-255" == cumask.hsa_cu_mask(0, usable)
        assert len(cumask.parse_ranges(env["HSA_CU_MASK"].split(":")[1])) == 248 and env["NANO_GPU_CUS"] == "248"
        assert ann == "full" and a.cus == 0 and plugin.cus[0].used == {}
        plugin.release_pod(pu.pod_uid(store.get_pod("default", "whole")))
        env, ann, a = await _answer(plugin, store, "quarter", 25, "0")
        bits = cumask.parse_ranges(env["HSA_CU_MASK"].split(":")[1])
        assert len(bits) == 56 == a.cus and not set(bits) & set(_unit_bits(5)) and ann == env["HSA_CU_MASK"]
        # two whole devices, device 0 fenced: an entry for that one only. The runtime in the container
        # numbers its devices itself, by physical index, whatever order the placement lists them in
        for name, placed in (("both", "1,0"), ("both2", "0,1")):
            env, ann, a = await _answer(plugin, store, name, 200, placed)
            assert env["HSA_CU_MASK"] == "0:0-39,48-255", placed
            assert env["NANO_GPU_CUS"] == str(256 + 248) and ann == "full" and env["NANO_GPU_DEVICES"] == placed
            plugin.release_pod(pu.pod_uid(store.get_pod("default", name)))
        plugin.cus[1].fence([9])                                  # both fenced: two entries, by rank
        env, _, _ = await _answer(plugin, store, "both3", 200, "1,0")
        assert env["HSA_CU_MASK"] == "0:0-39,48-255;1:0-71,80-255"
        plugin.release_pod(pu.pod_uid(store.get_pod("default", "both3")))
        plugin.cus[1].fenced.clear()
        # the unfenced device answers as it always did
        env, ann, a = await _answer(plugin, store, "whole1", 100, "1")
        assert "HSA_CU_MASK" not in env and "NANO_GPU_CUS" not in env and ann == "full" and a.cus == 0
        assert env == {"NANO_GPU_DEVICES": "1", "NANO_GPU_PERCENT": "100"}
        plugin.release_pod(pu.pod_uid(store.get_pod("default", "whole1")))
        env, ann, a = await _answer(plugin, store, "quarter1", 25, "1")
        assert env == {"NANO_GPU_DEVICES": "1", "NANO_GPU_PERCENT": "25", "HSA_CU_MASK": "0:0-63", "NANO_GPU_CUS": "64"}
        assert ann == "0:0-63" and a.cus == 64

    asyncio.run(main())


def test_a_short_grant_is_logged_with_both_counts(caplog):
    async def main():
        topo = synthetic_mi355x(1)
        store = FakeKubeStore()
        store.add_node(pu.make_node("n0", 1, topo.to_json()))
        plugin = NanoGpuPlugin(topo, InProcKube(store), "n0")
        for o in "abc":
            await _answer(plugin, store, o, 25)
        plugin.cus[0].fence([30, 31])
        with caplog.at_level("WARNING"):
            env, _, a = await _answer(plugin, store, "d", 25)
        assert a.cus == 48 and env["NANO_GPU_CUS"] == "48" and plugin.cus[0].short_grants == 1
        msg = [r.getMessage() for r in caplog.records if "short grant" in r.getMessage()]
        assert len(msg) == 1 and "sized 7 units" in msg[0] and "6 were left" in msg[0]

    asyncio.run(main())


# ----------------------------------------------------------------------------- restart
def _host(uids, partition="SPX"):
    return {"virtualization": "BAREMETAL", "links": [],
            "gpus": [{"kfd_node": 1 + k, "parent": k, "partition": 0, "compute_partition": partition, "cus": 256,
                      "num_xcc": 8, "vram_bytes": 288 << 30, "unique_id": u, "location_id": 0x500 + 0x1000 * k,
                      "gfx_target_version": 90500, "render_minor": 128 + 8 * k} for k, u in enumerate(uids)]}


def test_unique_id_comes_from_the_host_json_and_shows_only_next_to_a_fence():
    t = from_host_json(_host([0xABCDEF0123456789, 77]))
    assert [g.unique_id for g in t.gpus] == [0xABCDEF0123456789, 77]
    plain = t.to_json()
    assert "unique_id" not in plain and "fenced" not in plain
    t.devices[1].fenced = [4]
    d = json.loads(t.to_json())
    assert "unique_id" not in d["gpus"][0] and d["gpus"][1]["unique_id"] == 77
    assert "fenced" not in d["devices"][0] and d["devices"][1]["fenced"] == [4]
    back = NodeTopology.from_json(t.to_json())                    # the annotation round-trips
    assert back.devices[1].fenced == [4] and back.gpus[1].unique_id == 77 and back.to_json() == t.to_json()
    assert describe(back)["fenced"] == {1: "248/256"} and "fenced" not in describe(from_host_json(_host([1])))
    assert back.ledger_devices()[1]["pct_total"] == 100           # the ledger's view does not change


def test_a_topology_without_fences_serialises_exactly_as_before():
    t = synthetic_mi355x(2)
    d = json.loads(t.to_json())
    assert sorted(d["devices"][0]) == ["cus", "gpu", "hbm_mib", "healthy", "mib_share", "part", "pool", "xcds"]
    assert sorted(d["gpus"][0]) == ["bdf", "compute_partition", "cus", "hbm_busy_cal", "hbm_mib", "index",
                                    "memory_partition", "numa", "ras_ce", "ras_ue", "xcds", "xgmi_link_gbs",
                                    "xgmi_peers"]
    assert t.to_json() == json.dumps({"version": 1, "model": t.model, "gfx": t.gfx, "virtualization": t.virtualization,
                                      "gpus": [{k: v for k, v in g.__dict__.items() if k != "unique_id"} for g in t.gpus],
                                      "devices": [{k: v for k, v in x.__dict__.items() if k != "fenced"}
                                                  for x in t.devices],
                                      "link_bw": t.link_bw, "calibration": {}}, separators=(",", ":"), sort_keys=True)


def test_carry_fences_follows_the_silicon():
    old = from_host_json(_host([11, 22, 0]))
    for d in old.devices:
        d.fenced = [3]
    new = from_host_json(_host([22, 33, 0]))                      # GPU 22 moved to index 0, 11 was replaced
    assert carry_fences(new, NodeTopology.from_json(old.to_json())) == {0: [3]}
    assert [d.fenced for d in new.devices] == [[3], [], []]       # unique_id 0 carries nothing
    other = from_host_json(_host([22]))
    other.devices[0].cus = 128                                    # the same chip in another shape: shed
    assert carry_fences(other, old) == {}
    # a fence is carried whole, whatever --selftest-fence allows now; units the device lacks are dropped
    old.devices[1].fenced = [3, 4, 31, 32, -1]
    again = from_host_json(_host([22]))
    assert carry_fences(again, old) == {0: [3, 4, 31]}
    topo = synthetic_mi355x(1)
    topo.devices[0].fenced = [3, 99]
    assert NanoGpuPlugin(topo, None, "n0").cus[0].fenced == {3}


def _restart(uids_before, uids_after, **kw):
    async def main():
        store = FakeKubeStore()
        before = from_host_json(_host(uids_before))
        before.devices[0].fenced = [17]
        store.add_node(pu.make_node("n0", len(before.devices), before.to_json()))
        topo = from_host_json(_host(uids_after))
        agent = NodeAgent(InProcKube(store), "n0", topo, device_plugin=False, health_period_s=0, **kw)
        await agent.start()
        return topo.devices[0].fenced, _published(store).devices[0].fenced

    return asyncio.run(main())


def test_a_fence_survives_a_restart_on_the_same_gpu_only():
    assert _restart([5], [5], selftest_fence=1) == ([17], [17])
    assert _restart([5], [6], selftest_fence=1) == ([], [])       # a replaced GPU sheds it
    assert _restart([0], [0], selftest_fence=1) == ([], [])       # no identity, no fence
    assert _restart([5], [5], selftest_fence=1, selftest_fence_reset=True) == ([], [])
    assert _restart([5], [5]) == ([], [])                         # flag off: nothing is read, nothing carried
    assert _restart([5], [5], selftest_deep=True) == ([], [])


def test_a_carried_fence_reaches_the_plugin_and_the_plan():
    async def main():
        store = FakeKubeStore()
        before = from_host_json(_host([5]))
        before.devices[0].fenced = [17]
        store.add_node(pu.make_node("n0", 1, before.to_json()))
        api = InProcKube(store)
        topo = from_host_json(_host([5]))
        agent = NodeAgent(api, "n0", topo, device_plugin=False, health_period_s=0, selftest_fence=1, selftest_hbm_mib=64)
        await agent.start()
        agent.plugin = NanoGpuPlugin(topo, api, "n0")
        assert agent.plugin.cus[0].fenced == {17}
        P = _MaskProbe(bad_cus={0: [(3, 17)]})                    # the fenced CU still fails: nobody looks
        assert await agent.selftest(P) == []
        assert all(not set(bits) & set(_unit_bits(17)) for _, bits, _ in P.sweeps)
        assert P.hbm_calls == [(0, 64 << 20, agent.plugin.cus[0].usable_bits())]

    asyncio.run(main())


# ----------------------------------------------------------------------------- metrics
METRICS_BEFORE = """\
# HELP nanogpu_device_info schedulable device (GPU or compute partition) of this node
# TYPE nanogpu_device_info gauge
nanogpu_device_info{device="0",gpu="0",partition="SPX",part="0",numa="0",render="128"} 1
# HELP nanogpu_device_healthy 1 if the device is advertised Healthy to kubelet
# TYPE nanogpu_device_healthy gauge
nanogpu_device_healthy{device="0"} 0
# HELP nanogpu_device_granted_percent gpu-percent granted to running containers
# TYPE nanogpu_device_granted_percent gauge
nanogpu_device_granted_percent{device="0"} 0
# HELP nanogpu_device_cus compute units of the device
# TYPE nanogpu_device_cus gauge
nanogpu_device_cus{device="0"} 256
# HELP nanogpu_device_granted_cus compute units held by containers' CU masks
# TYPE nanogpu_device_granted_cus gauge
nanogpu_device_granted_cus{device="0"} 0
# HELP nanogpu_plugin_swaps_fixed_total containers kubelet admitted with another container's grant, reconciled from pod-resources
# TYPE nanogpu_plugin_swaps_fixed_total counter
nanogpu_plugin_swaps_fixed_total 0
# HELP nanogpu_plugin_id_mismatches_total Allocate calls whose kubelet IDs named another device than the container's placement
# TYPE nanogpu_plugin_id_mismatches_total counter
nanogpu_plugin_id_mismatches_total 0
# HELP nanogpu_selftest_last_run_timestamp_seconds when the device's last deep self-test ended
# TYPE nanogpu_selftest_last_run_timestamp_seconds gauge
# HELP nanogpu_selftest_cus_checked CUs whose MFMA pipes and LDS the last deep self-test checked
# TYPE nanogpu_selftest_cus_checked gauge
nanogpu_selftest_cus_checked{device="0"} 192
# HELP nanogpu_selftest_cus_failed CUs that failed the last deep self-test
# TYPE nanogpu_selftest_cus_failed gauge
nanogpu_selftest_cus_failed{device="0"} 1
# HELP nanogpu_selftest_cus_uncovered CUs the last deep self-test was meant to reach and did not
# TYPE nanogpu_selftest_cus_uncovered gauge
nanogpu_selftest_cus_uncovered{device="0"} 0
# HELP nanogpu_selftest_hbm_bytes_checked HBM bytes the last deep self-test pattern-checked
# TYPE nanogpu_selftest_hbm_bytes_checked gauge
nanogpu_selftest_hbm_bytes_checked{device="0"} 0
# HELP nanogpu_selftest_hbm_errors 16-byte HBM elements the last deep self-test read back wrong
# TYPE nanogpu_selftest_hbm_errors gauge
nanogpu_selftest_hbm_errors{device="0"} 0
# HELP nanogpu_selftest_seconds duration of the device's last deep self-test
# TYPE nanogpu_selftest_seconds gauge
# HELP nanogpu_selftest_runs_total deep self-tests run, by result
# TYPE nanogpu_selftest_runs_total counter
nanogpu_selftest_runs_total{device="0",result="fail"} 1
"""


def test_metrics_are_unchanged_without_the_flag_and_gain_families_with_it():
    async def main():
        off, _ = _agent(selftest_deep=True)
        on, _ = _agent(selftest_fence=1)
        for agent in (off, on):
            agent.plugin.cus[0].grant("t", 25)
            await agent.selftest_periodic(_MaskProbe(bad_cus={0: [(3, 17)]}))
        assert off.fence_metrics() is None
        args = (off.topo, off.plugin, off.render_minors(), "/nonexistent", off.selftest_stats)
        text = render_metrics(*args, off.fence_metrics())
        assert text == render_metrics(*args)                      # the renderer of before: no sixth argument
        # the text of this state as rendered before fences existed, less the two rows that hold a time
        timed = ("nanogpu_selftest_last_run_timestamp_seconds{", "nanogpu_selftest_seconds{")
        assert "".join(l + "\n" for l in text.splitlines() if not l.startswith(timed)) == METRICS_BEFORE
        assert "fenced" not in text and "short_grants" not in text and "localise" not in text
        assert 'nanogpu_selftest_runs_total{device="0",result="fail"} 1' in text
        text = render_metrics(on.topo, on.plugin, on.render_minors(), "/nonexistent", on.selftest_stats,
                              on.fence_metrics())
        plain = render_metrics(on.topo, on.plugin, on.render_minors(), "/nonexistent", on.selftest_stats)
        assert text.startswith(plain)
        for line in ('nanogpu_selftest_fenced_cus{device="0"} 8', 'nanogpu_selftest_fenced_units_in_use{device="0"} 0',
                     'nanogpu_selftest_short_grants_total{device="0"} 0',
                     'nanogpu_selftest_runs_total{device="0",result="fenced"} 1',
                     "# TYPE nanogpu_selftest_short_grants_total counter"):
            assert line in text.splitlines(), line
        assert 'nanogpu_selftest_localise_seconds{device="0"} ' in text
        assert 'nanogpu_device_healthy{device="0"} 1' in text and 'nanogpu_device_cus{device="0"} 256' in text

    asyncio.run(main())


# ----------------------------------------------------------------------------- python -m nanogpu.probe.selftest --fence
def test_would_fence_names_the_units_and_their_cus_and_changes_nothing():
    P = _MaskProbe(bad_cus={0: [(3, 17), (0, 2)]})
    rep = S.deep_selftest(P, 0, seed=1)
    plan = S.would_fence(P, 0, rep, 2)
    assert plan["units"] == [2, 17] and plan["reason"] == ""
    assert plan["cus"] == {"2": [[x, 2] for x in range(8)], "17": [[x, 17] for x in range(8)]}
    assert S.would_fence(P, 0, rep, 1)["units"] == [] and "more than 1" in S.would_fence(P, 0, rep, 1)["reason"]
    flaky = _MaskProbe(flaky={0: [(3, 17)]})
    assert "did not fail again" in S.would_fence(flaky, 0, S.deep_selftest(flaky, 0, seed=1), 4)["reason"]
    part = _MaskProbe(cus=32, bad_cus={0: [(3, 2)]})
    assert S.would_fence(part, 0, S.deep_selftest(part, 0, seed=1), 4)["units"] == []
