"""Fencing a failing CU's mask unit on a real MI355X (`pytest -m gpu`), device 0 only: the
localisation of an injected failure over all 32 units, the agent's flow end to end, the
whole-device grant's HSA_CU_MASK in a fresh process, and the HBM check on a masked stream.

Failures come from the sweep's own `inject` hook, which flips one bit of a result the workgroup
owns: nothing here makes the device fault."""
import asyncio
import json
import os
import subprocess
import sys
import time
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

MIB = 1 << 20
GIB = 1 << 30
SEED = 0x1234ABCD
UNIT = 8                     # mask bits of a unit on a whole MI355X: one CU on each XCD
UNITS = 32


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


@pytest.fixture(scope="module")
def cu_on_xcd3(P):
    """The CU the injections go to, picked as tests/test_gpu_selftest.py picks it."""
    from nanogpu.probe.selftest_common import cu_key

    r = P.cu_sweep(0, [], 8, SEED)
    return sorted({cu_key(h) for x, h, *_ in r["records"] if x == 3})[5]


class Injecting:
    """The real probe, with `inject` added to every sweep: (xcc, key, 'mfma' | 'lds', ...) goes to
    cu_sweep, (xcc, key, path name) to cu_sweep_paths. One device, whatever the box has. `calls`
    keeps (binding, mask words, rounds, CU keys of the records) of every sweep."""

    def __init__(self, P, inject):
        self._P, self.inject, self.calls = P, inject, []
        self.plain = inject[2] in ("mfma", "lds")

    def __getattr__(self, name):
        return getattr(self._P, name)

    def device_count(self):
        return 1

    def _keep(self, name, mask, rounds, r):
        from nanogpu.probe.selftest_common import cu_key

        self.calls.append((name, list(mask), rounds, {(rec[0], cu_key(rec[1])) for rec in r["records"]}))
        return r

    def cu_sweep(self, dev, mask, rounds, seed):
        return self._keep("cu_sweep", mask, rounds, self._P.cu_sweep(dev, mask, rounds, seed, self.inject if self.plain else None))

    def cu_sweep_paths(self, dev, mask, rounds, seed, paths):
        return self._keep("cu_sweep_paths", mask, rounds,
                          self._P.cu_sweep_paths(dev, mask, rounds, seed, paths, None if self.plain else self.inject))


def _localise(P, inject, paths):
    from nanogpu.probe.selftest import deep_selftest, failed_cus, fenceable, localise_failure

    proxy = Injecting(P, inject)
    rep = deep_selftest(proxy, 0, seed=SEED, paths=paths)
    assert not rep.ok and fenceable(rep), rep.to_dict()
    assert failed_cus(rep) == {(inject[0], inject[1])}
    loc = localise_failure(proxy, 0, rep, range(UNITS), UNIT, paths=paths, seed=SEED)
    print("localisation:", inject[2], paths, round(loc.seconds, 4), "s, launches", loc.launches, "uncovered", loc.uncovered)
    return loc


def _check_localisation(loc, inject):
    # every one of the 32 unit sweeps reached all 8 of its CUs, one per XCD, within the launch limit
    assert sorted(loc.unit_keys) == list(range(UNITS)) and loc.uncovered == {}, loc.uncovered
    for u, keys in loc.unit_keys.items():
        assert len(keys) == UNIT and sorted(x for x, _ in keys) == list(range(8)), (u, keys)
    assert len({k for keys in loc.unit_keys.values() for k in keys}) == UNITS * UNIT     # the units are disjoint
    assert len(loc.bad_units) == 1, loc.bad_units
    assert (inject[0], inject[1]) in loc.unit_keys[loc.bad_units[0]]
    assert loc.unexplained == []


@pytest.mark.parametrize("kind", ["mfma", "lds", "f16"])
def test_localisation_finds_exactly_the_injected_cus_unit(P, cu_on_xcd3, kind):
    inject = {"mfma": (3, cu_on_xcd3, "mfma"), "lds": (3, cu_on_xcd3, "lds", 0), "f16": (3, cu_on_xcd3, "f16")}[kind]
    loc = _localise(P, inject, ["f16"] if kind == "f16" else None)
    record(f"fence_localise_32_units_{kind}", {"seconds": round(loc.seconds, 4),
                                               "launches_per_unit_max": max(loc.launches.values()),
                                               "launches_total": sum(loc.launches.values())})
    _check_localisation(loc, inject)


def test_localisation_with_every_matrix_path(P, cu_on_xcd3):
    inject = (3, cu_on_xcd3, "f16")
    loc = _localise(P, inject, "all")
    record("fence_localise_32_units_all_paths", {"seconds": round(loc.seconds, 4),
                                                 "launches_per_unit_max": max(loc.launches.values()),
                                                 "launches_total": sum(loc.launches.values())})
    _check_localisation(loc, inject)


def _agent(P, inject, **kw):
    from nanogpu.agent.node import NodeAgent
    from nanogpu.agent.plugin import NanoGpuPlugin
    from nanogpu.k8s import podutil as pu
    from nanogpu.k8s.fake_apiserver import FakeKubeStore, InProcKube
    from nanogpu.topology.model import synthetic_mi355x

    store = FakeKubeStore()
    topo = synthetic_mi355x(1)
    store.add_node(pu.make_node("n0", 1, topo.to_json()))
    api = InProcKube(store)
    agent = NodeAgent(api, "n0", topo, device_plugin=False, health_period_s=0, selftest_hbm_mib=64, **kw)
    agent.plugin = NanoGpuPlugin(topo, api, "n0")
    return agent, store, Injecting(P, inject)


def test_agent_fences_the_unit_and_keeps_the_device(P, cu_on_xcd3):
    from nanogpu import types as T
    from nanogpu.topology.model import NodeTopology

    inject = (3, cu_on_xcd3, "mfma")

    async def main():
        agent, store, proxy = _agent(P, inject, selftest_fence=1)
        assert await agent.selftest(proxy) == []
        dev = agent.topo.devices[0]
        assert dev.healthy and agent.plugin.health == [True] and len(dev.fenced) == 1, dev
        u = dev.fenced[0]
        pub = NodeTopology.from_json(store.get_node("n0")["metadata"]["annotations"][T.ANNOTATION_TOPOLOGY])
        assert pub.devices[0].healthy and pub.devices[0].fenced == [u]
        # the verification: the last sweep saw the 248 usable CUs, and not the injected one
        name, mask, rounds, keys = proxy.calls[-1]
        assert len(keys) == 248 and (3, cu_on_xcd3) not in keys
        st = agent.selftest_stats
        rep = st["reports"][0]
        assert rep["sweep"]["cus_seen"] == rep["sweep"]["cus_expected"] == 248 and rep["sweep"]["failed"] == []
        assert rep["hbm"]["bytes"] == 64 * MIB and rep["hbm"]["errors"] == 0      # the HBM check ran, masked, clean
        assert st["runs"] == {(0, "fenced"): 1}
        record("fence_verification_sweep_248_cus", {"ms": round(rep["sweep"]["ms"], 3), "launches": rep["sweep"]["launches"],
                                                    "localise_seconds": round(agent.localise_seconds[0], 4),
                                                    "hbm_64MiB_fill_gbs": round(rep["hbm"]["fill_gbs"], 1),
                                                    "hbm_64MiB_verify_gbs": round(rep["hbm"]["verify_gbs"], 1)})
        granted = agent.plugin.cus[0].grant("t", 25)
        assert len(granted) == 56 and not {b // UNIT for b in granted} & {u}
        n = len(proxy.calls)
        assert await agent.selftest_periodic(proxy) == []
        assert len(proxy.calls) > n and all((3, cu_on_xcd3) not in c[3] for c in proxy.calls[n:])
        assert agent.plugin.health == [True] and agent.topo.devices[0].fenced == [u]

        off, store, proxy = _agent(P, inject, selftest_deep=True)
        assert await off.selftest(proxy) == [0]
        assert off.plugin.health == [False] and off.topo.devices[0].fenced == []

    asyncio.run(main())


_CHILD = r'''
import json, os, sys
sys.path.insert(0, os.environ["REPO"])
from nanogpu.native import probe
from nanogpu.probe.selftest_common import cu_key
P = probe(required=True)
want, seed = int(os.environ["WANT_CUS"]), int(os.environ["SEED"])
keys, rounds = set(), 8
for _ in range(3):                      # deep_selftest's policy: doubled rounds until every CU was reached
    keys |= {(x, cu_key(h)) for x, h, *_ in P.cu_sweep(0, [], rounds, seed)["records"]}
    if len(keys) >= want:
        break
    rounds *= 2
print(json.dumps(sorted(keys)))
'''


def _masked_keys(P, bits, want):
    from nanogpu.agent import cumask
    from nanogpu.probe.selftest_common import cu_key

    keys, rounds = set(), 8
    for _ in range(3):
        keys |= {(x, cu_key(h)) for x, h, *_ in P.cu_sweep(0, cumask.mask_words(bits), rounds, SEED)["records"]}
        if len(keys) >= want:
            break
        rounds *= 2
    return keys


def test_the_whole_grants_environment_fences_a_fresh_process(P):
    """What the fence rests on: HSA_CU_MASK numbers the CUs as the stream mask does. An unmasked
    sweep in a fresh process under the whole-device grant's HSA_CU_MASK for a fence of unit u runs
    on exactly the CUs the parent's stream masked to the same bits reaches, and on none of unit u."""
    from nanogpu.agent import cumask

    u = 17
    dc = cumask.DeviceCUs(256, UNIT, fenced={u})
    usable = dc.usable_bits()
    value = cumask.hsa_cu_mask(0, usable)                 # what plugin._container_response puts into the env
    parent = _masked_keys(P, usable, 248)
    fenced = _masked_keys(P, [u * UNIT + k for k in range(UNIT)], UNIT)
    assert len(parent) == 248 and len(fenced) == UNIT and not parent & fenced
    env = dict(os.environ, REPO=str(Path(__file__).resolve().parent.parent), HSA_CU_MASK=value, WANT_CUS="248",
               SEED=str(SEED))
    r = subprocess.run([sys.executable, "-c", _CHILD], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    child = {tuple(k) for k in json.loads(r.stdout.strip().splitlines()[-1])}
    record("fence_env_in_child", {"hsa_cu_mask": value, "child_cus": len(child), "parent_cus": len(parent),
                                  "child_in_fenced_unit": len(child & fenced), "same_keys": child == parent})
    assert child == parent, (sorted(child - parent), sorted(parent - child))
    assert not child & fenced


def test_the_masked_hbm_check_runs_on_the_masked_cus(P):
    """One unit is an eighth of a 25 % tenant's CUs, and a lone 25 % tenant reaches 51 % of the
    HBM bandwidth (profiles/gpu_calibration.md): a check that really runs on one unit stays far
    below half the unmasked rates."""
    from nanogpu.agent import cumask
    from nanogpu.probe.selftest import pattern_at

    dc = cumask.DeviceCUs(256, UNIT, fenced={17})
    one = cumask.mask_words([17 * UNIT + k for k in range(UNIT)])
    usable = cumask.mask_words(dc.usable_bits())
    t0 = time.perf_counter()
    full = P.hbm_pattern_check(0, GIB, SEED, 2)
    unit = P.hbm_pattern_check(0, GIB, SEED, 2, cu_mask=one)
    most = P.hbm_pattern_check(0, GIB, SEED, 2, cu_mask=usable)
    print("hbm check GB/s (fill, verify): unmasked", full["fill_gbs"], full["verify_gbs"], "1 unit", unit["fill_gbs"],
          unit["verify_gbs"], "31 units", most["fill_gbs"], most["verify_gbs"], "in", time.perf_counter() - t0, "s")
    record("fence_hbm_check_1GiB_gbs", {k: {"fill": round(r["fill_gbs"], 1), "verify": round(r["verify_gbs"], 1)}
                                        for k, r in (("unmasked", full), ("1_unit", unit), ("31_units", most))})
    for r in (full, unit, most):
        assert r["bytes"] == GIB and r["errors"] == 0 and r["first"] == [], r
    assert unit["fill_gbs"] < 0.5 * full["fill_gbs"], (unit, full)
    assert unit["verify_gbs"] < 0.5 * full["verify_gbs"], (unit, full)
    off = 5 * MIB + 16 * 1024 + 7
    r = P.hbm_pattern_check(0, 64 * MIB, SEED, 1, corrupt=[(off, 1)], cu_mask=usable)
    assert r["errors"] == 1 and [f[0] for f in r["first"]] == [off], r
    assert r["first"][0][1] == pattern_at(off, SEED, 0) and r["first"][0][2] == r["first"][0][1] ^ (1 << (8 * (off % 4)))
