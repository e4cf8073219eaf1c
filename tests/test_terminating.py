"""A terminating pod keeps its share until it stops (VERDICT r2 Weak #2).

The reference releases a pod's GPU share as soon as its deletionTimestamp is set
(/root/reference/pkg/utils/pod.go:15-24, controller.go:303-306). The containers keep running
through the grace period, though, holding their HBM and CUs; with an HBM dimension, handing
those to the next pod lets it OOM. kube-scheduler itself keeps terminating pods in its node
accounting. Here the extender's ledger and the agent's CU grants release on DELETED or a
terminal phase (Succeeded/Failed); `--compat` keeps the reference's release-at-deletion.
"""
import asyncio
import json

import aiohttp
import pytest

from nanogpu.app import Config, Runtime
from nanogpu.k8s import podutil as pu
from nanogpu.k8s.client import KubeClient, KubeConfig
from nanogpu.k8s.fake_apiserver import FakeKubeStore, InProcKube, serve
from nanogpu.topology.model import synthetic_mi355x

from test_control_plane import wait_for

TS = "2026-01-01T00:00:00Z"


def _one_gpu_node():
    t = synthetic_mi355x(1)
    return pu.make_node("n0", 1, t.to_json(), {"amd.com/gpu.present": "true"}), t.devices[0].hbm_mib


async def _verb(s, base, verb, body):
    async with s.post(f"{base}/scheduler/{verb}", data=json.dumps(body)) as r:
        return await r.json()


@pytest.mark.parametrize("compat", [False, True])
def test_terminating_pod_keeps_its_hbm_until_deleted(compat):
    """REST client + HTTP fake + native watch filter (the production path). A Running pod
    with a deletionTimestamp keeps 60 % of the GPU's HBM; a second pod needing 60 % fails
    filter until the first is DELETED. In compat mode it fits as soon as deletion starts."""
    async def main():
        node, mib = _one_gpu_node()
        store = FakeKubeStore()
        store.add_node(node)
        runner, port = await serve(store)
        url = f"http://127.0.0.1:{port}"
        rt = Runtime(Config(kube_api=url, port=0, host="127.0.0.1", policy_config_path="/nonexistent",
                            compat=compat, track_hbm=True))
        await rt.start()
        base = f"http://127.0.0.1:{rt.bound_port}"
        big = mib * 6 // 10
        try:
            assert rt.pod_informer.watch_filter is not None
            assert rt.pod_informer.watch_filter.release_on_terminating == compat
            assert await wait_for(lambda: rt.state.node_entry("n0") is not None)
            a = store.create_pod(pu.make_pod("a", [("main", 30, big)]))
            async with aiohttp.ClientSession() as s:
                res = await _verb(s, base, "bind", {"PodName": "a", "PodNamespace": "default",
                                                    "PodUID": pu.pod_uid(a), "Node": "n0"})
                assert res["Error"] == ""
                uid = pu.pod_uid(a)
                led = rt.state.ledger
                assert await wait_for(lambda: (led.lookup(uid) or {}).get("state") == "committed")
                store.set_phase("default", "a", "Running")
                inf = rt.pod_informer
                seen = lambda: inf.events + inf.watch_filter.dropped   # handed on or dropped natively
                ev0 = seen()
                # kubectl delete: the API server sets the deletionTimestamp, the pod runs on
                store.patch_pod("default", "a", {"metadata": {"deletionTimestamp": TS,
                                                              "deletionGracePeriodSeconds": 30}})
                assert await wait_for(lambda: seen() >= ev0 + 1)
                await asyncio.sleep(0.05)
                b = store.create_pod(pu.make_pod("b", [("main", 30, big)]))
                res = await _verb(s, base, "filter", {"Pod": b, "NodeNames": ["n0"]})
                if compat:
                    # the reference's semantics: the share is gone at the deletionTimestamp
                    assert await wait_for(lambda: led.lookup(uid) is None)
                    res = await _verb(s, base, "filter", {"Pod": b, "NodeNames": ["n0"]})
                    assert res["NodeNames"] == ["n0"]
                    return
                assert led.lookup(uid) is not None, "a terminating pod lost its share"
                assert res["NodeNames"] == [] and "n0" in res["FailedNodes"], res
                # the bind is refused too, not only the filter
                res = await _verb(s, base, "bind", {"PodName": "b", "PodNamespace": "default",
                                                    "PodUID": pu.pod_uid(b), "Node": "n0"})
                assert res["Error"]
                # the containers stop and the object goes: now it fits
                store.delete_pod("default", "a")
                assert await wait_for(lambda: led.lookup(uid) is None)
                res = await _verb(s, base, "filter", {"Pod": b, "NodeNames": ["n0"]})
                assert res["NodeNames"] == ["n0"]
        finally:
            await rt.stop()
            await runner.cleanup()

    asyncio.run(main())


def test_terminal_phase_releases_and_restart_counts_terminating_pods():
    """Succeeded releases at once; a rebuild after a restart counts a terminating pod."""
    from nanogpu.state.cluster import ClusterState
    from test_control_plane import annotated, node, runtime, free

    async def main():
        store = FakeKubeStore()
        store.add_node(node())
        rt = await runtime(store)
        try:
            store.create_pod(annotated("t", "n0", [[2]], 40))
            store.create_pod(annotated("d", "n0", [[3]], 40))
            assert await wait_for(lambda: free(rt)[2] == 60 and free(rt)[3] == 60)
            store.patch_pod("default", "t", {"metadata": {"deletionTimestamp": TS}})
            store.set_phase("default", "d", "Succeeded")
            assert await wait_for(lambda: free(rt)[3] == 100)
            await asyncio.sleep(0.05)
            assert free(rt)[2] == 60                       # still terminating: still held
        finally:
            await rt.stop()
        st = ClusterState()
        st.register_node(store.get_node("n0"))
        pods, _ = store.list_pods()
        assert st.rebuild(pods) == 1                       # "t" (terminating), not "d" (done)
        assert st.status()["n0"]["GPUs"][2]["Percent"] == 60
        compat = ClusterState(compat=True)
        compat.register_node(store.get_node("n0"))
        assert compat.rebuild(pods) == 0                   # reference: completed at deletion

    asyncio.run(main())


def test_agent_keeps_a_terminating_pods_cus_out_of_new_grants(sock_dir):
    """The node agent's CU grant outlives the deletionTimestamp: a pod admitted next to a
    terminating one gets disjoint CUs; the grant goes back when the pod has stopped."""
    from nanogpu.agent.node import NodeAgent
    from nanogpu.sim.kubelet import FakeKubelet as SimKubelet
    from test_agent import _schedule

    async def main():
        store = FakeKubeStore()
        topo = synthetic_mi355x(1)
        store.add_node(pu.make_node("n0", 1, topo.to_json()))
        api = InProcKube(store)
        kl = SimKubelet(api, "n0", str(sock_dir))
        await kl.start()
        agent = NodeAgent(api, "n0", topo, device_plugin=True, plugin_dir=str(sock_dir), health_period_s=0)
        await agent.start()
        try:
            await asyncio.wait_for(kl.ready.wait(), 10)
            await _schedule(store, "n0", [pu.make_pod("a", [("main", 60)])])
            a = store.get_pod("default", "a")
            await kl.admit(a)
            owner_a = f"{pu.pod_uid(a)}/main"
            cus = agent.plugin.cus[0]
            assert owner_a in cus.used
            store.patch_pod("default", "a", {"metadata": {"deletionTimestamp": TS}})
            await asyncio.sleep(0.05)
            assert owner_a in cus.used, "CU grant released while the pod still runs"
            # the extender (which holds a's 60 % too) places a 40 % pod on the same GPU
            await _schedule(store, "n0", [pu.make_pod("b", [("main", 40)])], )
            b = store.get_pod("default", "b")
            await kl.admit(b)
            owner_b = f"{pu.pod_uid(b)}/main"
            assert not set(cus.used[owner_a]) & set(cus.used[owner_b])
            store.set_phase("default", "a", "Succeeded")
            assert await wait_for(lambda: owner_a not in cus.used)
        finally:
            await agent.stop()
            await kl.stop()

    asyncio.run(main())
