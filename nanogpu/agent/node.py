"""Node agent: discovers the node's MI355X devices, publishes them, runs the device plugin.

Reference counterpart: the node side is outside the reference repo (nano-gpu-agent,
reference README.md:9, 30-34); the scheduler only reads `capacity["nano-gpu/gpu-percent"]`
(reference pkg/utils/node.go:8-14). This agent publishes, per node:
  * annotation `nano-gpu/topology`: devices (GPU or partition), CUs, XCDs, HBM MiB, NUMA,
    xGMI link matrix, partition modes and optional probe calibration (topology.model);
  * label `amd.com/gpu.present=true` (the load-aware poller's node selector);
  * status capacity/allocatable `nano-gpu/gpu-memory` (HBM MiB) and, without the device
    plugin (`--advertise status`), `nano-gpu/gpu-percent` = 100 x devices;
and serves the kubelet device plugin (plugin.py) for `nano-gpu/gpu-percent`.
"""
from __future__ import annotations

import asyncio
import functools
import json
import logging
import os
import time

from .. import types as T
from ..k8s import podutil as pu
from ..topology.model import NodeTopology, from_host_json

log = logging.getLogger(__name__)


def discover(sysfs_root: str = "", use_amdsmi: bool = True) -> tuple[NodeTopology, dict]:
    from ..native import core

    host = json.loads(core().discover_topology(sysfs_root, use_amdsmi))
    return from_host_json(host), host


def calibrate(topo: NodeTopology, device: int = 0, host: dict | None = None, busy_s: float = 3.0) -> dict:
    """Measures what the annotation cannot read from sysfs, on the real devices (HIP probe):
    the HBM copy rate, and each GPU's own mem_busy_percent scale (GpuSpec.hbm_busy_cal) under
    the probe's stream at 25 % and 100 % of its CUs, which the extender's poller reads HBM
    activity through (telemetry.store.normalize_hbm_activity)."""
    from ..native import probe
    from ..probe.calibrate import hbm_bandwidth, hbm_busy_calibration, local_gpu_facts, mem_busy_files

    out: dict = {}
    facts = local_gpu_facts(device)
    props = facts.get("props") or {}
    if props:
        out["gcn_arch"] = props.get("gcn_arch")
        out["hbm_copy_gbs"] = round(hbm_bandwidth(device, 1 << 30, 10), 1)
        P = probe()
        h = host if host is not None else facts.get("host") or {}
        files = mem_busy_files(h)
        by_index = {g.index: g for g in topo.gpus}
        cals, seen = {}, set()
        # HIP ordinal k is the k-th device the reader lists (KFD order). Whole GPUs (SPX) only:
        # the probe's CU masks assume the full chip
        for k, hg in enumerate((h.get("gpus") or [])[:P.device_count()]):
            parent = int(hg.get("parent", k))
            g = by_index.get(parent)
            if g is None or parent in seen or (hg.get("compute_partition") or "SPX").upper() != "SPX":
                continue
            seen.add(parent)
            try:
                g.hbm_busy_cal = hbm_busy_calibration(P, k, files.get(parent), seconds=busy_s)
            except Exception:   # a probe failure leaves that GPU on the reference scale
                log.exception("mem_busy calibration of GPU %d failed", parent)
                g.hbm_busy_cal = []
            if g.hbm_busy_cal:
                cals[parent] = g.hbm_busy_cal
        out["hbm_busy_cal"] = cals
    topo.calibration.update(out)
    return out


# Elements of the basic tile that hold a chosen value instead of the hashed one: between them they
# set and clear every bit of the bf16 code. 1.0 = 0x3F80 and 2.0 = 0x4000 differ in all eight
# exponent bits, 255 = 0x437F sets the seven mantissa bits, 129 and 131 are odd and >= 129, and
# 256 = 0x4380 is the largest magnitude. A's are on (row, k) = (i, i), B's on (k, col) = (8 + i, i),
# so that no accumulator multiplies two large values.
_BASIC_TILE_A = {(0, 0): 1, (1, 1): 2, (2, 2): 255, (3, 3): -129, (4, 4): 256, (5, 5): -1}
_BASIC_TILE_B = {(8, 0): 1, (9, 1): 2, (10, 2): -255, (11, 3): 131, (12, 4): -256, (13, 5): -2}


def basic_tile_operands() -> tuple[list[float], list[float]]:
    """Operands of `gpu_selftest`'s one tile: A[32][16] and B[16][32], row-major, a fixed function
    of the index. With t = mix32(i) >> 28, element i of the 1,024 is t - 8 where t < 8 and t - 7
    otherwise, so one of +-1..8 (A's element (r, k) is i = 16 r + k, B's (k, c) is
    i = 512 + 32 k + c), but for the twelve of _BASIC_TILE_A and _BASIC_TILE_B.
    tests/test_basic_selftest.py checks each of these conditions:

    * Exact. Every element is an integer of magnitude <= 256, so a bf16 value, and for every
      accumulator sum_k |a||b| < 2^24 (it is below 2^13), so the fp32 result is exact in any
      summation order. Below 2^17 every multiple of 2^-7 is an fp32 value too, so one flipped
      mantissa bit of an operand (2^-7 at the least, times an integer) is not rounded away.
    * Every element matters. No element is 0: each A[r][k] meets a non-zero B[k][c] and each
      B[k][c] a non-zero A[r][k], and a flipped sign bit changes the value.
    * Routing. The rows of A are pairwise distinct, and so are the columns of B. A and B have
      rank 16, so the 16 k-slices differ, a permutation of k applied to one operand alone changes
      C, and distinct rows or columns stay distinct in C. A.B differs from what A or B read
      column-major gives.
    * Bits. Across A, and across B, each of the 16 bits of the bf16 code is 0 in some element and
      1 in some element; both signs occur.
    * C is not constant, and no row or column of C repeats."""
    a, b, _c = _basic_tile()
    return list(a), list(b)


@functools.lru_cache(maxsize=1)
def _basic_tile() -> tuple[tuple[float, ...], tuple[float, ...], tuple[float, ...]]:
    """(A, B, the host's A.B) of `basic_tile_operands`, made once."""
    from ..probe.selftest_common import mix32

    def hashed(i: int) -> int:
        t = mix32(i) >> 28
        return t - 8 if t < 8 else t - 7

    a = [float(_BASIC_TILE_A.get((r, k), hashed(16 * r + k))) for r in range(32) for k in range(16)]
    b = [float(_BASIC_TILE_B.get((k, c), hashed(512 + 32 * k + c))) for k in range(16) for c in range(32)]
    c = [sum(a[r * 16 + k] * b[k * 32 + col] for k in range(16)) for r in range(32) for col in range(32)]
    return tuple(a), tuple(b), tuple(c)


def gpu_selftest(P, device: int) -> bool:
    """Active check of one HIP device with the probe's kernels: a bit-exact 16 MiB HBM copy
    and one bf16 MFMA tile (32x32x16, `basic_tile_operands`: integers, so the fp32 result is
    exact, chosen so that a misrouted row, column or k, a changed element and a flipped bit of
    an operand code all change it) against a host reference. A device that loads its driver and
    shows in sysfs can still compute wrong or fault; the agent then reports it Unhealthy
    (kubelet) and unschedulable (the extender). Runs on the calling thread (HIP's current device)."""
    try:
        if not P.copy_check(device, 1 << 22):
            return False
        a, b = basic_tile_operands()
        c = P.gemm_tile(a, b)                  # on `device`: copy_check made it current
        want = _basic_tile()[2]
        if len(c) != len(want):
            return False
        for i in range(len(want)):
            if c[i] != want[i]:
                return False
        return True
    except Exception:                          # a HIP error is a failed device
        log.exception("self-test of device %d raised", device)
        return False


def node_patch(topo: NodeTopology) -> dict:
    labels = {T.AMD_GPU_NODE_LABEL[0]: T.AMD_GPU_NODE_LABEL[1]}
    if topo.gpus:
        labels["nano-gpu/compute-partition"] = topo.gpus[0].compute_partition or "SPX"
    return {"metadata": {"annotations": {T.ANNOTATION_TOPOLOGY: topo.to_json()}, "labels": labels}}


def status_patch(topo: NodeTopology, advertise_percent: bool) -> dict:
    res = {T.RESOURCE_GPU_MEMORY: str(topo.hbm_capacity_mib())}
    if advertise_percent:
        res[T.RESOURCE_GPU_PERCENT] = str(T.GPU_PERCENT_EACH_CARD * len(topo.devices))
    return {"status": {"capacity": dict(res), "allocatable": dict(res)}}


def carry_fences(topo: NodeTopology, old: NodeTopology) -> dict[int, list[int]]:
    """Copies into `topo` the fences `old` (the node's published topology) holds for the same
    silicon: a device whose GPU has the same non-zero `unique_id` and that has the same part,
    CUs and XCDs. A replaced GPU, or one whose partition mode changed, sheds its fence. A fence
    is a statement about the silicon, so all of it is carried, whatever `--selftest-fence` allows
    now: that number only bounds what this agent adds. Unit indices the device does not have are
    dropped. Returns {device index: units} of what was carried."""
    uid = {g.index: g.unique_id for g in old.gpus}
    was = {(uid.get(d.gpu, 0), d.part): d for d in old.devices if d.fenced and uid.get(d.gpu, 0)}
    now = {g.index: g.unique_id for g in topo.gpus}
    carried = {}
    for i, d in enumerate(topo.devices):
        o = was.get((now.get(d.gpu, 0), d.part))
        if o is not None and (o.cus, o.xcds) == (d.cus, d.xcds):
            n_units = d.cus // max(1, d.xcds)
            d.fenced = sorted({int(u) for u in o.fenced if 0 <= int(u) < n_units})
            if d.fenced:
                carried[i] = d.fenced
    return carried


async def publish(api, node_name: str, topo: NodeTopology, advertise_percent: bool) -> None:
    await api.patch_node(node_name, node_patch(topo))
    await api.patch_node_status(node_name, status_patch(topo, advertise_percent))


class NodeAgent:
    def __init__(self, api, node_name: str, topo: NodeTopology, host: dict | None = None,
                 device_plugin: bool = True, plugin_dir: str = "", health_period_s: float = 10.0,
                 sysfs_root: str = "", kubelet_check_s: float = 1.0, pod_resources_socket: str | None = None,
                 reconcile_period_s: float = 5.0, selftest_deep: bool = False, selftest_hbm_mib: int = 0,
                 selftest_period_s: float = 0.0, selftest_paths=None, selftest_fence: int = 0,
                 selftest_fence_reset: bool = False, selftest_valu=None, selftest_scalar=None, selftest_mem=None,
                 selftest_xcd=None):
        self.api = api
        self.node = node_name
        self.topo = topo
        self.host = host or {}
        self.device_plugin = device_plugin
        self.plugin_dir = plugin_dir
        self.health_period_s = health_period_s
        self.sysfs_root = sysfs_root
        self.kubelet_check_s = kubelet_check_s
        self.selftest_failed: set[int] = set()   # devices whose active self-test failed
        self.selftest_deep = selftest_deep       # probe.selftest.deep_selftest instead of gpu_selftest
        self.selftest_hbm_mib = selftest_hbm_mib  # cap of the HBM pattern check (0: free HBM less 2 GiB)
        self.selftest_period_s = selftest_period_s
        from ..probe.selftest import Selection

        # what every deep sweep also runs of each optional part ("all", "a,b" or names); any of them makes the sweep deep
        self.selftest_parts = Selection.parse(paths=selftest_paths, valu=selftest_valu, scalar=selftest_scalar, mem=selftest_mem)
        if any(vars(self.selftest_parts).values()):
            self.selftest_deep = True
        from ..probe.selftest_xcd import parse_xcd

        # the groups of the XCD check every deep run makes once, on the mask of the sweep; any makes the sweep deep
        self.selftest_xcd = parse_xcd(selftest_xcd)
        if self.selftest_xcd:
            self.selftest_deep = True
        self._no_paths_logged = False
        # > 0: a whole GPU whose deep sweep fails on CUs that fail again when swept alone loses the
        # CU-mask units that hold them (at most this many a device) instead of its health (`_deep_fenced`)
        self.selftest_fence = max(0, int(selftest_fence))
        self.selftest_fence_reset = selftest_fence_reset   # start without the fences the node's annotation holds
        if self.selftest_fence:
            self.selftest_deep = True
        self._fence_proposed: dict[int, list[int]] = {}    # device -> units, from a run until the loop applies them
        self.localise_seconds: dict[int, float] = {}       # device -> its last localisation, for /metrics
        # device -> {(pod uid, container): units} of the whole-device grants that held the device
        # when those units were fenced: they got no mask for them and run there until their pods end
        self.whole_over_fence: dict[int, dict[tuple[str, str], set[int]]] = {}
        self._fence_unpublished = False                    # a fence's node patch failed: sent again at the next run
        self.selftest_stats: dict | None = None  # last deep report per device, for /metrics
        self._no_deep_logged = False
        # kubelet's pod-resources API: which container got which device IDs (plugin.reconcile)
        from .podresources import SOCKET as _PR_SOCKET

        self.pod_resources_socket = pod_resources_socket if pod_resources_socket is not None else _PR_SOCKET
        self.reconcile_period_s = reconcile_period_s
        self.registrations = 0
        self._register = True
        self.plugin = None
        self.server = None
        self.socket_path = ""
        self.informer = None
        self.tasks: list[asyncio.Task] = []

    def render_minors(self) -> list[int]:
        gpus = self.host.get("gpus") or []
        if len(gpus) == len(self.topo.devices):
            return [int(g.get("render_minor", 0)) for g in gpus]
        return [128 + 8 * i for i in range(len(self.topo.devices))]

    async def start(self, register: bool = True) -> None:
        from ..k8s.informer import Informer
        from .plugin import NanoGpuPlugin

        if self.selftest_fence and not self.selftest_fence_reset:
            await self._carry_fences()
        await publish(self.api, self.node, self.topo, advertise_percent=not self.device_plugin)
        if not self.device_plugin:
            return
        self.plugin = NanoGpuPlugin(self.topo, self.api, self.node, self.render_minors())
        # pods on this node: CU grants are rebuilt from the synced informer's view (the API
        # server is the checkpoint), and released when pods finish or go away. Selected by node
        # (as kubelet watches), not by the assume label: each agent sees its own node's pods,
        # not every GPU pod of the cluster, and a label that lands after the binding is no gap
        self.informer = Informer(self.api, "pods", field_selector=f"{T.NODE_NAME_FIELD}={self.node}")
        self.informer.add_handler(self._on_pod)
        self.tasks.append(self.informer.start())
        await self.informer.synced.wait()
        restored = await self.plugin.rebuild(self.informer.list())
        log.info("agent %s: %d devices, %d CU grants restored", self.node, len(self.topo.devices), restored)
        self._register = register
        await self._serve()
        if register and self.kubelet_check_s > 0:
            self.tasks.append(asyncio.ensure_future(self._kubelet_watch()))
        if self.health_period_s > 0:
            self.tasks.append(asyncio.ensure_future(self._health_loop()))
        if self.reconcile_period_s > 0 and self.pod_resources_socket:
            self.tasks.append(asyncio.ensure_future(self._reconcile_loop()))

    async def _carry_fences(self) -> None:
        """Before the first publish: the fences this node's annotation holds stay on the GPUs
        they were measured on (`carry_fences`). A node that cannot be read carries nothing."""
        try:
            node = await self.api.get_node(self.node)
            ann = ((node.get("metadata") or {}).get("annotations") or {}).get(T.ANNOTATION_TOPOLOGY)
            carried = carry_fences(self.topo, NodeTopology.from_json(ann)) if ann else {}
        except Exception as e:
            log.warning("agent %s: no fences carried over, the node's topology could not be read: %s", self.node, e)
            return
        for i, units in sorted(carried.items()):
            log.warning("agent %s: device %d starts with units %s fenced (carried over)", self.node, i, units)

    async def reconcile_now(self) -> list[tuple[str, str]]:
        """One pass: kubelet's pod-resources List against the plugin's grants."""
        from .podresources import list_devices

        if self.plugin is None or not os.path.exists(self.pod_resources_socket):
            return []
        listed = await list_devices(self.pod_resources_socket, T.RESOURCE_GPU_PERCENT)
        moved = await self.plugin.reconcile(listed)
        if moved:
            log.warning("agent %s: %d containers ran with another container's grant; reconciled", self.node,
                        len(moved))
        return moved

    async def _reconcile_loop(self) -> None:
        while True:
            await asyncio.sleep(self.reconcile_period_s)
            try:
                await self.reconcile_now()
            except Exception as e:   # kubelet restarting, socket not served yet
                log.debug("agent %s: pod-resources check failed: %s", self.node, e)

    def _dir(self) -> str:
        return self.plugin_dir or "/var/lib/kubelet/device-plugins"

    async def _serve(self) -> None:
        from .plugin import serve

        self.server, self.socket_path = await serve(self.plugin, self._dir(), register=self._register)
        self.registrations += int(self._register)

    @staticmethod
    def _identity(path: str) -> tuple[int, int] | None:
        try:
            st = os.stat(path)
            return st.st_ino, st.st_mtime_ns
        except OSError:
            return None

    async def _kubelet_watch(self) -> None:
        """A restarted kubelet removes every plugin socket and serves a new kubelet.sock; a
        plugin has to notice, serve again and re-register (its devices are unknown to the new
        kubelet until it does). Both files are polled every `kubelet_check_s`."""
        kubelet_sock = os.path.join(self._dir(), "kubelet.sock")
        seen = self._identity(kubelet_sock)
        while True:
            await asyncio.sleep(self.kubelet_check_s)
            now = self._identity(kubelet_sock)
            if now is None:
                continue                                  # kubelet down: wait for it
            if now == seen and os.path.exists(self.socket_path):
                continue
            log.warning("agent %s: kubelet restarted (or our socket vanished): registering again", self.node)
            try:
                if self.server is not None:
                    await self.server.stop(grace=0.5)
                await self._serve()
                seen = now
            except Exception:
                log.exception("agent %s: re-registration failed; retrying", self.node)

    def _on_pod(self, etype: str, pod: dict, old: dict | None) -> None:
        if pu.node_name_of(pod) != self.node or self.plugin is None:
            return
        # a terminating pod's containers still run on their CUs through the grace period: the
        # grant goes back when they stop (Succeeded/Failed) or the pod object is gone
        if etype == "DELETED" or pu.is_terminated(pod):
            self.plugin.release_pod(pu.pod_uid(pod))

    async def _health_loop(self) -> None:
        while True:
            await asyncio.sleep(self.health_period_s)
            try:
                await self.check_health()
            except Exception:
                log.exception("health check failed")

    async def check_health(self) -> list[int]:
        """Re-reads KFD/DRM sysfs: a device whose render node vanished or whose GPU reports
        uncorrectable RAS errors becomes Unhealthy for kubelet and unschedulable for the
        extender (re-published topology annotation). Returns the devices that changed."""
        topo, host = discover(self.sysfs_root, use_amdsmi=False)
        present = {int(g["render_minor"]) for g in host.get("gpus", [])}
        ras_ok = [d.healthy for d in topo.devices] if len(topo.devices) == len(self.topo.devices) else None
        changed = []
        for i, minor in enumerate(self.render_minors()):
            ok = minor in present and (ras_ok is None or ras_ok[i]) and i not in self.selftest_failed
            if self.topo.devices[i].healthy != ok:
                self.topo.devices[i].healthy = ok
                changed.append(i)
            if self.plugin is not None:
                self.plugin.set_health(i, ok)
        if changed:
            log.warning("agent %s: devices %s health changed", self.node, changed)
            await self.api.patch_node(self.node, node_patch(self.topo))
            self._fence_unpublished = False
        else:
            await self._publish_fences(False)
        return changed

    def run_selftest(self, P=None) -> list[int] | None:
        """`gpu_selftest` on every HIP device; returns the failed device indices, or None when
        the probe is missing or its device count does not match the topology (HIP orders
        devices like the KFD nodes the topology is read from). In deep mode (`selftest_deep`)
        a probe that has `cu_sweep` runs `probe.selftest.deep_selftest` per device instead."""
        if P is None:
            from ..native import probe

            P = probe(required=False)
        if P is None:
            return None
        n = P.device_count()
        if n != len(self.topo.devices):
            log.warning("agent %s: %d HIP devices vs %d topology devices: self-test skipped", self.node, n,
                        len(self.topo.devices))
            return None
        if self.selftest_deep and self._has_deep(P):
            return sorted(i for i, r in self.run_deep(P).items() if not r.ok)
        return [i for i in range(n) if not gpu_selftest(P, i)]

    def _has_deep(self, P) -> bool:
        if hasattr(P, "cu_sweep"):
            return True
        if not self._no_deep_logged:
            self._no_deep_logged = True
            log.warning("agent %s: this probe has no cu_sweep: the basic self-test runs instead of the deep one",
                        self.node)
        return False

    def _is_spx(self, i: int) -> bool:
        gpu = self.topo.devices[i].gpu
        g = next((g for g in self.topo.gpus if g.index == gpu), None)
        return g is None or (g.compute_partition or "SPX").upper() == "SPX"

    def deep_plan(self, i: int) -> tuple[list[int] | None, bool] | None:
        """What a deep self-test may touch on device `i` right now: (CU-mask bits, or None for
        every CU; whether the HBM check may run), or None to leave the device alone. A device
        with no grant gets the whole test. A whole GPU (SPX) that is shared gets a sweep of the
        units no tenant holds and no HBM check; the probe's masks assume the whole chip, so a
        partition that holds a grant is left alone, as is a device without a free unit."""
        if self.plugin is None:
            return None, True
        dc = self.plugin.cus[i]
        whole = any(i in a.devices and (len(a.devices) > 1 or a.percent >= 100 or not a.cus)
                    for a in self.plugin.grants.values())
        if not whole and not dc.used:
            # a fenced unit is never swept again, and the HBM check runs on the usable CUs
            return (dc.usable_bits(), True) if dc.fenced else (None, True)
        free = dc.free_units()
        if whole or not free or not self._is_spx(i):
            return None
        return [u * dc.unit + k for u in free for k in range(dc.unit)], False

    def run_deep(self, P, plans: dict | None = None) -> dict:
        """`deep_selftest` on every device its plan allows (`deep_plan`, taken now unless
        given); returns {device: DeepReport} and keeps the reports for /metrics."""
        from ..probe.selftest import deep_selftest, free_hbm_bytes

        if plans is None:
            plans = {i: self.deep_plan(i) for i in range(len(self.topo.devices))}
        reports = {}
        for i, plan in sorted(plans.items()):
            if plan is None:
                continue
            bits, hbm = plan
            nbytes = 0
            if hbm:
                try:
                    nbytes = free_hbm_bytes(P, i, self.selftest_hbm_mib)
                except Exception:              # the sweep below reports a device that cannot answer
                    log.exception("agent %s: memory info of device %d failed", self.node, i)
            if self.selftest_parts.paths and not hasattr(P, "cu_sweep_paths") and not self._no_paths_logged:
                self._no_paths_logged = True
                log.warning("agent %s: this probe has no cu_sweep_paths: the deep self-test runs without the "
                            "matrix paths", self.node)
            fenced_now = False
            if self.selftest_fence and self.plugin is not None and self._is_spx(i):
                r, fenced_now = self._deep_fenced(P, i, bits, nbytes)
            else:
                r = deep_selftest(P, i, cu_mask_bits=bits, hbm_bytes=nbytes, xcd=self.selftest_xcd, **vars(self.selftest_parts))
            reports[i] = r
            if self.selftest_stats is None:
                self.selftest_stats = {"reports": {}, "at": {}, "runs": {}}
            st = self.selftest_stats
            st["reports"][i], st["at"][i] = r.to_dict(), time.time()
            key = (i, "fenced" if fenced_now else "pass" if r.ok else "fail")
            st["runs"][key] = st["runs"].get(key, 0) + 1
            if not r.ok:
                log.warning("agent %s: deep self-test failed on device %d: %s", self.node, i, r.describe_failure())
        return reports

    def _deep_fenced(self, P, i: int, bits: list[int] | None, nbytes: int):
        """The deep test of whole GPU `i` in fence mode (`--selftest-fence`), on the executor's
        thread: (the report that decides the device, whether it proposes a new fence).

        The sweep runs alone; only a clean chip (or what is usable of it) judges HBM and runs the XCD check
        (`selftest_xcd`), which goes to the runs that get `hbm_bytes`. A failing
        sweep that names CUs (`fenceable`) is localised over the plan's units. When every failed
        CU failed again in a unit swept alone, and the device's fence stays within
        `selftest_fence` units, one verification run over the plan's bits less those units
        (with the HBM check, where the plan allowed it) decides: clean, and with no record from a
        CU that failed, the device passes and the units are proposed for `_fence_locally`.
        Anything else fails the device as without the flag."""
        from ..probe.selftest import deep_selftest, failed_cus, fenceable, localise_failure

        dc = self.plugin.cus[i]
        select = vars(self.selftest_parts)
        sweep = deep_selftest(P, i, cu_mask_bits=bits, **select)
        if sweep.ok:
            more = nbytes or self.selftest_xcd
            return (deep_selftest(P, i, cu_mask_bits=bits, hbm_bytes=nbytes, xcd=self.selftest_xcd, **select) if more else sweep), False
        if not fenceable(sweep):
            return sweep, False
        all_bits = bits if bits is not None else list(range(dc.cus))
        units = sorted({b // dc.unit for b in all_bits} - dc.fenced)
        loc = localise_failure(P, i, sweep, units, dc.unit, **select)
        self.localise_seconds[i] = loc.seconds
        bad = set(loc.bad_units)
        why = (f"CUs {loc.unexplained} failed and no unit swept alone explains them" if loc.unexplained
               else "no unit failed when swept alone" if not bad
               else f"units {sorted(dc.fenced | bad)} are more than the {self.selftest_fence} this agent may fence"
               if len(dc.fenced | bad) > self.selftest_fence else "")
        if why:
            sweep.notes.append("not fenced: " + why)
            log.warning("agent %s: device %d is not fenced: %s", self.node, i, why)
            return sweep, False
        verify = deep_selftest(P, i, cu_mask_bits=[b for b in all_bits if b // dc.unit not in bad],
                               hbm_bytes=nbytes, xcd=self.selftest_xcd, **select)
        stray = sorted(set(verify.cu_keys) & failed_cus(sweep))
        if verify.ok and stray:
            verify.ok = False
            verify.notes.append(f"the sweep masked to the fence still ran on failed CUs {stray}")
        if not verify.ok:
            log.warning("agent %s: device %d: the verification without units %s failed: %s", self.node, i,
                        sorted(bad), verify.describe_failure() or "; ".join(verify.notes))
            return verify, False
        verify.notes.append(f"units {sorted(bad)} fenced: {sweep.describe_failure()}")
        self._fence_proposed[i] = sorted(bad)
        return verify, True

    def _whole_grants(self, i: int) -> list[tuple[str, str]]:
        """Keys of the plugin's grants that hold device `i` whole (no CU mask of their own)."""
        return sorted(k for k, a in self.plugin.grants.items()
                      if i in a.devices and (len(a.devices) > 1 or a.percent >= 100 or not a.cus))

    def _fence_locally(self) -> bool:
        """On the event loop, after a run, without a call that can fail: what `_deep_fenced`
        proposed goes into the plugin's CU maps and the topology. A grant that arrived during the
        run keeps what it got until its pod ends: a fractional one its now-fenced unit
        (`fenced_in_use`), a whole-device one the whole device, answered before there was a fence
        to mask (`whole_over_fence`). Both are logged and counted. True when a fence was added."""
        proposed, self._fence_proposed = self._fence_proposed, {}
        if not proposed or self.plugin is None:
            return False
        for i, units in sorted(proposed.items()):
            dc = self.plugin.cus[i]
            dc.fence(units)
            self.topo.devices[i].fenced = sorted(dc.fenced)
            log.warning("agent %s: device %d: units %s fenced, %d of %d CUs stay usable", self.node, i, units,
                        len(dc.usable_bits()), dc.cus)
            if dc.fenced_in_use():
                log.warning("agent %s: device %d: grants %s hold fenced units until their pods end", self.node, i,
                            dc.fenced_in_use())
            whole = self._whole_grants(i)
            for k in whole:
                self.whole_over_fence.setdefault(i, {}).setdefault(k, set()).update(units)
            if whole:
                log.warning("agent %s: device %d: whole-device grants %s arrived before units %s were fenced and "
                            "run on every CU until their pods end", self.node, i, whole, units)
        return True

    async def _publish_fences(self, added: bool) -> None:
        """The node's annotation gets the fences, after the health of this run is applied. A
        patch that fails is logged and sent again at the next run or health check, so one API
        error neither hides a failed device nor loses a fence for good."""
        if not (added or self._fence_unpublished):
            return
        try:
            await self.api.patch_node(self.node, node_patch(self.topo))
            self._fence_unpublished = False
        except Exception as e:
            self._fence_unpublished = True
            log.warning("agent %s: publishing the fences failed, to be sent again: %s", self.node, e)

    def _fenced_units_in_use(self, i: int) -> int:
        dc = self.plugin.cus[i]
        held = {u for us in dc.used.values() for u in us}
        for k, units in list(self.whole_over_fence.get(i, {}).items()):
            if k in self.plugin.grants:
                held |= units
            else:
                del self.whole_over_fence[i][k]        # its pod ended
        return len(dc.fenced & held)

    def fence_metrics(self) -> dict | None:
        """What /metrics shows of the fences; None without `--selftest-fence` (then nothing is added)."""
        if not self.selftest_fence:
            return None
        cus = self.plugin.cus if self.plugin is not None else []
        return {"fenced_cus": {i: len(dc.fenced) * dc.unit for i, dc in enumerate(cus)},
                "units_in_use": {i: self._fenced_units_in_use(i) for i in range(len(cus))},
                "short_grants": {i: dc.short_grants for i, dc in enumerate(cus)},
                "localise_seconds": dict(self.localise_seconds)}

    async def selftest(self, P=None) -> list[int] | None:
        """Runs the self-test off the event loop and applies it: failed devices become
        Unhealthy for kubelet and unschedulable in the published topology."""
        failed = await asyncio.get_running_loop().run_in_executor(None, self.run_selftest, P)
        if failed is None:
            return None
        self.selftest_failed = set(failed)
        added = self._fence_locally()
        await self._apply_selftest()
        await self._publish_fences(added)
        return failed

    async def _apply_selftest(self) -> None:
        changed = False
        for i, d in enumerate(self.topo.devices):
            ok = i not in self.selftest_failed and d.healthy
            if i in self.selftest_failed and d.healthy:
                d.healthy = False
                changed = True
            if self.plugin is not None:
                self.plugin.set_health(i, ok)
        if changed:
            log.warning("agent %s: self-test failed on devices %s", self.node, sorted(self.selftest_failed))
            await self.api.patch_node(self.node, node_patch(self.topo))

    def _run_periodic(self, P, plans: dict) -> list[int] | None:
        if P is None:
            from ..native import probe

            P = probe(required=False)
        if P is None or P.device_count() != len(self.topo.devices) or not self._has_deep(P):
            return None
        return sorted(i for i, r in self.run_deep(P, plans).items() if not r.ok)

    async def selftest_periodic(self, P=None) -> list[int] | None:
        """One periodic deep run, off the event loop. A shared whole GPU is re-swept on a stream
        masked to the units no tenant holds at this moment (`deep_plan`), so no tenant's CUs are
        touched; HBM is checked only on devices without a grant. A grant that arrives while a
        sweep is in flight shares its new CUs with the sweep until that one ends: 0.26 ms at
        4 rounds, 1 ms at 16, measured on MI355X (profiles/gpu_calibration.md); with `selftest_xcd` another 0.20 ms.
        Failures are sticky
        until the agent restarts: this only ever adds to `selftest_failed`, and a later clean
        run clears nothing. Returns the devices that failed this run, or None when skipped."""
        plans = {i: self.deep_plan(i) for i in range(len(self.topo.devices))}
        failed = await asyncio.get_running_loop().run_in_executor(None, self._run_periodic, P, plans)
        if failed is None:
            return None
        self.selftest_failed |= set(failed)
        added = self._fence_locally()
        await self._apply_selftest()
        await self._publish_fences(added)
        return failed

    async def _selftest_loop(self) -> None:
        while True:
            await asyncio.sleep(self.selftest_period_s)
            try:
                await self.selftest_periodic()
            except Exception:
                log.exception("periodic self-test failed to run")

    def start_selftest_loop(self) -> None:
        if self.selftest_period_s > 0:
            self.tasks.append(asyncio.ensure_future(self._selftest_loop()))

    async def stop(self) -> None:
        for t in self.tasks:
            t.cancel()
        if self.informer is not None:
            await self.informer.stop()
        if self.server is not None:
            await self.server.stop(grace=1.0)


def build_parser():
    import argparse

    ap = argparse.ArgumentParser(prog="nanogpu-agent", description="MI355X node agent for nano-gpu-scheduler")
    ap.add_argument("--node-name", default=os.environ.get("NODE_NAME", ""))
    ap.add_argument("--sysfs-root", default="")
    ap.add_argument("--no-amdsmi", action="store_true")
    ap.add_argument("--calibrate", action="store_true", help="run the HIP probe (HBM GB/s) before publishing")
    ap.add_argument("--advertise", choices=["device-plugin", "status"], default="device-plugin")
    ap.add_argument("--plugin-dir", default="/var/lib/kubelet/device-plugins")
    ap.add_argument("--kube-api", default=None)
    ap.add_argument("--kubeconfig", default=os.environ.get("KUBECONFIG"))
    ap.add_argument("--print", action="store_true", help="print the topology annotation and exit")
    ap.add_argument("--selftest", action="store_true",
                    help="run the HIP self-test (HBM copy + MFMA tile) on every device at start-up")

    class _Deep(argparse.Action):              # --selftest-deep implies --selftest
        def __call__(self, parser, ns, values, option_string=None):
            ns.selftest = ns.selftest_deep = True

    ap.add_argument("--selftest-deep", action=_Deep, nargs=0, default=False,
                    help="the start-up self-test checks every CU (MFMA pipes, LDS) and the free HBM with an "
                         "address-derived pattern instead of one tile and 16 MiB (implies --selftest)")
    from ..probe.selftest import PARTS

    class _Names(argparse.Action):             # the flag of a part (its `const`) of the deep self-test implies --selftest-deep
        def __call__(self, parser, ns, values, option_string=None):
            try:
                setattr(ns, self.dest, self.const.parse(values))
            except ValueError as e:
                parser.error(f"{option_string}: {e}")
            if not getattr(ns, self.dest):
                parser.error(f"{option_string}: name at least one {self.const.flag_noun}, or 'all'")
            ns.selftest = ns.selftest_deep = True

    for part in PARTS:
        ap.add_argument(f"--selftest-{part.key}", action=_Names, const=part, default=[], metavar="all|LIST",
                        help=part.agent_help if part.listed else argparse.SUPPRESS)
    from ..probe import selftest_xcd

    # the XCD check's groups: a check of the device, no part, with the parts' flag action and wording
    ap.add_argument("--selftest-xcd", action=_Names, const=selftest_xcd.FLAG, default=[], metavar="all|LIST", help=argparse.SUPPRESS)

    class _Fence(argparse.Action):             # --selftest-fence N > 0 implies --selftest-deep
        def __call__(self, parser, ns, values, option_string=None):
            if values < 0:
                parser.error(f"{option_string}: a number of units, 0 or more")
            ns.selftest_fence = values
            if values:
                ns.selftest = ns.selftest_deep = True

    ap.add_argument("--selftest-fence", action=_Fence, type=int, default=0, metavar="UNITS",
                    help="a whole GPU (SPX) whose deep self-test fails on CUs that fail again when swept alone stays "
                         "Healthy and loses the CU-mask units (8 CUs, one per XCD, each) that hold them: at most UNITS "
                         "a device, those carried over a restart included (0: off; implies --selftest-deep; needs "
                         "the device plugin)")
    ap.add_argument("--selftest-fence-reset", action="store_true",
                    help="start without the fences the node's topology annotation holds")
    ap.add_argument("--selftest-hbm-mib", type=int, default=0,
                    help="cap of the deep self-test's HBM check in MiB (0: all free HBM less 2 GiB); "
                         "only devices without a grant are checked")
    ap.add_argument("--selftest-period", type=float, default=0.0,
                    help="seconds between deep re-tests of the CUs no tenant holds (0: off)")
    ap.add_argument("--metrics-port", type=int, default=9410,
                    help="device / pod / container GPU metrics on :PORT/metrics (0: off)")
    ap.add_argument("--pod-resources-socket", default="/var/lib/kubelet/pod-resources/kubelet.sock",
                    help="kubelet's pod-resources API: the grants are checked against it ('' : off)")
    ap.add_argument("--reconcile-period", type=float, default=5.0,
                    help="seconds between pod-resources checks (0: off)")
    return ap


def main(argv: list[str] | None = None) -> int:
    ap = build_parser()
    a = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(levelname)s %(name)s: %(message)s")
    topo, host = discover(a.sysfs_root, not a.no_amdsmi)
    if a.calibrate:
        calibrate(topo, host=host)
    if a.print:
        print(json.dumps(topo.to_dict(), indent=1))
        return 0 if topo.devices else 1
    if not a.node_name:
        ap.error("--node-name (or NODE_NAME) is required")

    async def run() -> int:
        import signal

        from ..k8s.client import KubeClient, KubeConfig
        from ..probe.selftest import PARTS

        api = KubeClient(KubeConfig.auto(a.kubeconfig, a.kube_api))
        agent = NodeAgent(api, a.node_name, topo, host, device_plugin=a.advertise == "device-plugin",
                          plugin_dir=a.plugin_dir, sysfs_root=a.sysfs_root,
                          pod_resources_socket=a.pod_resources_socket, reconcile_period_s=a.reconcile_period,
                          selftest_deep=a.selftest_deep, selftest_hbm_mib=a.selftest_hbm_mib,
                          selftest_period_s=a.selftest_period,
                          selftest_fence=a.selftest_fence, selftest_fence_reset=a.selftest_fence_reset,
                          selftest_xcd=a.selftest_xcd,
                          **{name: getattr(a, name) for name in (f"selftest_{part.key}" for part in PARTS)})
        await agent.start()
        if a.selftest:
            failed = await agent.selftest()
            log.info("agent %s: self-test %s", a.node_name,
                     "skipped" if failed is None else f"failed on {failed}" if failed else "passed")
        agent.start_selftest_loop()
        metrics = None
        if a.metrics_port:
            from .metrics import serve_metrics

            metrics, _ = await serve_metrics(agent, port=a.metrics_port)
        stop = asyncio.Event()
        loop = asyncio.get_running_loop()
        for sig in (signal.SIGINT, signal.SIGTERM):
            loop.add_signal_handler(sig, stop.set)
        await stop.wait()
        if metrics is not None:
            await metrics.cleanup()
        await agent.stop()
        await api.close()
        return 0

    return asyncio.run(run())
