"""Node agent /metrics: GPU monitoring at device, pod and container level.

The reference lists "GPU monitor at pod and container level" on its roadmap
(README.md:93) and leaves device metrics to an external exporter queried through Prometheus
(pkg/prometheus/prometheus.go:68-83). This agent serves them itself, in the Prometheus text
format, joined with what it granted:

  per device (schedulable device = GPU or compute partition), read from amdgpu sysfs on scrape
    nanogpu_device_info{device,gpu,partition,part,numa,render}       1
    nanogpu_device_healthy{device}                                   1 | 0
    nanogpu_device_busy_percent{device}                              gpu_busy_percent
    nanogpu_device_mem_busy_percent{device}                          mem_busy_percent (HBM activity)
    nanogpu_device_vram_used_bytes{device} / _vram_total_bytes        mem_info_vram_{used,total}
    nanogpu_device_granted_percent{device}                           sum of container shares
    nanogpu_device_granted_cus{device} / nanogpu_device_cus{device}  CU-mask grants vs CUs
  per container (the grants the device plugin handed out)
    nanogpu_container_gpu_percent{namespace,pod,container,device}
    nanogpu_container_cus{...}                                       CUs in its HSA_CU_MASK
    nanogpu_container_hbm_budget_bytes{...}                          its HBM budget
  per device, once a deep self-test has run (probe/selftest.py; absent before)
    nanogpu_selftest_last_run_timestamp_seconds{device}, nanogpu_selftest_seconds{device}
    nanogpu_selftest_cus_checked / _cus_failed / _cus_uncovered{device}
    nanogpu_selftest_hbm_bytes_checked / _hbm_errors{device}
    nanogpu_selftest_runs_total{device,result}                       result = pass | fail
  per device, when the deep self-test also ran matrix paths (--selftest-paths; absent otherwise)
    nanogpu_selftest_paths_checked{device}                           paths the last run checked on every CU
    nanogpu_selftest_path_cus_failed{device,path}                    CUs that failed that path
  per device, when the deep self-test also ran the vector-ALU part (--selftest-valu; absent otherwise)
    nanogpu_selftest_valu_checked{device}                            groups the last run checked on every CU
  per device, when the deep self-test also ran the scalar part (--selftest-scalar; absent otherwise)
    nanogpu_selftest_scalar_checked{device}                          groups the last run checked on every CU
  per device, when the deep self-test also ran the memory part (--selftest-mem; absent otherwise)
    nanogpu_selftest_mem_checked{device}                             groups the last run checked on every CU
  per device, only with --selftest-fence (agent/node.py: a failing CU's mask unit is fenced, not the GPU)
    nanogpu_selftest_fenced_cus{device}                              CUs in fenced units
    nanogpu_selftest_fenced_units_in_use{device}                     fenced units a grant from before still holds
    nanogpu_selftest_short_grants_total{device}                      grants that got fewer units than their size
    nanogpu_selftest_localise_seconds{device}                        the last localisation (absent before one)
    nanogpu_selftest_runs_total{device,result="fenced"}              runs that ended with a new fence

A pod's utilisation is its share of its device's busy time: the container's CUs over the
device's CUs, times `nanogpu_device_busy_percent` (spatial sharing gives each tenant its own
CUs, which the co-location measurements in profiles/gpu_calibration.md confirm). A sysfs file
that this GPU or partition does not have is left out rather than reported as zero.
"""
from __future__ import annotations

from pathlib import Path

from ..probe.selftest import PARTS


def _esc(v) -> str:
    return str(v).replace("\\", "\\\\").replace('"', '\\"').replace("\n", "\\n")


def _labels(**kv) -> str:
    return "{" + ",".join(f'{k}="{_esc(v)}"' for k, v in kv.items()) + "}"


def _read_int(p: Path) -> int | None:
    try:
        return int(p.read_text().strip())
    except (OSError, ValueError):
        return None


def render(topo, plugin=None, render_minors: list[int] | None = None, sysfs_root: str = "",
           selftest: dict | None = None, fence: dict | None = None) -> str:
    """Prometheus text exposition of the node's devices and the plugin's live grants, of the
    deep self-test (`NodeAgent.selftest_stats`) once one has run, and of the fences
    (`NodeAgent.fence_metrics()`: None, and nothing added, without --selftest-fence)."""
    devs = topo.devices
    minors = render_minors or [128 + 8 * i for i in range(len(devs))]
    health = plugin.health if plugin is not None else [bool(d.healthy) for d in devs]
    grants = list(plugin.grants.values()) if plugin is not None else []
    g_pct = [0] * len(devs)
    g_cus = [0] * len(devs)

    def share(a, d):   # (percent, CUs) a grant holds on device d; no mask = the whole device
        whole = len(a.devices) > 1 or a.percent >= 100 or not a.cus
        return (100 if len(a.devices) > 1 else min(a.percent, 100)), (devs[d].cus if whole else a.cus)

    for a in grants:
        for d in a.devices:
            if 0 <= d < len(devs):
                p, c = share(a, d)
                g_pct[d] += p
                g_cus[d] += c
    out: list[str] = []

    def family(name: str, kind: str, help_: str, rows: list[tuple[str, float]]) -> None:
        if not rows:
            return
        out.append(f"# HELP {name} {help_}")
        out.append(f"# TYPE {name} {kind}")
        out.extend(f"{name}{lab} {val}" for lab, val in rows)

    root = Path(sysfs_root or "/")
    busy, mbusy, used, total = [], [], [], []
    for i, d in enumerate(devs):
        base = root / "sys/class/drm" / f"renderD{minors[i]}" / "device"
        for rows, f in ((busy, "gpu_busy_percent"), (mbusy, "mem_busy_percent"),
                        (used, "mem_info_vram_used"), (total, "mem_info_vram_total")):
            v = _read_int(base / f)
            if v is not None:
                rows.append((_labels(device=i), v))
    gpus = {g.index: g for g in topo.gpus}

    def info(i, d):
        g = gpus.get(d.gpu)
        return _labels(device=i, gpu=d.gpu, partition=g.compute_partition if g else "SPX", part=d.part,
                       numa=g.numa if g else -1, render=minors[i])

    family("nanogpu_device_info", "gauge", "schedulable device (GPU or compute partition) of this node",
           [(info(i, d), 1) for i, d in enumerate(devs)])
    family("nanogpu_device_healthy", "gauge", "1 if the device is advertised Healthy to kubelet",
           [(_labels(device=i), int(bool(health[i]))) for i in range(len(devs))])
    family("nanogpu_device_busy_percent", "gauge", "amdgpu gpu_busy_percent", busy)
    family("nanogpu_device_mem_busy_percent", "gauge", "amdgpu mem_busy_percent (HBM activity)", mbusy)
    family("nanogpu_device_vram_used_bytes", "gauge", "amdgpu mem_info_vram_used", used)
    family("nanogpu_device_vram_total_bytes", "gauge", "amdgpu mem_info_vram_total", total)
    family("nanogpu_device_granted_percent", "gauge", "gpu-percent granted to running containers",
           [(_labels(device=i), g_pct[i]) for i in range(len(devs))])
    family("nanogpu_device_cus", "gauge", "compute units of the device",
           [(_labels(device=i), d.cus) for i, d in enumerate(devs)])
    family("nanogpu_device_granted_cus", "gauge", "compute units held by containers' CU masks",
           [(_labels(device=i), g_cus[i]) for i in range(len(devs))])
    rows_p, rows_c, rows_m = [], [], []
    for a in sorted(grants, key=lambda a: (a.pod_key, a.container)):
        ns, _, pod = a.pod_key.partition("/")
        for d in a.devices:
            if not 0 <= d < len(devs):
                continue
            lab = _labels(namespace=ns, pod=pod, container=a.container, device=d)
            p, c = share(a, d)
            rows_p.append((lab, p))
            rows_c.append((lab, c))
            if a.mib:
                rows_m.append((lab, a.mib * (1 << 20) // max(1, len(a.devices))))
    family("nanogpu_container_gpu_percent", "gauge", "gpu-percent of the device granted to the container", rows_p)
    family("nanogpu_container_cus", "gauge", "compute units the container may use on the device", rows_c)
    family("nanogpu_container_hbm_budget_bytes", "gauge", "HBM budget of the container on the device", rows_m)
    if plugin is not None:
        family("nanogpu_plugin_swaps_fixed_total", "counter",
               "containers kubelet admitted with another container's grant, reconciled from pod-resources",
               [("", plugin.swaps_fixed)])
        family("nanogpu_plugin_id_mismatches_total", "counter",
               "Allocate calls whose kubelet IDs named another device than the container's placement",
               [("", plugin.id_mismatches)])
    if selftest and selftest.get("reports"):
        reps = sorted(selftest["reports"].items())

        def rows(f):
            return [(_labels(device=i), f(r)) for i, r in reps]

        def sweep(key):
            return lambda r: (r.get("sweep") or {}).get(key, 0)

        def hbm(key):
            return lambda r: (r.get("hbm") or {}).get(key, 0)

        family("nanogpu_selftest_last_run_timestamp_seconds", "gauge", "when the device's last deep self-test ended",
               [(_labels(device=i), selftest["at"][i]) for i, _ in reps])
        family("nanogpu_selftest_cus_checked", "gauge", "CUs whose MFMA pipes and LDS the last deep self-test checked",
               rows(sweep("cus_seen")))
        family("nanogpu_selftest_cus_failed", "gauge", "CUs that failed the last deep self-test",
               rows(lambda r: len((r.get("sweep") or {}).get("failed", []))))
        family("nanogpu_selftest_cus_uncovered", "gauge", "CUs the last deep self-test was meant to reach and did not",
               rows(sweep("cus_uncovered")))
        family("nanogpu_selftest_hbm_bytes_checked", "gauge", "HBM bytes the last deep self-test pattern-checked",
               rows(hbm("bytes")))
        family("nanogpu_selftest_hbm_errors", "gauge", "16-byte HBM elements the last deep self-test read back wrong",
               rows(hbm("errors")))
        family("nanogpu_selftest_seconds", "gauge", "duration of the device's last deep self-test",
               rows(lambda r: r.get("seconds", 0)))
        family("nanogpu_selftest_runs_total", "counter", "deep self-tests run, by result",
               [(_labels(device=i, result=res), n) for (i, res), n in sorted(selftest.get("runs", {}).items())])
        for part in PARTS:
            ran = [(i, r[part.key]) for i, r in reps if r.get(part.key)]
            family(f"nanogpu_selftest_{part.key}_checked", "gauge", part.metric_help,
                   [(_labels(device=i), len(p["checked"])) for i, p in ran])
            if part.failed_metric:
                name, label, help_ = part.failed_metric
                family(name, "gauge", help_, [(_labels(device=i, **{label: n}), len(p["failed"].get(n, [])))
                                              for i, p in ran for n in p["checked"]])
        xcd = [(i, r["xcd"]) for i, r in reps if r.get("xcd")]     # only devices where the XCD check ran
        family("nanogpu_selftest_xcd_checked", "gauge", "groups of the XCD check the last deep self-test ran on the device",
               [(_labels(device=i), len(x["checked"])) for i, x in xcd])
        family("nanogpu_selftest_xcd_failed_pairs", "gauge",
               "ordered pairs (writer XCD, reader XCD) that failed the last deep self-test's XCD check, by group",
               [(_labels(device=i, group=g), len(x["failed"].get(g, []))) for i, x in xcd for g in x["checked"]])
        family("nanogpu_selftest_xcd_pairs_verified", "gauge",
               "ordered pairs (writer XCD, reader XCD) the last deep self-test's XCD check verified",
               [(_labels(device=i), x.get("pairs_verified", 0)) for i, x in xcd])
    if fence is not None:
        def per_device(key):
            return [(_labels(device=i), v) for i, v in sorted(fence.get(key, {}).items())]

        family("nanogpu_selftest_fenced_cus", "gauge", "CUs in the CU-mask units the self-test fenced: never granted",
               per_device("fenced_cus"))
        family("nanogpu_selftest_fenced_units_in_use", "gauge",
               "fenced units a grant from before the fence still holds, until its pod ends", per_device("units_in_use"))
        family("nanogpu_selftest_short_grants_total", "counter",
               "grants on a fenced device that got fewer units than their size", per_device("short_grants"))
        family("nanogpu_selftest_localise_seconds", "gauge",
               "duration of the device's last localisation of a failing sweep over its units",
               per_device("localise_seconds"))
    return "\n".join(out) + "\n"


async def serve_metrics(agent, host: str = "0.0.0.0", port: int = 9410):
    """aiohttp server with /metrics and /healthz for a running NodeAgent."""
    from aiohttp import web

    async def metrics(_req):
        text = render(agent.topo, agent.plugin, agent.render_minors(), agent.sysfs_root,
                      getattr(agent, "selftest_stats", None), getattr(agent, "fence_metrics", lambda: None)())
        return web.Response(text=text, content_type="text/plain", charset="utf-8")

    async def healthz(_req):
        return web.Response(text="ok")

    app = web.Application()
    app.router.add_get("/metrics", metrics)
    app.router.add_get("/healthz", healthz)
    runner = web.AppRunner(app)
    await runner.setup()
    site = web.TCPSite(runner, host, port)
    await site.start()
    bound = site._server.sockets[0].getsockname()[1] if site._server and site._server.sockets else port
    return runner, bound
