"""The deep self-test's matrix paths without a GPU: the format decoders against torch and
written-out tables, the stand-alone host program against the Python twin, the twin's own
exactness and coverage conditions, the folding of path records, and deep_selftest, the node
agent, its flag and its metrics over a fake probe."""
import asyncio
import json
import math
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
from nanogpu.probe import selftest_paths as SP
from nanogpu.topology.model import synthetic_mi355x

GIB = 1 << 30
ALL = [(x, k) for x in range(8) for k in range(32)]


# ----------------------------------------------------------------------------- decoders
@pytest.mark.parametrize("dtype,decode", [("float8_e4m3fn", SP.decode_e4m3fn), ("float8_e5m2", SP.decode_e5m2)])
def test_fp8_decoders_agree_with_torch_on_every_code(dtype, decode):
    import torch

    want = torch.arange(256, dtype=torch.int32).to(torch.uint8).view(getattr(torch, dtype)).float().tolist()
    checked = 0
    for c in range(256):
        got = decode(c)
        if math.isnan(want[c]):
            assert math.isnan(got), c
            continue
        checked += 1
        assert got == want[c] and math.copysign(1, got) == math.copysign(1, want[c]), (c, got, want[c])
    assert checked == (254 if dtype == "float8_e4m3fn" else 250)
    assert SP.decode_e4m3fn(0x7E) == 448.0 and SP.decode_e5m2(0x7B) == 57344.0


def test_small_format_decoders_against_their_tables():
    e2m1 = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
    assert [SP.decode_e2m1(c) for c in range(16)] == e2m1 + [-v for v in e2m1]
    assert math.copysign(1, SP.decode_e2m1(8)) == -1
    e2m3 = [0.0, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875,          # subnormal: m / 8
            1.0, 1.125, 1.25, 1.375, 1.5, 1.625, 1.75, 1.875,
            2.0, 2.25, 2.5, 2.75, 3.0, 3.25, 3.5, 3.75,
            4.0, 4.5, 5.0, 5.5, 6.0, 6.5, 7.0, 7.5]
    assert [SP.decode_e2m3(c) for c in range(64)] == e2m3 + [-v for v in e2m3]
    assert {c: SP.decode_e8m0(c) for c in (0, 120, 126, 127, 128, 129, 254)} == {
        0: 2.0 ** -127, 120: 1 / 128, 126: 0.5, 127: 1.0, 128: 2.0, 129: 4.0, 254: 2.0 ** 127}
    assert math.isnan(SP.decode_e8m0(255))
    assert SP.path_decode("i8", 0x80) == (-128, 0) and SP.path_decode("i8", 0x7F) == (127, 0)
    assert SP.path_decode("f16", 0x3C00) == (1 << 10, -10) and SP.path_decode("f32", 0x3F800000) == (1 << 23, -23)


# ----------------------------------------------------------------------------- host program and twin
@pytest.fixture(scope="module")
def twin():
    """Every path's expected tile from the Python twin, computed once."""
    out = {}
    for p in SP.PATHS:
        t = SP.path_expected(p)
        t["checksum"] = C.tile_checksum(SP.tile_words(p, SP.tile_values(p, t["units"], t["unit_exp"])))
        out[p] = t
    return out


@pytest.mark.parametrize("kind", ["plain", "asan"])
def test_host_program_agrees_with_the_twin(kind, twin):
    """native/tests/selftest_paths_host_main.cpp asserts the header's bounds and coverage itself
    (under ASan + UBSan too); its tiles are the twin's, bit for bit."""
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "native"))
    import build  # native/build.py

    exe = build.build_selftest_host(kind, target="paths")
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    host = json.loads(r.stdout)
    assert list(host) == list(SP.PATHS)
    for p in SP.PATHS:
        assert host[p]["checksum"] == twin[p]["checksum"], p
        assert host[p]["unit_exp"] == twin[p]["unit_exp"] and host[p]["sum_abs_max"] == twin[p]["sum_abs_max"], p


@pytest.mark.parametrize("path", SP.PATHS)
def test_twin_exactness_bound_and_coverage(path, twin):
    t = twin[path]
    limit = {"i8": 31, "f64": 53}.get(path, 24)
    assert t["limit_bits"] == limit and t["exact"] and 0 < t["sum_abs_max"] < 1 << limit
    assert len(t["units"]) == SP.path_dim(path) ** 2 and len(set(t["units"])) > 1
    assert all(abs(u) <= t["sum_abs_max"] for u in t["units"])
    assert SP.path_coverage(path) == []


def test_generators_pack_codes_as_the_kernel_holds_them():
    row = SP.path_codes("mxfp6", 0, 3, 7)
    packed = SP.path_dword("mxfp6", 0, 3, 7, 0) | SP.path_dword("mxfp6", 0, 3, 7, 1) << 32
    assert len(row) == 64 and row[5] == (packed >> 30) & 0x3F                 # code 5 straddles two dwords
    assert all(5 <= (c >> 3) & 0xF <= 8 for c in SP.path_codes("fp8", 1, 2, 9))
    assert all(14 <= (c >> 2) & 0x1F <= 17 for c in SP.path_codes("bf8", 0, 6, 31))
    assert (SP.path_codes("f16", 0, 0, 2)[0] >> 10) & 0x1F == 16 and SP.path_codes("f16", 0, 1, 2)[0] == 0
    assert SP.path_codes("f32", 1, 0, 9)[0] & 0x7FFFFFFF == 0x3F800000
    assert {SP.path_opsel(op, s) for op in range(2) for s in range(SP.PATH_STEPS)} == {0, 1, 2, 3}
    assert SP.parse_paths("all") == list(SP.PATHS) and SP.parse_paths("mxfp4, fp8") == ["fp8", "mxfp4"]
    assert SP.parse_paths(None) == SP.parse_paths("") == SP.parse_paths([]) == []
    with pytest.raises(ValueError):
        SP.parse_paths("fp8,fp9")


# ----------------------------------------------------------------------------- fold_paths
def _hw(key: int, simd: int = 0) -> int:
    return (key << 8) | (simd << 4)


def _records(keys, path_fail=0, waves=0):
    return [(x, _hw(k), 0, 0xF, -1, path_fail, waves) for x, k in keys]


def test_fold_paths_keeps_a_failure_across_a_clean_revisit():
    fp8, mxfp4 = 1 << SP.PATHS.index("fp8"), 1 << SP.PATHS.index("mxfp4")
    seen = [c for c in ALL if c != (6, 9)]
    recs = _records(seen) + _records([(3, 17)], fp8 | mxfp4, 0b0100) + _records(seen)   # two visits; one of (3,17)'s three fails
    rep = SP.fold_paths(recs, SP.PATHS, ALL)
    assert rep["failed"] == {"fp8": [[3, 17]], "mxfp4": [[3, 17]]}
    assert rep["cus"] == [{"xcc": 3, "cu_key": 17, "paths": ["fp8", "mxfp4"], "waves": 0b0100}]
    assert rep["uncovered"] == [[6, 9]] and rep["cus_uncovered"] == 1           # not a failure
    assert rep["cus_seen"] == 255 and rep["cus_expected"] == 256
    clean = SP.fold_paths(_records(ALL), SP.PATHS, 256)
    assert clean["failed"] == {} and clean["cus"] == [] and clean["cus_uncovered"] == 0


# ----------------------------------------------------------------------------- fake probe
class _FakePathProbe:
    """Stands in for nanogpu._probe with the path bindings. Mask bit i is CU (i % 8, i // 8).
    `bad_paths[dev]` = [(xcc, key, path name)]: that CU fails that path when it is selected."""

    def __init__(self, n=2, cus=256, bad_paths=None, free=200 * GIB):
        self.n, self.cus, self.free = n, cus, free
        self.bad_paths = bad_paths or {}
        self.sweeps, self.path_sweeps, self.hbm_calls = [], [], []

    def device_count(self):
        return self.n

    def device_props(self, dev):
        return {"cus": self.cus}

    def mem_info(self, dev):
        return self.free, 288 * GIB

    def _keys(self, mask):
        return [(i % 8, i // 8) for i in range(self.cus) if not mask or (mask[i // 32] >> (i % 32)) & 1]

    def cu_sweep(self, dev, mask, rounds, seed, inject=None):
        self.sweeps.append((dev, list(mask), rounds))
        return {"records": [r[:5] for r in _records(self._keys(mask))], "lds_bytes": 163840, "ms": 0.25}

    def cu_sweep_paths(self, dev, mask, rounds, seed, paths, inject=None):
        self.path_sweeps.append((dev, list(mask), rounds, list(paths)))
        recs = _records(self._keys(mask))
        for x, k, name in self.bad_paths.get(dev, ()):
            if name in paths:
                recs += _records([(x, k)], 1 << SP.PATHS.index(name), 0b0001)
        return {"records": recs, "paths": list(SP.PATHS), "checked": list(paths), "lds_bytes": 163840, "ms": 0.25}

    def hbm_pattern_check(self, dev, nbytes, seed, passes=2, corrupt=(), verify_seed=None):
        self.hbm_calls.append((dev, nbytes))
        return {"bytes": nbytes, "errors": 0, "first": [], "fill_gbs": 5000.0, "verify_gbs": 6000.0}


class _NoPathProbe(_FakePathProbe):
    """A probe from before the path bindings."""
    cu_sweep_paths = property()        # hasattr() is False


def test_deep_selftest_with_all_paths():
    P = _FakePathProbe()
    rep = S.deep_selftest(P, 0, paths="all", seed=1)
    assert rep.ok and rep.paths == {"checked": list(SP.PATHS), "failed": {}}
    assert P.sweeps == [] and [s[3] for s in P.path_sweeps] == [list(SP.PATHS)]     # one visit per CU, not two
    assert rep.sweep["cus_seen"] == 256 and rep.sweep["launches"] == 1
    bad = _FakePathProbe(bad_paths={0: [(3, 17, "mxfp6")]})
    rep = S.deep_selftest(bad, 0, paths="all", seed=1)
    assert not rep.ok and rep.paths["failed"] == {"mxfp6": [[3, 17]]} and rep.sweep["failed"] == []
    assert "mxfp6" in rep.describe_failure() and "xcc 3" in rep.describe_failure()
    assert S.deep_selftest(bad, 0, paths=["fp8", "f64"], seed=1).ok                 # the bad path is not asked for
    assert bad.path_sweeps[-1][3] == ["fp8", "f64"]
    assert rep.to_dict()["paths"]["checked"] == list(SP.PATHS)


def test_deep_selftest_without_paths_never_calls_the_path_sweep():
    for spec in (None, "", []):
        P = _FakePathProbe(bad_paths={0: [(3, 17, "fp8")]})
        rep = S.deep_selftest(P, 0, paths=spec, seed=1)
        assert rep.ok and rep.paths is None and P.path_sweeps == [] and len(P.sweeps) == 1
    assert S.deep_selftest(_FakePathProbe(), 0, seed=1).paths is None


def test_a_probe_without_the_binding_gets_a_note_and_the_plain_sweep():
    P = _NoPathProbe()
    assert not hasattr(P, "cu_sweep_paths")
    rep = S.deep_selftest(P, 0, paths="all", seed=1)
    assert rep.ok and rep.paths is None and len(P.sweeps) == 1
    assert any("no cu_sweep_paths" in n for n in rep.notes)
    assert not S.deep_selftest(_FakePathProbe(), 0, paths="all", seed=1).notes


def test_selftest_cli_rejects_an_unknown_path():
    with pytest.raises(SystemExit) as e:
        S.main(["--paths", "fp8,nope"])
    assert e.value.code == 2


# ----------------------------------------------------------------------------- agent, flag, metrics
def _agent(n=2, **kw):
    store = FakeKubeStore()
    topo = synthetic_mi355x(n)
    store.add_node(pu.make_node("n0", n, topo.to_json()))
    return NodeAgent(InProcKube(store), "n0", topo, device_plugin=False, health_period_s=0, **kw), store


def test_flag_parses_implies_deep_and_rejects_unknown_names(capsys):
    ap = build_parser()
    a = ap.parse_args(["--node-name", "n", "--selftest-paths", "fp8,mxfp4"])
    assert a.selftest and a.selftest_deep and a.selftest_paths == ["fp8", "mxfp4"]
    assert ap.parse_args(["--selftest-paths", "all"]).selftest_paths == list(SP.PATHS)
    a = ap.parse_args(["--node-name", "n", "--selftest-deep"])
    assert a.selftest_deep and a.selftest_paths == []                            # the default is off
    for bad in ("fp8,fp9", "", "bf16"):
        with pytest.raises(SystemExit) as e:
            ap.parse_args(["--selftest-paths", bad])
        assert e.value.code == 2
    assert "unknown matrix path" in capsys.readouterr().err
    assert NodeAgent(None, "n", synthetic_mi355x(1), device_plugin=False, selftest_paths="fp8").selftest_deep
    assert not NodeAgent(None, "n", synthetic_mi355x(1), device_plugin=False).selftest_parts.paths


def test_a_failing_path_makes_the_device_unhealthy_at_startup_and_periodically():
    async def main():
        agent, _ = _agent(2, selftest_paths=["fp8", "mxfp4"], selftest_hbm_mib=64)
        await agent.start()
        P = _FakePathProbe(2, bad_paths={1: [(3, 17, "mxfp4")]})
        assert await agent.selftest(P) == [1]
        assert [d.healthy for d in agent.topo.devices] == [True, False]
        assert P.sweeps == [] and [s[3] for s in P.path_sweeps] == [["fp8", "mxfp4"]] * 2
        assert agent.selftest_stats["reports"][1]["paths"]["failed"] == {"mxfp4": [[3, 17]]}
        later = _FakePathProbe(2, bad_paths={0: [(0, 1, "fp8")]})
        assert await agent.selftest_periodic(later) == [0]                        # the periodic run takes the same paths
        assert [s[3] for s in later.path_sweeps] == [["fp8", "mxfp4"]] * 2 and agent.selftest_failed == {0, 1}
        await agent.stop()

    asyncio.run(main())


def test_an_older_probe_runs_the_plain_deep_test_and_says_so_once(caplog):
    async def main():
        agent, _ = _agent(2, selftest_paths="all")
        await agent.start()
        P = _NoPathProbe(2)
        with caplog.at_level("WARNING"):
            assert await agent.selftest(P) == [] and await agent.selftest(P) == []
        assert sum("no cu_sweep_paths" in r.getMessage() for r in caplog.records) == 1
        assert len(P.sweeps) == 4 and agent.selftest_stats["reports"][0]["paths"] is None
        await agent.stop()

    asyncio.run(main())


def test_metrics_gain_the_two_families_only_when_paths_were_checked():
    async def main():
        with_paths, _ = _agent(2, selftest_paths=["fp8", "mxfp4"], selftest_hbm_mib=64)
        plain, _ = _agent(2, selftest_deep=True, selftest_hbm_mib=64)
        for agent in (with_paths, plain):
            await agent.start()
            assert await agent.selftest(_FakePathProbe(2, bad_paths={1: [(3, 17, "mxfp4"), (3, 18, "mxfp4")]})) == (
                [1] if agent is with_paths else [])
        text = render_metrics(with_paths.topo, None, None, "/nonexistent", with_paths.selftest_stats)
        for line in ('nanogpu_selftest_paths_checked{device="0"} 2', 'nanogpu_selftest_paths_checked{device="1"} 2',
                     'nanogpu_selftest_path_cus_failed{device="0",path="fp8"} 0',
                     'nanogpu_selftest_path_cus_failed{device="1",path="fp8"} 0',
                     'nanogpu_selftest_path_cus_failed{device="1",path="mxfp4"} 2',
                     "# TYPE nanogpu_selftest_paths_checked gauge", "# TYPE nanogpu_selftest_path_cus_failed gauge"):
            assert line in text.splitlines(), line
        # without the flag: byte-identical to what the same reports rendered before paths existed
        stats = plain.selftest_stats
        assert all(r["paths"] is None for r in stats["reports"].values())
        now = render_metrics(plain.topo, None, None, "/nonexistent", stats)
        before = {"reports": {i: {k: v for k, v in r.items() if k != "paths"} for i, r in stats["reports"].items()},
                  "at": stats["at"], "runs": stats["runs"]}
        assert now == render_metrics(plain.topo, None, None, "/nonexistent", before)
        assert "nanogpu_selftest_cus_checked" in now and "nanogpu_selftest_path" not in now
        for agent in (with_paths, plain):
            await agent.stop()

    asyncio.run(main())
