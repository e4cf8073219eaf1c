"""The deep self-test's matrix paths on a real MI355X (`pytest -m gpu`): one instruction of every
path on arbitrary codes (`matrix_tile`, which establishes the lane maps), the path sweep over
every CU, its injection hook, the masked run, the agent path, and what a visit costs next to
the plain sweep. Corruption is applied to data the kernel owns; nothing here makes the device
fault."""
import json
import random
import statistics

import pytest

pytestmark = pytest.mark.gpu

SEED = 0x1234ABCD


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


def _sweep_all(P, rounds=4, inject=None):
    """One unmasked path sweep with deep_selftest's own policy for coverage (a shortfall is not
    a failure: doubled rounds, three launches at most)."""
    from nanogpu.probe.selftest import fold_sweep
    from nanogpu.probe.selftest_paths import PATHS, fold_paths

    r = P.cu_sweep_paths(0, [], rounds, SEED, list(PATHS), inject)
    records = list(r["records"])
    for more in (rounds * 2, rounds * 4):
        if fold_sweep([x[:5] for x in records], 256)["cus_uncovered"] == 0:
            break
        records += list(P.cu_sweep_paths(0, [], more, SEED, list(PATHS), inject)["records"])
    r["records"] = records
    return r, fold_sweep([x[:5] for x in records], 256), fold_paths(records, r["paths"], 256)


@pytest.fixture(scope="module")
def clean(P):
    return _sweep_all(P)


# ----------------------------------------------------------------------------- one instruction
def _random_codes(path, rng, step):
    """Seeded random codes from the path's exactness window: (A[row][k], B[k][col]). The narrow
    formats draw sign, mantissa and the window's exponents freely. f16 / f32 / f64 hold one
    full-mantissa value per accumulator, as the sweep's generators do (wide_code with a random
    hash): step 0 puts it in A, step 1 in B."""
    from nanogpu.probe import selftest_paths as SP

    dim, K, cb = SP.path_dim(path), SP.PATH_K[path], SP.PATH_CODE_BITS[path]
    ebits, mbits, bias = SP.PATH_FORMAT[path]

    def code(op, idx, k):
        if path == "i8":
            return rng.getrandbits(8)
        if path in ("f16", "f32", "f64"):
            return SP.wide_code(cb, mbits, bias, op, step, idx, k, rng.getrandbits(cb))
        e = rng.choice(SP.PATH_EXP_WINDOW[path])
        return (rng.getrandbits(1) << (ebits + mbits)) | (e << mbits) | rng.getrandbits(mbits)

    a = [[code(0, r, k) for k in range(K)] for r in range(dim)]
    b = [[code(1, c, k) for c in range(dim)] for k in range(K)]
    return a, b


def _assert_exact(path, abs_units):
    """The instruction's own exactness condition: every term is a multiple of the unit (the lowest
    set bit of the sums of |term|), and no accumulator's sum of |term| reaches the limit."""
    from nanogpu.probe import selftest_paths as SP

    tz = min(SP._trailing_zeros(v) for row in abs_units for v in row if v)
    assert max(v >> tz for row in abs_units for v in row) < 1 << SP.PATH_LIMIT_BITS.get(path, 24)


@pytest.mark.parametrize("path", ["f16", "fp8", "bf8", "i8", "mxfp8", "mxfp6", "mxfp4", "f32", "f64"])
def test_matrix_tile_is_the_exact_product(P, path):
    """Every lane, every register and both k halves of one tile, on asymmetric random codes and
    scales: bit-equal with the twin's integer product. A wrong operand or C lane map, a wrong
    code packing or a scale taken from another block or byte cannot pass."""
    from nanogpu.probe import selftest_paths as SP

    rng = random.Random(SEED ^ SP.PATHS.index(path))
    dim = SP.path_dim(path)
    for step, opsel in ((0, (0, 0)), (1, (2, 1))):
        a, b = _random_codes(path, rng, step)
        sa = sb = None
        args = []
        if path in SP.SCALED_PATHS:
            sa = [[rng.choice(SP.SCALE_WINDOW) for _ in range(2)] for _ in range(dim)]
            sb = [[rng.choice(SP.SCALE_WINDOW) for _ in range(dim)] for _ in range(2)]
            args = [[v for row in sa for v in row], [v for row in sb for v in row], opsel]
        assert a != [[b[k][i] for k in range(len(b))] for i in range(dim)]          # asymmetric
        units, abs_units, unit_exp = SP.exact_product(path, a, b, sa, sb)
        _assert_exact(path, abs_units)
        want = SP.tile_words(path, SP.tile_values(path, [u for row in units for u in row], unit_exp))
        got = P.matrix_tile(path, [c for row in a for c in row], [c for row in b for c in row], *args)
        got_words = SP.tile_words(path, got)
        wrong = [i for i in range(len(want)) if want[i] != got_words[i]]
        print(path, "step", step, "opsel", opsel, "wrong words", len(wrong), "of", len(want), wrong[:8])
        assert got_words == want, (path, step, len(wrong), wrong[:8])


# ----------------------------------------------------------------------------- the sweep
def test_path_sweep_reaches_every_cu_and_every_path_is_clean(P, clean):
    from nanogpu.probe.selftest_paths import PATHS

    r, rep, paths = clean
    print("path sweep:", rep["cus_seen"], rep["per_xcd"], r["lds_bytes"], r["ms"], paths["failed"])
    assert list(r["paths"]) == list(PATHS) and list(r["checked"]) == list(PATHS)
    assert rep["cus_seen"] == 256 and rep["per_xcd"] == {x: 32 for x in range(8)}
    assert rep["failed"] == [] and rep["cus_uncovered"] == 0
    assert paths["failed"] == {} and paths["cus"] == [] and paths["cus_seen"] == 256
    assert r["lds_bytes"] == P.device_props(0)["max_shared_per_cu_bytes"]


def _a_cu_on_xcd3(records):
    from nanogpu.probe.selftest_common import cu_key

    return sorted({cu_key(x[1]) for x in records if x[0] == 3})[5]


@pytest.mark.parametrize("path", ["f16", "fp8", "bf8", "i8", "mxfp8", "mxfp6", "mxfp4", "f32", "f64"])
def test_injected_path_fault_fails_exactly_that_cu_and_path(P, clean, path):
    key = _a_cu_on_xcd3(clean[0]["records"])
    _r, rep, paths = _sweep_all(P, 8, (3, key, path))
    assert paths["failed"] == {path: [[3, key]]}, paths["failed"]
    assert paths["cus"] == [{"xcc": 3, "cu_key": key, "paths": [path], "waves": 1}], paths["cus"]
    assert rep["failed"] == []                       # the bf16 chain and the LDS are clean


def test_masked_path_sweep_sees_the_cus_the_census_sees(P):
    from nanogpu.agent import cumask
    from nanogpu.probe.selftest import fold_sweep
    from nanogpu.probe.selftest_common import cu_key
    from nanogpu.probe.selftest_paths import PATHS, fold_paths

    words = cumask.mask_words(cumask.DeviceCUs(256, 8).grant("t", 25))
    census = {(x, cu_key(h)) for x, h in P.cu_census(0, words, 2048, 64)}
    r = P.cu_sweep_paths(0, words, 8, SEED, list(PATHS))
    swept = {(x[0], cu_key(x[1])) for x in r["records"]}
    rep = fold_sweep([x[:5] for x in r["records"]], census)
    assert len(census) == 64
    assert swept == census, (sorted(census - swept), sorted(swept - census))
    assert rep["failed"] == [] and rep["uncovered"] == [] and rep["cus_seen"] == 64
    assert fold_paths(r["records"], r["paths"], census)["failed"] == {}


def test_deep_selftest_with_paths_and_agent_on_the_real_device(P):
    import asyncio

    from nanogpu.agent.metrics import render
    from nanogpu.agent.node import NodeAgent
    from nanogpu.native import core
    from nanogpu.probe.selftest import deep_selftest
    from nanogpu.probe.selftest_paths import PATHS
    from nanogpu.topology.model import from_host_json

    rep = deep_selftest(P, 0, paths="all", hbm_bytes=256 << 20)
    record("deep_selftest_paths_256MiB", {"seconds": round(rep.seconds, 4), "launches": rep.sweep["launches"],
                                          "cus_seen": rep.sweep["cus_seen"], "paths": rep.paths["checked"]})
    assert rep.ok, rep.to_dict()
    assert rep.paths == {"checked": list(PATHS), "failed": {}}
    assert rep.sweep["cus_seen"] == 256 and rep.hbm["errors"] == 0
    topo = from_host_json(json.loads(core().discover_topology("", True)))
    agent = NodeAgent(api=None, node_name="box", topo=topo, device_plugin=False, selftest_paths="all",
                      selftest_hbm_mib=256)
    assert agent.selftest_deep
    failed = asyncio.run(agent.selftest(P)) if len(topo.devices) == P.device_count() else []
    assert failed == [], failed
    if agent.selftest_stats:
        text = render(topo, selftest=agent.selftest_stats)
        assert 'nanogpu_selftest_paths_checked{device="0"} 9' in text
        assert 'nanogpu_selftest_path_cus_failed{device="0",path="mxfp4"} 0' in text


def test_a_path_visit_costs_no_more_than_a_plain_one(P):
    """The sweep runs in the window in which a new grant could share CUs, so a visit must not
    get longer: about 70 MFMA instructions a wave are added to an LDS test of 160 KiB twice.
    Five interleaved pairs of cu_sweep and cu_sweep_paths (all paths) at the same rounds,
    unmasked and at the 25 % mask: the path sweep's median is at most the plain one's plus
    10 %, the run-to-run spread test_pattern_verify_keeps_up_with_the_copy allows on this box."""
    from nanogpu.agent import cumask
    from nanogpu.probe.selftest_paths import PATHS

    words = cumask.mask_words(cumask.DeviceCUs(256, 8).grant("t", 25))
    out = {}
    for name, mask, rounds in (("unmasked_4_rounds", [], 4), ("masked_25pct_8_rounds", words, 8)):
        plain, paths = [], []
        for _ in range(5):
            plain.append(P.cu_sweep(0, mask, rounds, SEED)["ms"])
            paths.append(P.cu_sweep_paths(0, mask, rounds, SEED, list(PATHS))["ms"])
        out[name] = {"cu_sweep_ms": round(statistics.median(plain), 4),
                     "cu_sweep_paths_ms": round(statistics.median(paths), 4),
                     "ratio": round(statistics.median(paths) / statistics.median(plain), 3)}
        print(name, out[name], "plain", plain, "paths", paths)
    record("deep_selftest_path_sweep_time", out)
    for name, m in out.items():
        assert m["cu_sweep_paths_ms"] <= 1.10 * m["cu_sweep_ms"], (name, m)
