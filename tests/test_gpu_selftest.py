"""Deep self-test on a real MI355X (`pytest -m gpu`): the probe's cu_sweep over every CU, the
HBM pattern check, and the agent path on top of them. Corruption is applied by the host or in
data the kernel owns; nothing here makes the device fault."""
import json

import pytest

pytestmark = pytest.mark.gpu

MIB = 1 << 20
SEED = 0x1234ABCD
BIG = 64 * MIB + 48          # full blocks plus a 3-element tail


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
def clean(P):
    """One unmasked sweep, shared by the tests that start from a clean chip."""
    from nanogpu.probe.selftest import fold_sweep

    r = P.cu_sweep(0, [], 4, SEED)
    rep = fold_sweep(r["records"], 256)
    for rounds in (8, 16):          # a coverage shortfall is not a failure: deep_selftest's own policy
        if rep["cus_uncovered"] == 0:
            break
        r2 = P.cu_sweep(0, [], rounds, SEED)
        r["records"] = list(r["records"]) + list(r2["records"])
        rep = fold_sweep(r["records"], 256)
    return r, rep


def test_sweep_reaches_every_cu_and_whole_lds(P, clean):
    r, rep = clean
    print("sweep:", {k: rep[k] for k in ("cus_seen", "per_xcd", "simds_seen_min")}, r["lds_bytes"], r["ms"])
    record("deep_selftest_sweep", {"ms_4_rounds": round(r["ms"], 3), "simds_seen_min": rep["simds_seen_min"],
                                   "lds_bytes": r["lds_bytes"], "cus_seen": rep["cus_seen"]})
    assert rep["cus_seen"] == 256
    assert rep["per_xcd"] == {x: 32 for x in range(8)}
    assert rep["failed"] == [] and rep["cus_uncovered"] == 0
    assert r["lds_bytes"] == P.device_props(0)["max_shared_per_cu_bytes"]


def test_masked_sweep_sees_the_cus_the_census_sees(P):
    from nanogpu.agent import cumask
    from nanogpu.probe.selftest import fold_sweep
    from nanogpu.probe.selftest_common import cu_key

    bits = cumask.DeviceCUs(256, 8).grant("t", 25)
    words = cumask.mask_words(bits)
    census = {(x, cu_key(h)) for x, h in P.cu_census(0, words, 2048, 64)}
    r = P.cu_sweep(0, words, 8, SEED)
    swept = {(x, cu_key(h)) for x, h, *_ in r["records"]}
    rep = fold_sweep(r["records"], census)
    record("deep_selftest_masked_sweep_ms_25pct_8_rounds", round(r["ms"], 3))
    assert len(census) == 64
    assert swept == census, (sorted(census - swept), sorted(swept - census))
    assert rep["failed"] == [] and rep["uncovered"] == [] and rep["cus_seen"] == 64


def _a_cu_on_xcd3(rep_records):
    from nanogpu.probe.selftest_common import cu_key

    return sorted({cu_key(h) for x, h, *_ in rep_records if x == 3})[5]


def test_injected_mfma_fault_fails_exactly_that_cu(P, clean):
    from nanogpu.probe.selftest import fold_sweep

    key = _a_cu_on_xcd3(clean[0]["records"])
    r = P.cu_sweep(0, [], 8, SEED, (3, key, "mfma"))
    rep = fold_sweep(r["records"], 256)
    assert rep["failed"] == [{"xcc": 3, "cu_key": key, "kinds": ["mfma"], "lds_bad_off": -1}], rep["failed"]


# The read-back visits dword n - 1 - j with a stride of 256 threads: besides the two ends, the
# last dword of the first stride and the first of the second (255, 256), the middle, and the
# same two counted from the end (n - 256, n - 257) are where an index slip would hide.
LDS_OFFSETS = {"last": lambda n: n - 1, "first": lambda n: 0, "255": lambda n: 255, "256": lambda n: 256,
               "half": lambda n: n // 2, "n-256": lambda n: n - 256, "n-257": lambda n: n - 257}


@pytest.mark.parametrize("where", list(LDS_OFFSETS))
def test_injected_lds_fault_reports_the_offset(P, clean, where):
    from nanogpu.probe.selftest import fold_sweep

    key = _a_cu_on_xcd3(clean[0]["records"])
    n = clean[0]["lds_bytes"] // 4              # 40960 when the workgroup holds all 160 KiB
    off = LDS_OFFSETS[where](n)
    r = P.cu_sweep(0, [], 8, SEED, (3, key, "lds", off))
    rep = fold_sweep(r["records"], 256)
    assert rep["failed"] == [{"xcc": 3, "cu_key": key, "kinds": ["lds"], "lds_bad_off": off}], rep["failed"]


def test_two_injected_cus_fold_to_two_cus_with_their_own_offsets(P, clean):
    """Two runs, each with one CU injected at its own LDS dword, folded together: fold_sweep
    keeps both CUs and gives each the offset that was put into it."""
    from nanogpu.probe.selftest import fold_sweep
    from nanogpu.probe.selftest_common import cu_key

    n = clean[0]["lds_bytes"] // 4
    keys5 = sorted({cu_key(h) for x, h, *_ in clean[0]["records"] if x == 5})
    first = (3, _a_cu_on_xcd3(clean[0]["records"]), n - 257)
    second = (5, keys5[-1], 256)
    records = []
    for xcc, key, off in (first, second):
        records += list(P.cu_sweep(0, [], 8, SEED, (xcc, key, "lds", off))["records"])
    rep = fold_sweep(records, 256)
    assert rep["failed"] == [{"xcc": xcc, "cu_key": key, "kinds": ["lds"], "lds_bad_off": off}
                             for xcc, key, off in (first, second)], rep["failed"]
    assert rep["cus_seen"] == 256


# 16 B: the tail path alone; one short of 4096 elements, and 4096; the same around the kernel's own
# block of 1024 elements; full blocks plus a 3-element tail
@pytest.mark.parametrize("nbytes", [16, 4096 * 16 - 16, 4096 * 16, 1024 * 16 - 16, 1024 * 16, 1024 * 16 + 16, BIG])
def test_pattern_check_clean(P, nbytes):
    r = P.hbm_pattern_check(0, nbytes, SEED, 2)
    assert r["bytes"] == nbytes and r["errors"] == 0 and r["first"] == [], r


def test_pattern_check_finds_host_corruption(P):
    from nanogpu.probe.selftest import pattern_at

    # byte 0, the last byte, the first byte of element 4096, and the last byte before the
    # kernel's own block boundary (element 1024): four distinct elements
    corrupt = [(0, 0x01), (BIG - 1, 0x80), (4096 * 16, 0x10), (1024 * 16 - 1, 0x04)]
    r = P.hbm_pattern_check(0, BIG, SEED, 1, corrupt)
    assert r["errors"] == 4, r
    assert [f[0] for f in r["first"]] == sorted(o for o, _ in corrupt)
    xor = dict(corrupt)
    for off, expected, got in r["first"]:
        assert expected == pattern_at(off, SEED, 0)
        assert got == expected ^ (xor[off] << (8 * (off % 4)))
    r2 = P.hbm_pattern_check(0, BIG, SEED, 2, corrupt)       # each pass is corrupted and counted
    assert r2["errors"] == 8, r2
    offs = sorted(o for o, _ in corrupt)
    assert sorted(f[0] for f in r2["first"]) == sorted(offs * 2)
    for off, expected, got in r2["first"]:
        assert expected in (pattern_at(off, SEED, 0), pattern_at(off, SEED, 1))
        assert got == expected ^ (xor[off] << (8 * (off % 4)))


def test_pattern_check_wrong_seed_counts_every_element(P):
    r = P.hbm_pattern_check(0, MIB, SEED, 1, [], SEED + 1)
    assert r["errors"] == 65536, r["errors"]
    assert len(r["first"]) == 16


def test_pattern_verify_keeps_up_with_the_copy(P):
    """A copy of N bytes reads N and writes N, so a read-only check of N bytes has no reason
    to take longer: verify_gbs (bytes read per second) >= half the copy's read+write rate,
    less the 10 % run-to-run spread of streaming numbers on this box."""
    copy_gbs = P.hbm_bandwidth(0, 1 << 30, 10)
    r = P.hbm_pattern_check(0, 1 << 30, SEED, 2)
    print("copy", copy_gbs, "verify", r["verify_gbs"], "fill", r["fill_gbs"])
    record("deep_selftest_hbm_1GiB", {"copy_gbs": round(copy_gbs, 1), "verify_gbs": round(r["verify_gbs"], 1),
                                      "fill_gbs": round(r["fill_gbs"], 1)})
    assert r["errors"] == 0
    assert r["verify_gbs"] >= 0.5 * copy_gbs * 0.9, (r["verify_gbs"], copy_gbs)


def test_deep_selftest_and_agent_on_the_real_device(P):
    import asyncio

    from nanogpu.agent.metrics import render
    from nanogpu.agent.node import NodeAgent
    from nanogpu.native import core
    from nanogpu.probe.selftest import deep_selftest
    from nanogpu.topology.model import from_host_json

    rep = deep_selftest(P, 0, hbm_bytes=256 << 20)
    record("deep_selftest_256MiB", {"seconds": round(rep.seconds, 4), "launches": rep.sweep["launches"],
                                    "cus_seen": rep.sweep["cus_seen"]})
    assert rep.ok, rep.to_dict()
    assert rep.sweep["cus_seen"] == 256 and rep.hbm["bytes"] == 256 << 20 and rep.hbm["errors"] == 0
    topo = from_host_json(json.loads(core().discover_topology("", True)))
    agent = NodeAgent(api=None, node_name="box", topo=topo, device_plugin=False, selftest_deep=True,
                      selftest_hbm_mib=256)
    failed = asyncio.run(agent.selftest(P)) if len(topo.devices) == P.device_count() else []
    assert failed == [], failed
    if agent.selftest_stats:
        assert 'nanogpu_selftest_cus_checked{device="0"} 256' in render(topo, selftest=agent.selftest_stats)


# ----------------------------------------------------------------------------- bounds and small sizes
GUARD = 4096

# float4 counts around the fast path's test `base + 3 * 256 < n` (n = 768 + 1 is the first size
# at which thread 0 takes it), around one thread block's 256 threads and one block's 1,024
# elements, two blocks and a bit, and many blocks plus a 3-element tail
COPY_COUNTS = [1, 255, 256, 257, 767, 768, 769, 1023, 1024, 1025, 2049, (1 << 20) + 3]


@pytest.mark.parametrize("n4", COPY_COUNTS)
def test_copy_writes_the_destination_and_nothing_around_it(P, n4):
    r = P.copy_check(0, 4 * n4, GUARD)
    assert r == {"ok": True, "guards_ok": True, "guard_bytes_changed": 0}, (n4, r)


def test_copy_check_without_a_guard_is_still_a_bool_and_a_guard_is_whole_elements(P):
    assert P.copy_check(0, 4 * 769) is True
    assert P.copy_check(0, 4 * 769, 0) is True
    with pytest.raises(ValueError):
        P.copy_check(0, 4 * 769, 4097)
    assert "guard_ok" not in P.hbm_pattern_check(0, 16, SEED, 1)


@pytest.mark.parametrize("nbytes", [16, 4096 * 16 - 16, 4096 * 16, 1024 * 16 - 16, 1024 * 16, 1024 * 16 + 16, BIG])
def test_pattern_fill_writes_the_buffer_and_nothing_around_it(P, nbytes):
    r = P.hbm_pattern_check(0, nbytes, SEED, 2, [], None, GUARD)
    assert r["bytes"] == nbytes and r["errors"] == 0 and r["first"] == [], r
    assert r["guard_ok"] is True


def test_a_changed_guard_byte_is_reported(P):
    """The guard check itself can fail: with a guard, `corrupt` may address the guard behind
    the buffer (one pass: a second pass would flip the byte back)."""
    nbytes = 1024 * 16 + 16
    for off in (nbytes, nbytes + GUARD - 1):
        r = P.hbm_pattern_check(0, nbytes, SEED, 1, [(off, 0x01)], None, GUARD)
        assert r["errors"] == 0 and r["guard_ok"] is False, (off, r)
    with pytest.raises(ValueError):
        P.hbm_pattern_check(0, nbytes, SEED, 1, [(nbytes + GUARD, 0x01)], None, GUARD)
    with pytest.raises(ValueError):
        P.hbm_pattern_check(0, nbytes, SEED, 1, [(nbytes, 0x01)])


def test_pattern_check_wrong_seed_counts_every_element_of_a_tail(P):
    """3 full blocks and 5 elements: the last block takes hbm_verify's tail path for all of its
    threads, and the tail must count, not merely run."""
    n = 3 * 1024 + 5
    r = P.hbm_pattern_check(0, n * 16, SEED, 1, [], SEED + 1, GUARD)
    assert r["errors"] == n, r["errors"]
    assert len(r["first"]) == 16 and r["guard_ok"] is True


# ----------------------------------------------------------------------------- launch spans
# A pass is one launch after another (selftest_host.h: launch_spans), each below the 2^32
# work-items HIP supports. fill_launch_blocks / verify_launch_blocks move the seams between the
# launches, separately: a seam bug that fill and verify shared would otherwise hide itself.
SEAM_N = 7 * 1024 + 5            # elements: with 3 blocks a launch, seams at elements 3072 and 6144 and a partial last block
MAX_LAUNCH_BLOCKS = 1 << 22
GIB = 1 << 30
ODD_BLOCKS = 65535               # an odd chunk size: its seams do not sit on powers of two
ODD_CHUNK = ODD_BLOCKS * 1024 * 16


def _launches(n_elements: int, blocks: int) -> int:
    per = (blocks or MAX_LAUNCH_BLOCKS) * 1024
    return -(-n_elements // per)


@pytest.mark.parametrize("fill,verify", [(3, 3), (3, 0), (0, 3), (1, 2)])
def test_pattern_check_is_clean_across_launch_seams(P, fill, verify):
    r = P.hbm_pattern_check(0, SEAM_N * 16, SEED, 2, [], None, GUARD, fill_launch_blocks=fill,
                            verify_launch_blocks=verify)
    assert r["bytes"] == SEAM_N * 16 and r["errors"] == 0 and r["first"] == [], r
    assert r["guard_ok"] is True
    assert (r["fill_launches"], r["verify_launches"]) == (_launches(SEAM_N, fill), _launches(SEAM_N, verify))


@pytest.mark.parametrize("verify", [3, 1])
def test_split_verify_visits_every_element_exactly_once(P, verify):
    r = P.hbm_pattern_check(0, SEAM_N * 16, SEED, 1, [], SEED + 1, GUARD, fill_launch_blocks=0,
                            verify_launch_blocks=verify)
    assert r["errors"] == SEAM_N, r["errors"]
    assert len(r["first"]) == 16 and r["guard_ok"] is True
    assert r["verify_launches"] == _launches(SEAM_N, verify)


def _check_corruption(P, nbytes, corrupt, blocks, guard=0):
    """One pass with `corrupt` applied: every corrupted element is counted once and reported at its
    exact offset with the twin's expected word."""
    from nanogpu.probe.selftest import pattern_at

    assert len({o // 16 for o, _ in corrupt}) == len(corrupt) <= 16       # distinct elements, all reported
    r = P.hbm_pattern_check(0, nbytes, SEED, 1, corrupt, None, guard, fill_launch_blocks=blocks,
                            verify_launch_blocks=blocks)
    assert r["errors"] == len(corrupt), r
    assert [f[0] for f in r["first"]] == sorted(o for o, _ in corrupt)
    xor = dict(corrupt)
    for off, expected, got in r["first"]:
        assert expected == pattern_at(off, SEED, 0), hex(off)
        assert got == expected ^ (xor[off] << (8 * (off % 4))), hex(off)
    return r


def test_pattern_check_reports_corruption_on_both_sides_of_a_seam(P):
    nbytes = SEAM_N * 16
    corrupt = [(3 * 1024 * 16 - 1, 0x80), (3 * 1024 * 16, 0x01), (6 * 1024 * 16, 0x10), (nbytes - 1, 0x04)]
    r = _check_corruption(P, nbytes, corrupt, 3, GUARD)
    assert r["errors"] == 4 and r["guard_ok"] is True


def _need_free(P, nbytes):
    free, total = P.mem_info(0)
    if free < nbytes + 2 * GIB:
        pytest.skip(f"{free} of {total} bytes free: the test needs {nbytes} + 2 GiB = {nbytes + 2 * GIB}")


def test_pattern_check_across_byte_offset_2_to_the_32(P):
    nbytes = 4 * GIB + 1024 * 16 + 80
    _need_free(P, nbytes)
    seam = round((1 << 32) / ODD_CHUNK) * ODD_CHUNK                       # the launch seam nearest to 2^32
    assert 0 < abs(seam - (1 << 32)) < ODD_CHUNK // 2 and seam % 16 == 0
    corrupt = [(0, 0x01), ((1 << 32) - 1, 0x80), (1 << 32, 0x02), (seam, 0x10), (nbytes - 1, 0x04)]
    r = _check_corruption(P, nbytes, corrupt, ODD_BLOCKS)
    assert r["errors"] == 5
    assert r["fill_launches"] == r["verify_launches"] == _launches(nbytes // 16, ODD_BLOCKS) == 5
    r = P.hbm_pattern_check(0, nbytes, SEED, 2)                           # production chunking
    assert r["bytes"] == nbytes and r["errors"] == 0 and r["first"] == [], r
    assert r["fill_launches"] == r["verify_launches"] == 1


def test_pattern_check_across_word_index_2_to_the_32(P):
    """Past byte 2^34 the word index 4 i + k has a non-zero high half, so the expected words there
    are the first ones the device computes through pattern_word's `(w >> 32) * kHiMul` term."""
    from nanogpu.probe.selftest import pattern_at

    nbytes = 16 * GIB + 1024 * 16 + 80
    _need_free(P, nbytes)
    seam = round((1 << 34) / ODD_CHUNK) * ODD_CHUNK
    assert 0 < abs(seam - (1 << 34)) < ODD_CHUNK // 2 and seam % 16 == 0
    corrupt = [((1 << 34) - 1, 0x80), (1 << 34, 0x02), ((1 << 34) + 16, 0x01), (seam, 0x10), (nbytes - 1, 0x04)]
    for off in ((1 << 34), (1 << 34) + 16, nbytes - 1):                   # the high half is in these words
        assert pattern_at(off, SEED, 0) != pattern_at(off - (1 << 34), SEED, 0)
    r = _check_corruption(P, nbytes, corrupt, ODD_BLOCKS)
    assert r["fill_launches"] == r["verify_launches"] == _launches(nbytes // 16, ODD_BLOCKS) == 17
    r = P.hbm_pattern_check(0, nbytes, SEED, 2)                           # production chunking
    assert r["bytes"] == nbytes and r["errors"] == 0 and r["first"] == [], r


def test_pattern_check_past_the_first_production_launch(P):
    """64 GiB and a bit, production chunking: the second launch starts at element 2^32, the one
    size at which a `first` cut to 32 bits anywhere on its way into the pattern would show. The
    expected words there are the device's, compared with the twin's."""
    nbytes = 64 * GIB + 1024 * 16 + 80
    _need_free(P, nbytes)
    corrupt = [(0, 0x01), ((1 << 36) - 1, 0x80), (1 << 36, 0x02), ((1 << 36) + 1024 * 16, 0x10), (nbytes - 1, 0x04)]
    r = _check_corruption(P, nbytes, corrupt, 0)
    assert r["fill_launches"] == r["verify_launches"] == 2


@pytest.mark.parametrize("blocks", [-1, MAX_LAUNCH_BLOCKS + 1])
def test_launch_blocks_outside_their_range_are_refused(P, blocks):
    with pytest.raises(ValueError):
        P.hbm_pattern_check(0, 16, SEED, 1, fill_launch_blocks=blocks)
    with pytest.raises(ValueError):
        P.hbm_pattern_check(0, 16, SEED, 1, verify_launch_blocks=blocks)
    r = P.hbm_pattern_check(0, 16, SEED, 1, fill_launch_blocks=MAX_LAUNCH_BLOCKS, verify_launch_blocks=MAX_LAUNCH_BLOCKS)
    assert r["errors"] == 0


def test_a_copy_of_2_to_the_32_work_items_is_refused_before_it_allocates(P):
    """256 GiB is 2^24 blocks of 256 threads: no such launch is supported. The refusal comes
    before the buffers: two of 256 GiB do not fit the device, and a failed allocation would be
    a RuntimeError (copy_check: a MemoryError of the host's), not a ValueError."""
    with pytest.raises(ValueError):
        P.hbm_bandwidth(0, 256 << 30, 1)
    with pytest.raises(ValueError):
        P.copy_check(0, 4 << 34)
    with pytest.raises(ValueError):
        P.hbm_colocated(0, [[]], 256 << 30, 1)
    with pytest.raises(ValueError):
        P.mixed_colocated(0, [], [], 256 << 30, 1)
    if P.device_count() > 1:
        with pytest.raises(ValueError):
            P.peer_bandwidth(0, 1, 256 << 30, 1)
