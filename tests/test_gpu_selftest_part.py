"""The sweep's dynamic-LDS kernels on a real MI355X (`pytest -m gpu`). The occupancy query there
always answers that a block may hold a CU's whole 160 KiB, so the instantiations with `n` dwords
of dynamic LDS run only through the `lds_bytes` test hook of `cu_sweep` / `cu_sweep_paths`: clean
at the smallest legal sizes, comparing (a corrupted expected word fails every record), with the
dynamic `n` reaching the LDS test, and with illegal sizes rejected before anything is launched.
Several small workgroups share a CU, so none of this asks for a visit of every CU. Corruption is
applied to data the kernel owns or to the host's upload; nothing here makes the device fault."""
from collections import Counter

import pytest

pytestmark = pytest.mark.gpu

SEED = 0x1234ABCD
STAGED = 36864            # 4 * kNumPaths * kTileWords: the nine expected tiles staged in LDS
WORKGROUPS = 4 * 256      # rounds = 4, unmasked


@pytest.fixture(scope="module")
def P():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    from nanogpu.native import probe

    return probe(required=True)


def _paths():
    from nanogpu.probe.selftest_paths import PATHS

    return list(PATHS)


@pytest.fixture(scope="module")
def clean_plain(P):
    """cu_sweep at the staging size, shared by the clean case and the injection."""
    return P.cu_sweep(0, [], 4, SEED, lds_bytes=STAGED)


def _assert_clean(r, lds_bytes, fields):
    recs = r["records"]
    assert r["lds_bytes"] == lds_bytes
    assert len(recs) == WORKGROUPS and all(len(x) == fields for x in recs)      # an unwritten record raises
    bad = [x for x in recs if x[2] or x[4] != -1 or any(x[5:])]
    assert bad == [], bad[:4]


def test_plain_part_kernel_is_clean_at_16_bytes(P):
    _assert_clean(P.cu_sweep(0, [], 4, SEED, lds_bytes=16), 16, 5)


def test_plain_part_kernel_is_clean_at_the_staging_size(clean_plain):
    _assert_clean(clean_plain, STAGED, 5)


@pytest.mark.parametrize("lds_bytes", [STAGED, 65536])
def test_path_part_kernel_is_clean(P, lds_bytes):
    """At 36,864 bytes the tile staging and the LDS pattern test share every dword."""
    r = P.cu_sweep_paths(0, [], 4, SEED, _paths(), lds_bytes=lds_bytes)
    _assert_clean(r, lds_bytes, 7)
    assert list(r["paths"]) == _paths() and list(r["checked"]) == _paths()


def test_plain_part_kernel_compares_the_bf16_tile(P):
    r = P.cu_sweep(0, [], 4, SEED, corrupt_expected=(0, 1), lds_bytes=16)
    assert len(r["records"]) == WORKGROUPS
    assert all(x[2] & 0xF == 0xF for x in r["records"]), [x for x in r["records"] if x[2] & 0xF != 0xF][:4]


@pytest.mark.parametrize("flip", [("mxfp8", 1023, 1 << 31), ("f64", 511, 1)], ids=["mxfp8", "f64"])
def test_path_part_kernel_compares_the_path_tiles(P, flip):
    bit = 1 << _paths().index(flip[0])
    r = P.cu_sweep_paths(0, [], 4, SEED, _paths(), corrupt_expected=flip, lds_bytes=STAGED)
    assert len(r["records"]) == WORKGROUPS
    wrong = [x for x in r["records"] if not (x[5] & bit and x[6] == 0xF and x[2] == 0 and x[4] == -1)]
    assert wrong == [], wrong[:4]


def test_the_dynamic_size_reaches_the_lds_test(P, clean_plain):
    """The last dword of a 9,216-dword array, on the CU the clean run visited most often."""
    from nanogpu.probe.selftest import fold_sweep
    from nanogpu.probe.selftest_common import cu_key

    n = STAGED // 4
    (xcc, key), _visits = Counter((x[0], cu_key(x[1])) for x in clean_plain["records"]).most_common(1)[0]
    r = P.cu_sweep(0, [], 16, SEED, (xcc, key, "lds", n - 1), lds_bytes=STAGED)
    visited = {(x[0], cu_key(x[1])) for x in r["records"]}
    assert (xcc, key) in visited, f"CU (xcc {xcc}, key {key:#x}) got none of the {len(r['records'])} workgroups"
    rep = fold_sweep(r["records"], len(visited))
    assert rep["failed"] == [{"xcc": xcc, "cu_key": key, "kinds": ["lds"], "lds_bad_off": n - 1}], rep["failed"]
    with pytest.raises(ValueError):
        P.cu_sweep(0, [], 16, SEED, (xcc, key, "lds", n), lds_bytes=STAGED)


@pytest.mark.parametrize("lds_bytes", [0, 8, 24, 65552])
def test_illegal_sizes_are_rejected(P, lds_bytes):
    with pytest.raises(ValueError):
        P.cu_sweep(0, [], 4, SEED, lds_bytes=lds_bytes)
    with pytest.raises(ValueError):
        P.cu_sweep_paths(0, [], 4, SEED, _paths(), lds_bytes=lds_bytes)


def test_the_path_sweep_needs_room_for_its_tiles(P):
    with pytest.raises(ValueError):
        P.cu_sweep_paths(0, [], 4, SEED, _paths(), lds_bytes=STAGED - 16)
