"""The deep self-test's policy for coverage, `launch_until_covered`, and the GPU tests' `sweep_all` on top of it,
without a GPU: how often and with which rounds a launch is made, what is folded, and that `sweep_all` hands every
part's binding its arguments in the binding's order and folds under the part's own `names_key`."""
import pytest

from gpu_harness import SEED, sweep_all, unit_mask   # tests/ is on sys.path (no package)
from nanogpu.probe import selftest as S

KEYS = [(i % 8, i // 8) for i in range(256)]


def _hw(key):
    return key << 8


# ----------------------------------------------------------------------------- launch_until_covered
@pytest.mark.parametrize("covered_at,rounds", [(1, [4]), (2, [4, 8]), (None, [4, 8, 16])], ids=["at-once", "second", "never"])
def test_launches_with_doubled_rounds_until_covered_or_the_limit(covered_at, rounds):
    calls, folded = [], []

    def launch(r):
        calls.append(r)
        return [("launch", len(calls), k) for k in range(3)]            # three records a launch, each naming its launch

    def fold(records):
        folded.append(list(records))
        return {"cus_uncovered": 0 if len(calls) == covered_at else 1, "records": list(records)}

    report, launches = S.launch_until_covered(launch, fold, 4)
    assert calls == rounds and launches == len(rounds) <= S.MAX_LAUNCHES
    assert (covered_at is None) == (launches == S.MAX_LAUNCHES)
    everything = [("launch", n + 1, k) for n in range(launches) for k in range(3)]
    assert report["records"] == everything                                # the returned fold is the fold of all records
    assert folded == [everything[:3 * (n + 1)] for n in range(launches)]  # one fold a launch, of everything so far


def test_other_rounds_and_limits():
    calls = []
    report, launches = S.launch_until_covered(lambda r: calls.append(r) or [], lambda recs: {"cus_uncovered": 1}, 3, max_launches=4)
    assert calls == [3, 6, 12, 24] and launches == 4 and report == {"cus_uncovered": 1}


# ----------------------------------------------------------------------------- sweep_all over a stand-in probe
CLEAN = {"paths": (0, 0xF, -1, 0, 0), "valu": (0, 0xF, 0, -1, -1, 0x1234), "scalar": (0, 0xF, 0, -1, -1, -1),
         "mem": (0, 0xF, 0, -1, -1, -1)}            # a clean record of each part's binding, after (xcc, hw_id)


class _Probe:
    """Every part's binding with the parameters the real one has, in its order. Each keeps its arguments; launches
    below `shy_below` rounds leave out the first CU of the mask."""

    def __init__(self, shy_below=0):
        self.shy_below, self.calls = shy_below, []

    def _launch(self, part, dev, mask, rounds, seed, names, inject, corrupt_expected):
        self.calls.append((part.binding, dev, mask, rounds, seed, names, inject, corrupt_expected))
        keys = [k for i, k in enumerate(KEYS) if not mask or (mask[i // 32] >> (i % 32)) & 1]
        if rounds < self.shy_below:
            keys = keys[1:]
        # the names of the bits come back in full under the part's own key, whatever was asked for
        return {"records": [(x, _hw(k)) + CLEAN[part.key] for x, k in keys], part.names_key: list(part.names), "checked": list(names),
                "ms": 0.5, "rounds": rounds}

    def cu_sweep_paths(self, device=0, cu_mask=(), rounds=4, seed=0, paths=(), inject=None, corrupt_expected=None, lds_bytes=None):
        return self._launch(S.selftest_paths.PART, device, cu_mask, rounds, seed, paths, inject, corrupt_expected)

    def cu_sweep_valu(self, device=0, cu_mask=(), rounds=4, seed=0, groups=(), inject=None, corrupt_expected=None):
        return self._launch(S.selftest_valu.PART, device, cu_mask, rounds, seed, groups, inject, corrupt_expected)

    def cu_sweep_scalar(self, device=0, cu_mask=(), rounds=4, seed=0, groups=(), inject=None, corrupt_expected=None):
        return self._launch(S.selftest_scalar.PART, device, cu_mask, rounds, seed, groups, inject, corrupt_expected)

    def cu_sweep_mem(self, device=0, cu_mask=(), rounds=4, seed=0, groups=(), inject=None, corrupt_expected=None):
        return self._launch(S.selftest_mem.PART, device, cu_mask, rounds, seed, groups, inject, corrupt_expected)


@pytest.mark.parametrize("part", S.PARTS, ids=[p.key for p in S.PARTS])
def test_sweep_all_calls_the_parts_binding_in_its_order_and_folds_by_its_names(part):
    P = _Probe()
    names = part.names[1:3]
    r, f = sweep_all(P, part, names, inject=(3, 5, "x"), corrupt=("y", 1, 2))
    assert P.calls == [(part.binding, 0, [], 4, SEED, list(names), (3, 5, "x"), ("y", 1, 2))]
    assert len(r["records"]) == 256 and r["checked"] == list(names) and r[part.names_key] == list(part.names)
    assert f["cus_seen"] == 256 and f["cus_expected"] == 256 and f["cus_uncovered"] == 0 and f["failed"] == {}

    P = _Probe()
    mask = unit_mask(5)
    r, f = sweep_all(P, part, part.names, 2, mask=mask, cus=8)
    assert P.calls == [(part.binding, 0, mask, 2, SEED, list(part.names), None, None)]
    assert f["cus_seen"] == f["cus_expected"] == 8 and {(rec[0], rec[1] >> 8) for rec in r["records"]} == {(x, 5) for x in range(8)}

    P = _Probe(shy_below=16)               # two launches miss a CU: three launches, and the records of all three
    r, f = sweep_all(P, part, part.names)
    assert [c[3] for c in P.calls] == [4, 8, 16] and len(r["records"]) == 255 + 255 + 256
    assert r["rounds"] == 4 and f["cus_seen"] == 256 and f["cus_uncovered"] == 0

    P = _Probe(shy_below=32)               # never covered: `MAX_LAUNCHES` launches and the shortfall in the fold
    r, f = sweep_all(P, part, part.names)
    assert len(P.calls) == S.MAX_LAUNCHES and f["cus_seen"] == 255 and f["cus_uncovered"] == 1 and f["failed"] == {}
