"""What the GPU test files (tests/test_gpu*.py) share: the probe fixture, the file of measured facts, a sweep
of one `Part` under `deep_selftest`'s own policy for coverage, and the CUs and masks the tests pick. No test
in here, and nothing that needs a GPU to import."""
import json
from pathlib import Path

import pytest

from nanogpu.probe.selftest_common import cu_key

SEED = 0x1234ABCD


def record(key: str, value) -> None:
    """Measured facts for profiles/gpu_calibration.md (merged back from the GPU box)."""
    p = Path("gpurun_out/gpu_facts.json")
    p.parent.mkdir(exist_ok=True)
    d = json.loads(p.read_text()) if p.exists() else {}
    d[key] = value
    p.write_text(json.dumps(d, indent=1))


@pytest.fixture(scope="module")
def P():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    from nanogpu.native import probe

    return probe(required=True)  # fails loudly if the HIP extension is missing


def sweep_all(P, part, names, rounds=4, inject=None, corrupt=None, mask=(), cus=256):
    """One sweep of `part` (a `selftest_common.Part`) on device 0, unmasked or of the `cus` CUs of `mask`, launched
    by `launch_until_covered` as `deep_selftest` launches it. Returns (the first launch's result with the records of
    every launch, `part.fold` of those records)."""
    from nanogpu.probe.selftest import launch_until_covered

    launched = []

    def launch(r):
        launched.append(getattr(P, part.binding)(0, list(mask), r, SEED, list(names), inject, corrupt))
        return launched[-1]["records"]

    fold, _launches = launch_until_covered(launch, lambda records: part.fold(records, launched[0][part.names_key], cus), rounds)
    return dict(launched[0], records=[rec for r in launched for rec in r["records"]]), fold


def a_cu(records) -> tuple[int, int]:
    """The CU the injections of a part go to: `(xcc, cu_key)` of the record a third of the way in."""
    rec = records[len(records) // 3]
    return rec[0], cu_key(rec[1])


def a_cu_on_xcd3(records) -> int:
    """The CU key the injections of the sweep and the paths go to: the sixth of those seen on XCD 3."""
    return sorted({cu_key(rec[1]) for rec in records if rec[0] == 3})[5]


def unit_mask(unit: int) -> list[int]:
    """The mask words of one CU-mask unit of a whole MI355X: 8 bits of 256, one CU on each XCD."""
    from nanogpu.agent import cumask

    return cumask.mask_words(list(range(unit * 8, (unit + 1) * 8)), 256)


def census_keys(P, mask) -> set[tuple[int, int]]:
    """Which CUs a mask is: what the census kernel reports from a stream with the same mask."""
    return {(xcc, cu_key(hw_id)) for xcc, hw_id in P.cu_census(0, mask, 512, 64)}


def assert_fails_exactly(part, checked, fold, cu, name):
    """The tail of every injection test. `fold` is `sweep_all`'s of a sweep with one fault injected on `cu`: exactly
    that CU failed exactly `name`, every CU was still seen, and the report with that entry for `part` is a CU's to
    fence. Returns the report."""
    from nanogpu.probe import selftest as S

    assert fold["failed"] == {name: [list(cu)]}, fold["failed"]
    assert fold["cus_seen"] == 256
    rep = S.DeepReport(device=0, ok=False, **{part.key: {"checked": list(checked), "failed": fold["failed"], "cus": fold["cus"]}})
    assert S.fenceable(rep) and S.failed_cus(rep) == {cu}
    return rep
