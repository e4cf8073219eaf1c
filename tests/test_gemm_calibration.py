"""The GEMM tenant without a GPU: `gemm_interference` and `tenant_call(..., "gemm")` against a stand-in probe, and
the stand-alone check of nanogpu/gemm_host.h (tile map, shapes, every index), plain and under ASan + UBSan."""
import json
import subprocess
import sys
from pathlib import Path

import pytest

from nanogpu.agent import cumask
from nanogpu.probe import calibrate as C

ROOT = Path(__file__).resolve().parent.parent


class StandIn:
    """Rates that tell where they come from: the GEMM alone makes k / 10 TF/s and 90 % of that beside the copy; the
    copy 2000 GB/s alone and 1000 + k beside the GEMM."""

    def __init__(self):
        self.calls = []

    def gemm_throughput(self, device, mask, m, n, k, iters):
        self.calls.append(("gemm_throughput", mask, (m, n, k), iters))
        return {"ms": 0.5 * iters, "tflops": k / 10, "gbs": 7.0 * k, "m": m, "n": n, "k": k, "iters": iters}

    def hbm_colocated(self, device, masks, nbytes, iters):
        self.calls.append(("hbm_colocated", masks, nbytes, iters))
        return [2000.0]

    def gemm_colocated(self, device, gemm_mask, hbm_mask, m, n, k, gemm_iters, nbytes, hbm_iters):
        self.calls.append(("gemm_colocated", (gemm_mask, hbm_mask), (m, n, k), gemm_iters, hbm_iters))
        return [0.9 * k / 10, 1000.0 + k]


def test_interference_table_has_each_rate_in_its_column_on_the_agents_masks():
    P = StandIn()
    rows = C.gemm_interference(P, ks=(64, 4096), nbytes=1 << 30)
    d = cumask.DeviceCUs(256, 8)
    stream_mask, gemm_mask = cumask.mask_words(d.grant("a", 25)), cumask.mask_words(d.grant("b", 75))
    assert [r["k"] for r in rows] == [64, 4096]
    for r in rows:
        k = r["k"]
        assert r["gemm_tflops_alone"] == k / 10 and r["gemm_tflops_beside"] == pytest.approx(0.09 * k) and r["gemm_kept"] == pytest.approx(0.9)
        assert r["stream_gbs_alone"] == 2000.0 and r["stream_gbs_beside"] == 1000.0 + k and r["stream_kept"] == (1000.0 + k) / 2000.0
        assert r["flop_per_byte"] == pytest.approx(2 * 8192**2 * k / (4 * k * 8192 + 4 * 8192**2)) and r["gemm_compulsory_gbs_alone"] == 7.0 * k
        assert "mem_busy_percent" not in r
    for call in P.calls:
        if call[0] == "gemm_throughput":
            assert call[1] == gemm_mask and call[2][:2] == (8192, 8192)
        elif call[0] == "hbm_colocated":
            assert call[1] == [stream_mask]
        else:
            assert call[1] == (gemm_mask, stream_mask)
    # per k: the copy outlasts the GEMM in the first run together, the GEMM the copy in the second. One copy of
    # 1 GiB takes 2^31 B / 2000 GB/s = 1.07 ms here and one GEMM 0.5 ms.
    together = [c for c in P.calls if c[0] == "gemm_colocated"]
    assert len(together) == 4
    for first, second in (together[:2], together[2:]):
        assert first[4] * 1.07 > 2.5 * first[3] * 0.5 and second[3] * 0.5 > 2.5 * second[4] * 1.07, (first, second)


def test_tenant_call_sizes_the_gemm_from_one_trial_call():
    P = StandIn()
    call = C.tenant_call(P, "gemm", [0xFF], seconds=1.0, k=512)
    assert P.calls == [("gemm_throughput", [0xFF], (8192, 8192, 512), 4)]
    assert call() == 51.2
    assert P.calls[1] == ("gemm_throughput", [0xFF], (8192, 8192, 512), 2000)   # 0.5 ms a launch: 2,000 in a second


@pytest.mark.parametrize("kind", ["plain", "asan"])
def test_host_program_passes(kind):
    sys.path.insert(0, str(ROOT / "native"))
    import build  # native/build.py

    assert f"gemm-{kind}" in build.SELFTEST_HOST_CHOICES
    exe = build.build_selftest_host(kind, target="gemm")
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr   # the program asserts the bijection, the shapes and the bounds itself
    assert json.loads(r.stdout) == {"ok": True, "lds_bytes": 73728, "tile": [128, 128, 64]}
