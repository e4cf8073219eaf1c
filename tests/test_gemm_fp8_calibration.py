"""The FP8 GEMM tenant without a GPU: `tenant_call(..., "gemm_fp8")` and `gemm_interference(..., dtype="fp8")` against
a stand-in probe that takes the trailing dtype, and the stand-alone check of nanogpu/gemm_fp8_host.h (shapes, the
swizzle, every index, one replay), plain and under ASan + UBSan."""
import json
import subprocess
import sys
from pathlib import Path

import pytest

from nanogpu.probe import calibrate as C

ROOT = Path(__file__).resolve().parent.parent


class StandIn:
    """0.5 ms a GEMM launch and k / 10 TF/s, 90 % of that beside the copy; every GEMM call records its dtype."""

    def __init__(self):
        self.calls = []

    def gemm_throughput(self, device, mask, m, n, k, iters, dtype="bf16"):
        self.calls.append(("gemm_throughput", mask, (m, n, k), iters, dtype))
        return {"ms": 0.5 * iters, "tflops": k / 10, "gbs": 7.0 * k, "m": m, "n": n, "k": k, "iters": iters, "dtype": dtype}

    def hbm_colocated(self, device, masks, nbytes, iters):
        return [2000.0]

    def gemm_colocated(self, device, gemm_mask, hbm_mask, m, n, k, gemm_iters, nbytes, hbm_iters, dtype="bf16"):
        self.calls.append(("gemm_colocated", (gemm_mask, hbm_mask), (m, n, k), gemm_iters, dtype))
        return [0.9 * k / 10, 1000.0 + k]


def test_tenant_call_sizes_the_fp8_gemm_from_one_trial_call():
    P = StandIn()
    call = C.tenant_call(P, "gemm_fp8", [0xFF], seconds=1.0, k=512)
    assert P.calls == [("gemm_throughput", [0xFF], (8192, 8192, 512), 4, "fp8")]
    assert call() == 51.2
    assert P.calls[1] == ("gemm_throughput", [0xFF], (8192, 8192, 512), 2000, "fp8")   # 0.5 ms a launch: 2,000 in a second


def test_interference_passes_fp8_in_every_gemm_call_and_counts_a_byte_an_element():
    P = StandIn()
    rows = C.gemm_interference(P, dtype="fp8", ks=(128, 4096))
    assert [(r["k"], r["dtype"]) for r in rows] == [(128, "fp8"), (4096, "fp8")]
    for r in rows:
        k, mn = r["k"], 8192
        assert r["flop_per_byte"] == pytest.approx(2 * mn**2 * k / (2 * k * mn + 4 * mn**2))
        assert r["gemm_tflops_alone"] == k / 10 and r["gemm_kept"] == pytest.approx(0.9) and r["stream_gbs_beside"] == 1000.0 + k
    # per k: the trial and the GEMM alone, and two runs together
    assert len(P.calls) == 2 * (2 + 2) and all(call[-1] == "fp8" for call in P.calls), P.calls


@pytest.mark.parametrize("kind", ["plain", "asan"])
def test_host_program_passes(kind):
    sys.path.insert(0, str(ROOT / "native"))
    import build  # native/build.py

    assert f"gemmfp8-{kind}" in build.SELFTEST_HOST_CHOICES
    exe = build.build_selftest_host(kind, target="gemmfp8")
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr   # the program asserts the shapes, the bounds, the bijection and the replay itself
    assert json.loads(r.stdout) == {"ok": True, "lds_bytes": 65536, "tile": [128, 128, 128]}
