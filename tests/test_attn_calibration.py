"""The attention tenant without a GPU: `attn_interference` and `tenant_call(..., "attn")` against a stand-in probe, and the
stand-alone check of nanogpu/attn_host.h (shapes, block map, every index, the replayed kernel), plain and under ASan +
UBSan."""
import json
import subprocess
import sys
from pathlib import Path

import pytest

from nanogpu.agent import cumask
from nanogpu.probe import calibrate as C

ROOT = Path(__file__).resolve().parent.parent


class StandIn:
    """Rates that tell where they come from: an attention of sq queries alone makes sq / 10 TF/s in 0.5 ms a launch and
    90 % of that beside the copy; the copy 2000 GB/s alone and 1000 + sq beside the attention."""

    def __init__(self):
        self.calls = []

    def attn_throughput(self, device, mask, heads, sq, skv, iters):
        self.calls.append(("attn_throughput", mask, (heads, sq, skv), iters))
        return {"ms": 0.5 * iters, "tflops": sq / 10, "gbs": 7.0 * sq, "kernel": "split" if sq < 128 else "wide"}

    def hbm_colocated(self, device, masks, nbytes, iters):
        self.calls.append(("hbm_colocated", masks, nbytes, iters))
        return [2000.0]

    def attn_colocated(self, device, attn_mask, hbm_mask, heads, sq, skv, attn_iters, nbytes, hbm_iters):
        self.calls.append(("attn_colocated", (attn_mask, hbm_mask), (heads, sq, skv), attn_iters, hbm_iters))
        return [0.9 * sq / 10, 1000.0 + sq]


def test_interference_runs_each_side_alone_then_twice_together_on_the_agents_masks():
    P = StandIn()
    rows = C.attn_interference(P, shapes=((8, 512, 1024), (64, 32, 2048)))
    d = cumask.DeviceCUs(256, 8)
    stream_mask, attn_mask = cumask.mask_words(d.grant("a", 25)), cumask.mask_words(d.grant("b", 75))
    assert [(r["heads"], r["sq"], r["skv"], r["kernel"]) for r in rows] == [(8, 512, 1024, "wide"), (64, 32, 2048, "split")]
    for r in rows:
        sq, skv = r["sq"], r["skv"]
        assert r["attn_tflops_alone"] == sq / 10 and r["attn_kept"] == pytest.approx(0.9) and r["attn_compulsory_gbs_alone"] == 7.0 * sq
        assert r["stream_gbs_alone"] == 2000.0 and r["stream_gbs_beside"] == 1000.0 + sq and r["stream_kept"] == (1000.0 + sq) / 2000.0
        assert r["flop_per_byte"] == pytest.approx(512 * sq * skv / (256 * (sq + 2 * skv) + 512 * sq)) and "mem_busy_percent" not in r
    # the copy alone first, then per shape: a trial, the attention alone, the copy alone, and together twice
    assert [c[0] for c in P.calls] == ["hbm_colocated"] + ["attn_throughput", "attn_throughput", "hbm_colocated", "attn_colocated", "attn_colocated"] * 2
    for c in P.calls:
        assert c[1] == {"attn_throughput": attn_mask, "hbm_colocated": [stream_mask], "attn_colocated": (attn_mask, stream_mask)}[c[0]]
    # the copy outlasts the attention in the first run together, the attention the copy in the second: one copy of
    # 1 GiB takes 2^31 B / 2000 GB/s = 1.07 ms here and one attention 0.5 ms
    together = [c for c in P.calls if c[0] == "attn_colocated"]
    for first, second in (together[:2], together[2:]):
        assert first[4] * 1.07 > 2.5 * first[3] * 0.5 and second[3] * 0.5 > 2.5 * second[4] * 1.07, (first, second)


def test_tenant_call_sizes_the_attention_from_one_trial_call():
    P = StandIn()
    call = C.tenant_call(P, "attn", [0xFF], seconds=1.0, attn=(16, 32, 256))
    assert P.calls == [("attn_throughput", [0xFF], (16, 32, 256), 4)]
    assert call() == 3.2
    assert P.calls[1] == ("attn_throughput", [0xFF], (16, 32, 256), 2000)   # 0.5 ms a launch: 2,000 in a second


@pytest.mark.parametrize("kind", ["plain", "asan"])
def test_host_program_passes(kind):
    sys.path.insert(0, str(ROOT / "native"))
    import build  # native/build.py

    assert f"attn-{kind}" in build.SELFTEST_HOST_CHOICES
    exe = build.build_selftest_host(kind, target="attn")
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr   # the program asserts the shapes, the bijection, the bounds and the replay itself
    assert json.loads(r.stdout) == {"ok": True, "lds_bytes": 73728, "wide": [128, 64, 2], "split": [32, 128, 1]}
