"""Deep GPU self-test: every CU's MFMA pipes and LDS, and free HBM with an address pattern.

The basic self-test (agent.node.gpu_selftest) runs one wave on one CU and copies 16 MiB. This
one drives the probe's `cu_sweep` and `hbm_pattern_check` (native/hip/probe.hip):

* `cu_sweep` launches rounds x CUs workgroups that each hold a CU's whole LDS (so at most one
  is resident per CU and the dispatcher spreads them), run an exact bf16 MFMA chain on all 4
  waves and pattern-test the LDS. `fold_sweep` folds the per-workgroup records by CU identity
  `(xcc, (hw_id >> 8) & 0xFF)`. A CU that no workgroup reached is a coverage shortfall, not a
  failure: `deep_selftest` re-launches with doubled rounds (3 launches at most), then reports
  how many CUs it could not reach.
* `hbm_pattern_check` fills a buffer with words that are a function of their address and
  verifies it, then does the same with the complement. `pattern_word` / `pattern_at` are the
  host twin of that pattern, so a report (or a test) can state the expected value anywhere.

What it does not cover: HBM pages and CUs held by tenants (the agent sweeps only free units
and checks HBM only on devices without a grant), and the contents of L2 / Infinity Cache.

`python -m nanogpu.probe.selftest [--device N] [--hbm-mib M] [--json]` prints one report.
"""
from __future__ import annotations

import logging
import time
from dataclasses import asdict, dataclass, field

log = logging.getLogger(__name__)

M32 = 0xFFFFFFFF
HI_MUL = 0x9E3779B1
FAIL_LDS = 1 << 4            # fail bits 0..3: the MFMA check of wave 0..3
HBM_HEADROOM = 2 << 30       # left free by the "all free HBM" check
MAX_LAUNCHES = 3


def mix32(x: int) -> int:
    """The fixed 32-bit finaliser both kernels use (murmur3's)."""
    x &= M32
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    x ^= x >> 16
    return x


def pattern_word(index: int, k: int, seed: int, pass_: int = 0) -> int:
    """Word k (0..3) of 16-byte element `index` in pass `pass_`: with w = 4 index + k the
    64-bit word index, mix32(lo32(w) ^ seed) ^ hi32(w) * HI_MUL; odd passes hold the complement."""
    w = 4 * index + k
    v = mix32((w & M32) ^ (seed & M32)) ^ (((w >> 32) * HI_MUL) & M32)
    return v ^ M32 if pass_ & 1 else v


def pattern_at(byte_offset: int, seed: int, pass_: int = 0) -> int:
    """The 32-bit word that holds `byte_offset` (little-endian: byte b is bits 8b..8b+7)."""
    return pattern_word(byte_offset // 16, (byte_offset % 16) // 4, seed, pass_)


def cu_key(hw_id: int) -> int:
    """CU / SH / SE bits of HW_ID: with the XCC id, a CU's identity on the chip."""
    return (hw_id >> 8) & 0xFF


def fail_kinds(fail_bits: int) -> list[str]:
    kinds = []
    if fail_bits & 0xF:
        kinds.append("mfma")
    if fail_bits & FAIL_LDS:
        kinds.append("lds")
    if fail_bits & ~0x1F:
        kinds.append("record")
    return kinds


def fold_sweep(records, expected_cus) -> dict:
    """Folds `cu_sweep` records `(xcc, hw_id, fail_bits, simds, lds_bad_off)` by CU.

    `expected_cus` is the set of `(xcc, cu_key)` the sweep should reach, or, where the keys
    are not known in advance, their number. `uncovered` lists the expected keys no record came
    from (empty when only the number is known; `cus_uncovered` counts them either way). A CU is
    failed when any of its visits failed; `simds_seen_min` is the smallest number of distinct
    SIMDs any CU's waves reported."""
    seen: dict[tuple[int, int], dict] = {}
    for xcc, hw_id, fail, simds, bad in records:
        c = seen.setdefault((xcc, cu_key(hw_id)), {"fail": 0, "simds": 0, "bad": -1})
        c["fail"] |= fail
        c["simds"] |= simds
        if bad >= 0 and (c["bad"] < 0 or bad < c["bad"]):
            c["bad"] = bad
    if isinstance(expected_cus, int):
        n_expected, uncovered = expected_cus, []
        n_uncovered = max(0, n_expected - len(seen))
    else:
        expected = {tuple(k) for k in expected_cus}
        n_expected = len(expected)
        uncovered = sorted(expected - set(seen))
        n_uncovered = len(uncovered)
    per_xcd: dict[int, int] = {}
    for xcc, _ in seen:
        per_xcd[xcc] = per_xcd.get(xcc, 0) + 1
    failed = [{"xcc": k[0], "cu_key": k[1], "kinds": fail_kinds(c["fail"]), "lds_bad_off": c["bad"]}
              for k, c in sorted(seen.items()) if c["fail"]]
    return {"cus_seen": len(seen), "cus_expected": n_expected, "per_xcd": dict(sorted(per_xcd.items())),
            "failed": failed, "uncovered": [list(k) for k in uncovered], "cus_uncovered": n_uncovered,
            "simds_seen_min": min((bin(c["simds"]).count("1") for c in seen.values()), default=0)}


@dataclass
class DeepReport:
    device: int
    ok: bool = True
    seconds: float = 0.0
    sweep: dict | None = None        # fold_sweep's report + lds_bytes, launches, ms (last launch)
    hbm: dict | None = None          # hbm_pattern_check's report; None when not run
    error: str | None = None         # a HIP exception: the device failed
    masked: bool = False             # swept only the CUs in `cu_mask_bits`
    seed: int = 0
    notes: list[str] = field(default_factory=list)

    def to_dict(self) -> dict:
        return asdict(self)

    def describe_failure(self) -> str:
        """What failed, for the agent's warning line."""
        if self.error:
            return self.error
        parts = [f"CU (xcc {f['xcc']}, key {f['cu_key']:#x}) {'+'.join(f['kinds'])}"
                 + (f" at LDS dword {f['lds_bad_off']}" if f["lds_bad_off"] >= 0 else "")
                 for f in (self.sweep or {}).get("failed", [])]
        if self.hbm and self.hbm.get("errors"):
            first = self.hbm.get("first") or []
            at = f", first at byte {first[0][0]} (expected {first[0][1]:#010x}, got {first[0][2]:#010x})" if first else ""
            parts.append(f"{self.hbm['errors']} HBM elements wrong{at}")
        return "; ".join(parts)


def free_hbm_bytes(P, device: int, cap_mib: int = 0) -> int:
    """What the HBM check may take: the free memory less 2 GiB of headroom, capped by
    `cap_mib` when positive, in whole 16-byte elements."""
    free, _total = P.mem_info(device)
    n = max(0, int(free) - HBM_HEADROOM)
    if cap_mib > 0:
        n = min(n, cap_mib << 20)
    return n & ~15


def deep_selftest(P, device: int, cu_mask_bits: list[int] | None = None, hbm_bytes: int = 0,
                  seed: int | None = None, rounds: int = 4) -> DeepReport:
    """One deep check of HIP device `device` on the calling thread. `cu_mask_bits` restricts
    the sweep to those CU-mask bits (the agent passes the units no tenant holds; None: the
    whole chip). `hbm_bytes` > 0 adds the pattern check of that much fresh memory. `ok` is
    false if and only if a CU failed a check, HBM errors were counted, or HIP raised."""
    from ..agent import cumask

    if seed is None:
        seed = int(time.time() * 1000) & M32   # another pattern every run
    rep = DeepReport(device=device, masked=cu_mask_bits is not None, seed=seed)
    t0 = time.perf_counter()
    try:
        cus = int(P.device_props(device)["cus"])
        mask = cumask.mask_words(cu_mask_bits, cus) if cu_mask_bits is not None else []
        expected = len(set(cu_mask_bits)) if cu_mask_bits is not None else cus
        records, launches, r, last = [], 0, rounds, {}
        while True:
            last = P.cu_sweep(device, mask, r, seed)
            launches += 1
            records.extend(last["records"])
            sweep = fold_sweep(records, expected)
            if sweep["cus_uncovered"] == 0 or launches >= MAX_LAUNCHES:
                break
            r *= 2
        sweep.update(lds_bytes=int(last["lds_bytes"]), launches=launches, ms=float(last["ms"]))
        rep.sweep = sweep
        if sweep["cus_uncovered"]:
            rep.notes.append(f"{sweep['cus_uncovered']} CUs not reached in {launches} launches")
        if hbm_bytes > 0:
            want = hbm_bytes & ~15
            for _ in range(MAX_LAUNCHES):      # memory taken by someone else meanwhile is no device fault
                if want < 16:
                    break
                try:
                    rep.hbm = dict(P.hbm_pattern_check(device, want, seed, 2))
                    break
                except MemoryError:
                    rep.notes.append(f"{want} bytes of HBM could not be allocated")
                    want = (want // 2) & ~15
        rep.ok = not sweep["failed"] and not (rep.hbm and rep.hbm["errors"])
    except Exception as e:                     # a HIP error is a failed device
        log.exception("deep self-test of device %d raised", device)
        rep.ok, rep.error = False, f"{type(e).__name__}: {e}"
    rep.seconds = time.perf_counter() - t0
    return rep


def main(argv: list[str] | None = None) -> int:
    import argparse
    import json

    from ..native import probe

    ap = argparse.ArgumentParser(prog="python -m nanogpu.probe.selftest",
                                 description="deep self-test of one GPU: every CU's MFMA and LDS, and HBM")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--hbm-mib", type=int, default=1024,
                    help="HBM to pattern-check in MiB (default 1024; 0: all free memory less 2 GiB)")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args(argv)
    P = probe(required=True)
    nbytes = free_hbm_bytes(P, a.device, a.hbm_mib)
    rep = deep_selftest(P, a.device, hbm_bytes=nbytes)
    if a.json:
        print(json.dumps(rep.to_dict()))
    else:
        s, h = rep.sweep or {}, rep.hbm or {}
        print(f"device {a.device}: {'ok' if rep.ok else 'FAILED'} in {rep.seconds:.3f} s")
        if s:
            print(f"  CUs checked {s['cus_seen']}/{s['cus_expected']} (per XCD {s['per_xcd']}), "
                  f"{len(s['failed'])} failed, {s['cus_uncovered']} not reached, LDS {s['lds_bytes']} B per CU, "
                  f"sweep {s['ms']:.3f} ms in {s['launches']} launch(es)")
        if h:
            print(f"  HBM {h['bytes']} B x 2 passes: {h['errors']} errors, fill {h['fill_gbs']:.0f} GB/s, "
                  f"verify {h['verify_gbs']:.0f} GB/s")
        if not rep.ok:
            print("  " + rep.describe_failure())
        for n in rep.notes:
            print("  note: " + n)
    return 0 if rep.ok else 1


if __name__ == "__main__":
    raise SystemExit(main())
