"""Deep GPU self-test: every CU's MFMA pipes and LDS, and free HBM with an address pattern.

The basic self-test (agent.node.gpu_selftest) runs one wave on one CU and copies 16 MiB. This
one drives the probe's `cu_sweep` and `hbm_pattern_check` (native/hip/probe_sweep.inc, probe_hbm.inc):

* `cu_sweep` launches rounds x CUs workgroups that each hold a CU's whole LDS (so at most one
  is resident per CU and the dispatcher spreads them), run an exact bf16 MFMA chain on all 4
  waves and pattern-test the LDS. `fold_sweep` folds the per-workgroup records by CU identity
  `(xcc, (hw_id >> 8) & 0xFF)`. A CU that no workgroup reached is a coverage shortfall, not a
  failure: `deep_selftest` re-launches with doubled rounds (3 launches at most), then reports
  how many CUs it could not reach.
* `hbm_pattern_check` fills a buffer with words that are a function of their address and
  verifies it, then does the same with the complement. `pattern_word` / `pattern_at` are the
  host twin of that pattern, so a report (or a test) can state the expected value anywhere.

The optional parts are the entries of `PARTS`, each described by the `selftest_common.Part` its module
exports; `deep_selftest`, the report, the fence helpers and `main` loop over that table. `cu_sweep_paths`
(`selftest_paths.py`) takes `cu_sweep`'s place in the sweep's own launch and adds an exact chain of each
selected matrix path to every visit. `cu_sweep_valu` (`selftest_valu.py`: vector ALU, transcendentals, VGPR
file) and `cu_sweep_scalar` (`selftest_scalar.py`: scalar ALU, vector / scalar boundary, scalar loads, SGPR
file) are further launches on the same mask after each sweep launch, with records of their own, and so is
`cu_sweep_mem` (`selftest_mem.py`: the CU's memory pipeline: global and buffer loads and stores, the L1, LDS forms,
LDS-DMA, atomics), the last one.

`xcd_check` (`selftest_xcd.py`, the keyword `xcd=`) is a check of the device like the HBM check, not a part: after
the coverage loop and on the same mask it verifies on one XCD what another wrote, by a hand-off across a kernel
boundary, by release, ticket and acquire inside one kernel, and by memory-side atomics onto shared words. A
failure names a pair of XCDs, which no CU-mask fence can keep a tenant off.

What it does not cover: HBM pages and CUs held by tenants (the agent sweeps only free units
and checks HBM only on devices without a grant), the contents of L2 / Infinity Cache (whether a
handed-off line was still in L2 at the kernel's end is not claimed, nor which XCD draws a last ticket; the
write-through `sc1` forms of a hand-off are not run), and of
the matrix unit the 16x16 shapes, the sparse (smfmac) forms, bf6 operands, mixed A / B formats
and Inf and NaN operands.

`localise_failure` turns a failing sweep into CU-mask units (agent.cumask: one CU per XCD): it
runs `deep_selftest` once per candidate unit, masked to it, and says which units fail again and
which failing CUs no such unit explains. The agent fences those units (`--selftest-fence`)
instead of failing the device when `fenceable` allows it.

`python -m nanogpu.probe.selftest [--device N] [--hbm-mib M] [--paths all|LIST] [--valu all|LIST] [--scalar all|LIST] [--mem all|LIST] [--xcd all|LIST] [--json]`
prints one report;
with `--fence N` it also prints the units (at most N) an agent would fence, and changes nothing.
"""
from __future__ import annotations

import logging
import time
from dataclasses import asdict, dataclass, field, make_dataclass

from . import selftest_common, selftest_mem, selftest_paths, selftest_scalar, selftest_valu, selftest_xcd
from .selftest_common import HI_MUL, M32, Part, by_cu, coverage, cu_key, mix32, or_all, simds_seen_min

log = logging.getLogger(__name__)

PARTS: tuple[Part, ...] = (selftest_paths.PART, selftest_valu.PART, selftest_scalar.PART, selftest_mem.PART)   # in the order they launch
FAIL_LDS = 1 << 4            # fail bits 0..3: the MFMA check of wave 0..3
HBM_HEADROOM = 2 << 30       # left free by the "all free HBM" check
MAX_LAUNCHES = 3


def __getattr__(name: str):
    """The matrix-path twin and the shared helpers lived in this module before they had modules of
    their own: a name it no longer has is looked up there, so that earlier importers keep working."""
    for module in (selftest_paths, selftest_common):
        if name in vars(module):
            return vars(module)[name]
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def pattern_word(index: int, k: int, seed: int, pass_: int = 0) -> int:
    """Word k (0..3) of 16-byte element `index` in pass `pass_`: with w = 4 index + k the
    64-bit word index, mix32(lo32(w) ^ seed) ^ hi32(w) * HI_MUL; odd passes hold the complement."""
    w = 4 * index + k
    v = mix32((w & M32) ^ (seed & M32)) ^ (((w >> 32) * HI_MUL) & M32)
    return v ^ M32 if pass_ & 1 else v


def pattern_at(byte_offset: int, seed: int, pass_: int = 0) -> int:
    """The 32-bit word that holds `byte_offset` (little-endian: byte b is bits 8b..8b+7)."""
    return pattern_word(byte_offset // 16, (byte_offset % 16) // 4, seed, pass_)


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
    cus = by_cu(records)
    n_expected, uncovered, n_uncovered = coverage(cus, expected_cus)
    per_xcd: dict[int, int] = {}
    for xcc, _ in cus:
        per_xcd[xcc] = per_xcd.get(xcc, 0) + 1
    failed = []
    for k, visits in sorted(cus.items()):
        fail = or_all(fail for fail, _simds, _bad in visits)
        if fail:
            failed.append({"xcc": k[0], "cu_key": k[1], "kinds": fail_kinds(fail),
                           "lds_bad_off": min((bad for _fail, _simds, bad in visits if bad >= 0), default=-1)})
    return {"cus_seen": len(cus), "cus_expected": n_expected, "per_xcd": dict(sorted(per_xcd.items())),
            "failed": failed, "uncovered": [list(k) for k in uncovered], "cus_uncovered": n_uncovered,
            "simds_seen_min": simds_seen_min(cus, 1)}


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
    paths: dict | None = None        # {"checked": [names], "failed": {name: [[xcc, cu_key], ...]}}; None: not run
    cu_keys: list = field(default_factory=list, repr=False)   # sorted (xcc, cu_key) of every CU a record came from
    # {"checked": [names], "failed": {kind: [[xcc, cu_key], ...]}, "cus": its fold's, [s]reg_slots, "ms"}; None: not run
    valu: dict | None = field(default=None, repr=False)
    scalar: dict | None = field(default=None, repr=False)
    mem: dict | None = field(default=None, repr=False)
    xcd: dict | None = field(default=None, repr=False)       # selftest_xcd.run_xcd's; None: not run

    def to_dict(self) -> dict:
        """What /metrics and --json show: every field but `cu_keys`, as before that field existed;
        a part that did not run only where its `Part` says so (`none_in_dict`), the XCD check only where it ran."""
        d = asdict(self)
        del d["cu_keys"]
        if d["xcd"] is None:
            del d["xcd"]
        for part in PARTS:
            if d[part.key] is None and not part.none_in_dict:
                del d[part.key]
        return d

    def describe_failure(self) -> str:
        """What failed, for the agent's warning line."""
        if self.error:
            return self.error
        parts = [f"CU (xcc {f['xcc']}, key {f['cu_key']:#x}) {'+'.join(f['kinds'])}"
                 + (f" at LDS dword {f['lds_bad_off']}" if f["lds_bad_off"] >= 0 else "")
                 for f in (self.sweep or {}).get("failed", [])]
        for part, d in _part_reports(self):
            parts += part.clauses(d)
        if self.xcd and not self.xcd.get("ok", True):
            parts += selftest_xcd.clauses(self.xcd)
        if self.hbm and self.hbm.get("errors"):
            first = self.hbm.get("first") or []
            at = f", first at byte {first[0][0]} (expected {first[0][1]:#010x}, got {first[0][2]:#010x})" if first else ""
            parts.append(f"{self.hbm['errors']} HBM elements wrong{at}")
        return "; ".join(parts)


def _part_reports(report: DeepReport) -> list[tuple[Part, dict]]:
    """(part, its entry of `report`, {} where it did not run) of every part."""
    return [(part, getattr(report, part.key) or {}) for part in PARTS]


def hbm_check_takes_mask(P) -> bool:
    """Whether this probe's `hbm_pattern_check` has the `cu_mask` argument: read from the binding's
    own signature (a Python stand-in's parameters, or the signature line pybind11 puts into the doc
    string), never from an error's text, so that a refused argument stays an error."""
    import inspect

    f = P.hbm_pattern_check
    try:
        params = inspect.signature(f).parameters
    except (TypeError, ValueError):            # a built-in without a text signature: its doc string has one
        return "cu_mask" in (getattr(f, "__doc__", None) or "")
    return "cu_mask" in params or any(p.kind is p.VAR_KEYWORD for p in params.values())


def free_hbm_bytes(P, device: int, cap_mib: int = 0) -> int:
    """What the HBM check may take: the free memory less 2 GiB of headroom, capped by
    `cap_mib` when positive, in whole 16-byte elements."""
    free, _total = P.mem_info(device)
    n = max(0, int(free) - HBM_HEADROOM)
    if cap_mib > 0:
        n = min(n, cap_mib << 20)
    return n & ~15


def _hbm_check(P, device: int, hbm_bytes: int, seed: int, mask: list[int], notes: list[str]) -> dict | None:
    """`hbm_pattern_check`'s report for `hbm_bytes`, or for the half, or the quarter, where that
    much cannot be allocated; on a stream masked to `mask` when it is not empty. None where nothing
    was checked; `notes` gets every allocation that failed and a probe that takes no mask."""
    want = hbm_bytes & ~15
    for _ in range(MAX_LAUNCHES):      # memory taken by someone else meanwhile is no device fault
        if want < 16:
            break
        if mask and not hbm_check_takes_mask(P):
            notes.append("this probe's hbm_pattern_check takes no cu_mask: HBM was not checked on the masked device")
            break
        try:
            # the keyword only with a mask: a probe from before it is never called with it
            return dict(P.hbm_pattern_check(device, want, seed, 2, cu_mask=mask) if mask
                        else P.hbm_pattern_check(device, want, seed, 2))
        except MemoryError:
            notes.append(f"{want} bytes of HBM could not be allocated")
            want = (want // 2) & ~15
    return None


class Selection(make_dataclass("_PartFields", [(part.key, list, field(default_factory=list)) for part in PARTS], frozen=True)):
    """What every part of `PARTS` is to run: one field per part key (`.paths` and so on) with its list of names
    in bit order, empty where the part is off. `**vars(selection)` are the part keywords of `deep_selftest`,
    `localise_failure` and `would_fence`."""

    @classmethod
    def parse(cls, **specs) -> "Selection":
        """One spec per part key (None, "", "all", "a,b" or a list of names; a key left out is off).
        TypeError on a key that is no part, ValueError on an unknown name."""
        return cls(**{part.key: part.parse(specs.pop(part.key, None)) for part in PARTS}, **specs)


def deep_selftest(P, device: int, cu_mask_bits: list[int] | None = None, hbm_bytes: int = 0,
                  seed: int | None = None, rounds: int = 4, xcd=None, **select) -> DeepReport:
    """One deep check of HIP device `device` on the calling thread. `cu_mask_bits` restricts
    the sweep to those CU-mask bits (the agent passes the units no tenant holds; None: the
    whole chip). `hbm_bytes` > 0 adds the pattern check of that much fresh memory, on a stream
    with the same mask when one is given (a probe that cannot gets a note and no HBM check).
    `select` holds one keyword per part of `PARTS` to run (`Selection.parse`: `paths=`, `valu=`,
    `scalar=`, `mem=`, each None, "all", "a,b" or a list of names). A part without a launch of its own
    (the matrix paths) makes the sweep launches its binding instead of `cu_sweep`: still one visit
    per CU. Every other selected part adds, after each sweep launch of the coverage loop, a launch
    of its binding on the same mask, in the order of `PARTS`. A part this probe has no binding for
    gets a note and is not run. `xcd` (None, "all", "a,b" or a list of `selftest_xcd.GROUPS`) adds one `xcd_check`
    after the coverage loop and before the HBM check, on the same mask, with `rounds` capped at 4; it is no part
    of `select`, so `localise_failure`'s unit sweeps do not carry it. `ok` is false if and only if a CU failed a
    check or a name of a part, the XCD check failed, HBM errors were counted, or HIP raised."""
    from ..agent import cumask

    names = vars(Selection.parse(**select))
    xcd_names = selftest_xcd.parse_xcd(xcd)
    if seed is None:
        seed = int(time.time() * 1000) & M32   # another pattern every run
    rep = DeepReport(device=device, masked=cu_mask_bits is not None, seed=seed)
    for part in PARTS:
        if names[part.key] and not hasattr(P, part.binding):
            rep.notes.append(part.note_missing)
    active = [part for part in PARTS if names[part.key] and hasattr(P, part.binding)]
    in_sweep = next((part for part in active if part.in_sweep), None)
    swept = []                                      # the records of the sweep's launches, whichever binding made them
    records = {part.key: swept if part.in_sweep else [] for part in active}
    result = {}                                     # part key -> what its last launch returned
    t0 = time.perf_counter()
    try:
        cus = int(P.device_props(device)["cus"])
        mask = cumask.mask_words(cu_mask_bits, cus) if cu_mask_bits is not None else []
        expected = len(set(cu_mask_bits)) if cu_mask_bits is not None else cus
        launches, r = 0, rounds

        def launch(part: Part) -> dict:
            result[part.key] = getattr(P, part.binding)(device, mask, r, seed, names[part.key])
            records[part.key].extend(result[part.key]["records"])
            return result[part.key]

        while True:
            if in_sweep:
                last = launch(in_sweep)
            else:
                last = P.cu_sweep(device, mask, r, seed)
                swept.extend(last["records"])
            launches += 1
            for part in active:
                if not part.in_sweep:
                    launch(part)
            sweep = fold_sweep([rec[:5] for rec in swept], expected)
            if sweep["cus_uncovered"] == 0 or launches >= MAX_LAUNCHES:
                break
            r *= 2
        sweep.update(lds_bytes=int(last["lds_bytes"]), launches=launches, ms=float(last["ms"]))
        rep.sweep = sweep
        rep.cu_keys = sorted({(rec[0], cu_key(rec[1])) for rec in swept})
        for part in active:
            f = dict(result[part.key], **part.fold(records[part.key], result[part.key][part.names_key], expected))
            setattr(rep, part.key, {"checked": names[part.key], "failed": f["failed"], **{k: f[k] for k in part.kept}})
            rep.cu_keys = sorted(set(rep.cu_keys) | {(rec[0], cu_key(rec[1])) for rec in records[part.key]})
            if part.note_unreached and f["cus_uncovered"]:
                rep.notes.append(part.note_unreached.format(n=f["cus_uncovered"]))
        if sweep["cus_uncovered"]:
            rep.notes.append(f"{sweep['cus_uncovered']} CUs not reached in {launches} launches")
        if xcd_names and not hasattr(P, "xcd_check"):
            rep.notes.append(selftest_xcd.NOTE_MISSING)
        elif xcd_names:
            rep.xcd = selftest_xcd.run_xcd(P, device, mask, rounds, seed, xcd_names)
            rep.notes += selftest_xcd.notes(rep.xcd)
        if hbm_bytes > 0:
            rep.hbm = _hbm_check(P, device, hbm_bytes, seed, mask, rep.notes)
        rep.ok = (not sweep["failed"] and not (rep.hbm and rep.hbm["errors"]) and not (rep.xcd and not rep.xcd["ok"])
                  and not any(d.get("failed") for _part, d in _part_reports(rep)))
    except Exception as e:                     # a HIP error is a failed device
        log.exception("deep self-test of device %d raised", device)
        rep.ok, rep.error = False, f"{type(e).__name__}: {e}"
    rep.seconds = time.perf_counter() - t0
    return rep


def failed_cus(report: DeepReport) -> set[tuple[int, int]]:
    """The `(xcc, cu_key)` of every CU that failed a check or a name of any part in `report`."""
    out = {(f["xcc"], f["cu_key"]) for f in (report.sweep or {}).get("failed", [])}
    for _part, d in _part_reports(report):
        for where in (d.get("failed") or {}).values():
            out |= {(x, k) for x, k in where}
    return out


def fenceable(report: DeepReport) -> bool:
    """Whether a failed report names CUs that a CU-mask fence could keep tenants off: no HIP
    error, no HBM errors, no failed XCD check (a pair of XCDs is nothing a CU mask can avoid), no CU
    whose record is garbled (the `record` kind: then the CU's identity is as doubtful as its
    result), and at least one failed CU or path."""
    if report.error or (report.hbm and report.hbm.get("errors")) or (report.xcd and not report.xcd.get("ok", True)):
        return False
    if any("record" in f["kinds"] for f in (report.sweep or {}).get("failed", [])):
        return False
    if any("record" in (d.get("failed") or {}) for _part, d in _part_reports(report)):
        return False
    return bool(failed_cus(report))


@dataclass
class Localisation:
    bad_units: list[int] = field(default_factory=list)      # units whose own masked sweep failed
    unit_keys: dict = field(default_factory=dict)           # unit -> sorted [(xcc, cu_key)] its records came from
    unexplained: list = field(default_factory=list)         # failed CUs of the report outside every bad unit
    seconds: float = 0.0
    launches: dict = field(default_factory=dict)            # unit -> sweep launches it took
    uncovered: dict = field(default_factory=dict)           # unit -> CUs of it no launch reached (absent: 0)

    def to_dict(self) -> dict:
        return asdict(self)


def localise_failure(P, device: int, report: DeepReport, candidate_units, unit_size: int,
                     seed: int | None = None, rounds: int = 4, **select) -> Localisation:
    """Which CU-mask units hold the CUs that failed in `report`. Every unit of `candidate_units`
    (unit u is mask bits [u * unit_size, (u + 1) * unit_size)) gets one `deep_selftest` masked to
    it: the same parts (`select`, as `deep_selftest` takes them), no HBM check, and the same
    re-launch for coverage. A unit is bad when that run is not ok. `unexplained` lists the failed CUs of `report` that no bad unit's sweep
    ran on: a failure that did not come back, or a mask that does not reach where it lives.
    Either way a fence of the bad units would not cover it."""
    t0 = time.perf_counter()
    loc = Localisation()
    for u in sorted(set(candidate_units)):
        bits = [u * unit_size + k for k in range(unit_size)]
        r = deep_selftest(P, device, cu_mask_bits=bits, seed=seed, rounds=rounds, **select)
        loc.unit_keys[u] = list(r.cu_keys)
        if r.sweep:
            loc.launches[u] = r.sweep["launches"]
            if r.sweep["cus_uncovered"]:
                loc.uncovered[u] = r.sweep["cus_uncovered"]
        if not r.ok:
            loc.bad_units.append(u)
    explained = {k for u in loc.bad_units for k in loc.unit_keys[u]}
    loc.unexplained = sorted(failed_cus(report) - explained)
    loc.seconds = time.perf_counter() - t0
    return loc


def would_fence(P, device: int, report: DeepReport, max_units: int, **select) -> dict:
    """What `--fence N` prints: {"units", "cus" (unit -> its CUs), "reason" (when no unit),
    "seconds"}. Only a whole MI355X: the unit is one CU on each of its 8 XCDs."""
    from .. import types as T

    out = {"units": [], "cus": {}, "reason": "", "seconds": 0.0}
    cus = int(P.device_props(device)["cus"])
    if cus != T.MI355X_CUS:
        out["reason"] = f"{cus} CUs: the CU-mask units are measured on a whole MI355X ({T.MI355X_CUS} CUs) only"
    elif not fenceable(report):
        out["reason"] = "a HIP error, HBM errors or a garbled record are not a CU's to fence"
    else:
        loc = localise_failure(P, device, report, range(cus // T.MI355X_XCDS), T.MI355X_XCDS, **select)
        out["seconds"] = loc.seconds
        if loc.unexplained:
            out["reason"] = f"failing CUs {loc.unexplained} did not fail again in any unit"
        elif len(loc.bad_units) > max_units:
            out["reason"] = f"{len(loc.bad_units)} units fail, more than {max_units}"
        else:
            out["units"] = loc.bad_units
            out["cus"] = {str(u): [list(k) for k in loc.unit_keys[u]] for u in loc.bad_units}
    return out


def main(argv: list[str] | None = None) -> int:
    import argparse
    import json

    from ..native import probe

    ap = argparse.ArgumentParser(prog="python -m nanogpu.probe.selftest",
                                 description="deep self-test of one GPU: every CU's MFMA and LDS, and HBM")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--hbm-mib", type=int, default=1024,
                    help="HBM to pattern-check in MiB (default 1024; 0: all free memory less 2 GiB)")
    for part in PARTS:
        ap.add_argument(f"--{part.key}", default="", metavar="all|LIST", help=part.help if part.listed else argparse.SUPPRESS)
    ap.add_argument("--xcd", default="", metavar="all|LIST", help=argparse.SUPPRESS)   # groups of the XCD check
    ap.add_argument("--fence", type=int, default=0, metavar="N",
                    help="after a failed sweep, print the CU-mask units (at most N) and CUs an agent started with "
                         "--selftest-fence N would fence; changes nothing on the device or the node")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args(argv)
    try:
        select = vars(Selection.parse(**{part.key: getattr(a, part.key) for part in PARTS}))
        xcd = selftest_xcd.parse_xcd(a.xcd)
    except ValueError as e:
        ap.error(str(e))
    P = probe(required=True)
    nbytes = free_hbm_bytes(P, a.device, a.hbm_mib)
    rep = deep_selftest(P, a.device, hbm_bytes=nbytes, xcd=xcd, **select)
    plan = would_fence(P, a.device, rep, a.fence, **select) if a.fence > 0 and not rep.ok else None
    if a.json:
        print(json.dumps(dict(rep.to_dict(), fence=plan) if a.fence > 0 else rep.to_dict()))
    else:
        s, h = rep.sweep or {}, rep.hbm or {}
        print(f"device {a.device}: {'ok' if rep.ok else 'FAILED'} in {rep.seconds:.3f} s")
        if s:
            print(f"  CUs checked {s['cus_seen']}/{s['cus_expected']} (per XCD {s['per_xcd']}), "
                  f"{len(s['failed'])} failed, {s['cus_uncovered']} not reached, LDS {s['lds_bytes']} B per CU, "
                  f"sweep {s['ms']:.3f} ms in {s['launches']} launch(es)")
        for part, d in _part_reports(rep):
            if d:
                bad = d["failed"]
                print(f"  {part.label} {', '.join(d['checked'])}{part.detail.format(**d)}: "
                      + (", ".join(f"{n} failed on {len(w)} CU(s)" for n, w in sorted(bad.items())) if bad else "all clean"))
        if rep.xcd:
            x = rep.xcd
            print(f"  XCD check {', '.join(x['checked'])}: {x['pairs_verified']} ordered pair(s) of XCDs verified, {x['ms']:.3f} ms: "
                  + ("all clean" if x["ok"] else ", ".join(f"{g} {'+'.join(k)}" for g, k in x["kinds"].items())))
        if h:
            print(f"  HBM {h['bytes']} B x 2 passes: {h['errors']} errors, fill {h['fill_gbs']:.0f} GB/s, "
                  f"verify {h['verify_gbs']:.0f} GB/s, {h.get('verify_launches', 1)} launch(es) a pass")
        if not rep.ok:
            print("  " + rep.describe_failure())
        for n in rep.notes:
            print("  note: " + n)
        if plan is not None:
            if plan["units"]:
                print(f"  would fence {len(plan['units'])} unit(s) in {plan['seconds']:.3f} s:")
                for u in plan["units"]:
                    print(f"    unit {u}: " + ", ".join(f"(xcc {x}, key {k:#x})" for x, k in plan["cus"][str(u)]))
            else:
                print("  would fence nothing: " + plan["reason"])
    return 0 if rep.ok else 1


if __name__ == "__main__":
    raise SystemExit(main())
