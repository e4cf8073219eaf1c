"""What the parts of the deep self-test and its orchestration share: the hashes and checksums of the
host twins, the folding of per-visit records by CU, the parsing of name lists, and `Part`, the
description each optional part (`selftest_paths`, `selftest_valu`, `selftest_scalar`, `selftest_mem`) gives of
itself to `selftest.py`, the agent and /metrics. This module imports none of them."""
from __future__ import annotations

from dataclasses import dataclass
from functools import reduce
from operator import or_
from typing import Callable

M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1
HI_MUL = 0x9E3779B1


def mix32(x: int) -> int:
    """The fixed 32-bit finaliser the kernels use (murmur3's)."""
    x &= M32
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & M32
    x ^= x >> 16
    return x


def rotl32(x: int, r: int) -> int:
    r &= 31
    return ((x << r) | (x >> (32 - r))) & M32 if r else x & M32


def tile_checksum(words) -> int:
    """FNV-1a over the words' bytes, low byte first."""
    h = 0x811C9DC5
    for w in words:
        for b in range(4):
            h = ((h ^ ((w >> (8 * b)) & 0xFF)) * 0x01000193) & M32
    return h


def cu_key(hw_id: int) -> int:
    """CU / SH / SE bits of HW_ID: with the XCC id, a CU's identity on the chip."""
    return (hw_id >> 8) & 0xFF


def parse_names(spec, known, noun: str) -> list[str]:
    """None / "" / [] -> [], "all" -> every name of `known`, "a,b" or a list of names -> those,
    in bit order. Raises ValueError on an unknown name."""
    if not spec:
        return []
    names = list(known) if spec == "all" else [n.strip() for n in spec.split(",")] if isinstance(spec, str) else list(spec)
    bad = [n for n in names if n not in known]
    if bad or not names:
        raise ValueError(f"unknown {noun}(s) {bad}: choose from {', '.join(known)} or 'all'")
    return [n for n in known if n in names]


def coverage(seen, expected_cus) -> tuple[int, list, int]:
    """(n_expected, uncovered, n_uncovered) of the CU keys in `seen` against `expected_cus`: a set
    of `(xcc, cu_key)`, or only their number (then `uncovered` cannot be listed and is empty)."""
    if isinstance(expected_cus, int):
        return expected_cus, [], max(0, expected_cus - len(seen))
    expected = {tuple(k) for k in expected_cus}
    uncovered = sorted(expected - set(seen))
    return len(expected), uncovered, len(uncovered)


def by_cu(records) -> dict[tuple[int, int], list[list]]:
    """Records that begin `(xcc, hw_id, ...)`, grouped: `{(xcc, cu_key): [a visit's other fields, ...]}`."""
    out: dict[tuple[int, int], list[list]] = {}
    for xcc, hw_id, *rest in records:
        out.setdefault((xcc, cu_key(hw_id)), []).append(rest)
    return out


def or_all(values) -> int:
    return reduce(or_, values, 0)


def simds_seen_min(cus, field: int) -> int:
    return min((bin(or_all(v[field] for v in visits)).count("1") for visits in cus.values()), default=0)


def named_failures(cus, expected_cus, failures) -> dict:
    """The report of a fold whose failures have names. `cus` is `by_cu`'s grouping; `failures` holds,
    per failed CU in key order, `(key, the names it failed, what its entry of "cus" adds to xcc and cu_key)`."""
    n_expected, uncovered, n_uncovered = coverage(cus, expected_cus)
    failed: dict[str, list[list[int]]] = {}
    entries = []
    for (xcc, key), names, entry in failures:
        entries.append({"xcc": xcc, "cu_key": key, **entry})
        for n in names:
            failed.setdefault(n, []).append([xcc, key])
    return {"cus_seen": len(cus), "cus_expected": n_expected, "failed": failed, "cus": entries,
            "uncovered": [list(k) for k in uncovered], "cus_uncovered": n_uncovered}


@dataclass(frozen=True)
class Part:
    """One optional part of the deep self-test: everything `selftest.py`, the agent and /metrics need to
    know of it. `key` is the keyword of `deep_selftest`, the field of `DeepReport`, and the flags
    `--selftest-KEY` (agent) and `--KEY` (`python -m nanogpu.probe.selftest`)."""
    key: str
    names: tuple[str, ...]      # in the bit order of the records
    noun: str                   # of a parse error: "unknown NOUN(s) ..."
    flag_noun: str              # of the agent's flag: "name at least one FLAG_NOUN"
    binding: str                # the probe's function: (device, mask, rounds, seed, names) -> result
    names_key: str              # the key of its result that names the bits of the records
    fold: Callable              # (records, the names of the bits, expected CUs) -> {"failed", "cus_uncovered", ...}
    clauses: Callable           # its entry of the report -> its clauses of describe_failure
    label: str                  # of the printed line
    note_missing: str           # the probe has no such binding
    help: str                   # of --KEY
    agent_help: str             # of --selftest-KEY
    metric_help: str            # of nanogpu_selftest_KEY_checked
    in_sweep: bool = False      # the binding takes cu_sweep's place in the sweep's launch; else it is launched after it
    kept: tuple[str, ...] = ()  # keys of the fold's report and of the binding's result that its entry keeps
    detail: str = ""            # after the names on the printed line: a format over its entry
    note_unreached: str = ""    # a format over n, the CUs its launches did not reach
    failed_metric: tuple[str, str, str] | None = None   # (family, label, help) of a gauge of failed CUs per name
    none_in_dict: bool = False  # to_dict() shows the part, as None, when it did not run
    listed: bool = True         # --help shows its flags; False: they parse all the same

    def parse(self, spec) -> list[str]:
        """`parse_names` over this part's names."""
        return parse_names(spec, self.names, self.noun)
