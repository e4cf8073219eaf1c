"""XCD check of the deep self-test: data that one XCD wrote, read on another.

The eight L2s of an MI355X are not coherent with each other, a CU's L1 is never refreshed by another CU's
stores, and atomics execute at the memory side, behind all eight XCDs. Every other check of the deep
self-test judges a line of data on the XCD that produced it; the probe's `xcd_check`
(native/hip/probe_xcd.inc) judges it somewhere else, in three groups:

* `handoff`: a write kernel fills 16 KiB a workgroup with plain stores and enters the workgroup in its XCD's
  list; the next launch verifies, from every XCD, one slice out of every XCD's list. Whenever both launches put
  a workgroup on each of two XCDs, that ordered pair is verified.
* `ticket`: workgroups 8g .. 8g+7 share a ticket. Each reads the others' 4 KiB slices (its L1 then holds them),
  overwrites its own, releases at agent scope and draws a ticket; the one that draws the last acquires and reads
  the others again, which must now hold what their owners stored. Nobody waits.
* `atomic`: adds, or, xor, min, max and a counter from every workgroup onto the same words, each on a line of its
  own; the final words are functions of the seed and the number of workgroups alone.

This module is the host twin of native/include/nanogpu/selftest_xcd_host.h (patterns, layout, expected atomic
words), the folding of the binding's result into failed ordered pairs of XCDs, and the clauses of
`DeepReport.describe_failure`. It is a check of the device, not a per-CU part: a failure names a pair of XCDs,
and a CU-mask fence cannot keep a tenant off an XCD, so it is no entry of `selftest.PARTS`.
"""
from __future__ import annotations

from types import SimpleNamespace

from .selftest_common import HI_MUL, M32, M64, cu_key, mix32, parse_names, tile_checksum

GROUPS = ("handoff", "ticket", "atomic")
KINDS = ("data", "dir", "writer", "preread", "dup")     # bit order of a section's `kinds`
XCDS = 8
THREADS = 256
MAX_ROUNDS = 4
MAX_BLOCKS = 1024
SLICE_WORDS = 4096
TICKET_WORDS = 1024
GROUP_SIZE = 8
LINE_WORDS = 32

# the atomic words, a 128-byte line each
ADD32, ADD64, XOR, UMAX, SMAX, UMIN, SMIN, COUNTER, OR_MAP = range(9)
OR_MAP_WORDS = MAX_BLOCKS // 32
SEEN_MAP = OR_MAP + OR_MAP_WORDS
SEEN_MAP_WORDS = 4 * MAX_BLOCKS // 32
ATOM_WORDS = SEEN_MAP + SEEN_MAP_WORDS
ATOM_NAMES = ("add32", "add64", "xor", "umax", "smax", "umin", "smin", "counter")

# the directory, in 32-bit words
COUNT_AT = 0
READERS_AT = COUNT_AT + XCDS * LINE_WORDS
TICKET_AT = READERS_AT + XCDS * LINE_WORDS
ATOM_AT = TICKET_AT + (MAX_BLOCKS // GROUP_SIZE) * LINE_WORDS
LIST_AT = ATOM_AT + ATOM_WORDS * LINE_WORDS
WRITER_AT = LIST_AT + XCDS * MAX_BLOCKS
MEMBER_AT = WRITER_AT + 2 * MAX_BLOCKS
DIR_WORDS = MEMBER_AT + 2 * MAX_BLOCKS
RECORD_WORDS = 36


def hand_word(seed: int, b: int, i: int) -> int:
    """Word i of workgroup b's hand-off slice."""
    return mix32(((b << 12) | i) ^ seed)


def ticket_word(seed: int, b: int, i: int, after: int) -> int:
    """Word i of workgroup b's ticket slice, before (0) or after (1: the complement) its own store."""
    v = mix32(((b << 10) | i) ^ seed ^ 0x7E1C4E70) ^ HI_MUL
    return v ^ M32 if after else v


def atom_const(seed: int, b: int, k: int) -> int:
    return mix32(mix32((b * 8 + k + 0xA7000000) & M32) ^ seed)


def atom_add64(seed: int, b: int) -> int:
    """The 64-bit addend: bit 31 of its low half is set, so the sum of any two carries across bit 32."""
    return ((atom_const(seed, b, 1) & 0xFFFF) << 32) | atom_const(seed, b, 2) | 0x80000000


def _s32(v: int) -> int:
    return v - (1 << 32) if v & 0x80000000 else v


def atom_initial(w: int) -> int:
    return {SMAX: 0x80000000, UMIN: M32, SMIN: 0x7FFFFFFF}.get(w, 0)


def atomic_expected(seed: int, n: int) -> list[int]:
    """The final atomic words after n workgroups: functions of seed and n alone."""
    w = [atom_initial(i) for i in range(ATOM_WORDS)]
    for b in range(n):
        w[ADD32] = (w[ADD32] + atom_const(seed, b, 0)) & M32
        w[ADD64] = (w[ADD64] + atom_add64(seed, b)) & M64
        w[XOR] ^= atom_const(seed, b, 3)
        w[UMAX] = max(w[UMAX], atom_const(seed, b, 4))
        w[SMAX] = max(w[SMAX], atom_const(seed, b, 5), key=_s32)
        w[UMIN] = min(w[UMIN], atom_const(seed, b, 6))
        w[SMIN] = min(w[SMIN], atom_const(seed, b, 7), key=_s32)
        w[OR_MAP + b // 32] |= 1 << (b % 32)
    w[COUNTER] = 4 * n
    for t in range(4 * n):
        w[SEEN_MAP + t // 32] |= 1 << (t % 32)
    return w


def atom_word_name(w: int) -> str:
    if w < OR_MAP:
        return ATOM_NAMES[w]
    return f"or bitmap word {w - OR_MAP}" if w < SEEN_MAP else f"counter bitmap word {w - SEEN_MAP}"


def dir_initial() -> list[int]:
    d = [0] * DIR_WORDS
    for w in range(ATOM_WORDS):
        d[ATOM_AT + w * LINE_WORDS] = atom_initial(w)
    return d


def ticket_groups(n: int) -> int:
    return (n + GROUP_SIZE - 1) // GROUP_SIZE


def group_size(n: int, g: int) -> int:
    return min(GROUP_SIZE, n - g * GROUP_SIZE)


def pick_position(n: int, count: int, q: int):
    """The list position reader ordinal q takes of an XCD with `count` writers; None without one or out of range."""
    return None if count == 0 or count > n else q % count


def _halves(words):
    return [h for w in words for h in (w & M32, w >> 32)]


def twin_summary(seed: int = 0x1234ABCD) -> dict:
    """What the stand-alone host program prints, from this module."""
    hand = [hand_word(seed, b, i) for b in (0, 5, 1023) for i in range(SLICE_WORDS)]
    tick = [ticket_word(seed, b, i, after) for b in (0, 5, 1023) for after in (0, 1) for i in range(TICKET_WORDS)]
    return {"seed": seed, "hand_checksum": tile_checksum(hand), "ticket_checksum": tile_checksum(tick),
            "atomic": {str(n): tile_checksum(_halves(atomic_expected(seed, n))) for n in (1, 3, 8, 9, 256, 1024)},
            "dir_words": DIR_WORDS, "atom_words": ATOM_WORDS, "record_words": RECORD_WORDS, "slice_bytes": 4 * SLICE_WORDS,
            "ticket_bytes": 4 * TICKET_WORDS, "dir_checksum": tile_checksum(dir_initial())}


def parse_xcd(spec) -> list[str]:
    """`parse_names` over the groups: None / "" -> [], "all", "a,b" or a list of names."""
    return parse_names(spec, GROUPS, "XCD group")


FLAG = SimpleNamespace(parse=parse_xcd, flag_noun="group")   # what the agent's flag action needs of a part


# ---- folding -----------------------------------------------------------------------------------
def _kinds(bits: int) -> list[str]:
    return [k for i, k in enumerate(KINDS) if bits >> i & 1]


def _head_ok(sec, allowed: int) -> bool:
    """xcc in range and only kinds the section's kernel can set."""
    return sec is not None and 0 <= sec[0] < XCDS and 0 <= sec[2] <= allowed and not sec[2] & ~allowed


def _first(sec, at: int):
    """(block, word, entry) of a section's first failure, None without one; ValueError when it is garbled."""
    block, wxcc, whwid, word, expected, observed = sec[at:at + 6]
    if block is None and word is None:
        return None
    if block is None or word is None or not 0 <= block < MAX_BLOCKS or not 0 <= word < SLICE_WORDS:
        raise ValueError("first failure out of range")
    return block, word, {"writer": [wxcc if wxcc is not None else -1, cu_key(whwid) if whwid is not None else -1],
                         "reader": [sec[0], cu_key(sec[1])], "block": block, "word": word,
                         "expected": expected or 0, "observed": observed or 0}


def fold_xcd(result: dict) -> dict:
    """Folds what `xcd_check` returned. Per checked group: `failed` lists the ordered pairs `[writer_xcc, reader_xcc]`
    that failed, `kinds` what failed (`data`, `dir`, `writer`, `preread`, `dup`, `record` for a garbled record, `last`
    for a ticket group without exactly one last arriver, `words` for atomic words unlike the host's), `first` the
    first failure (lowest writer block, then word) with both CUs. `pairs_seen` counts the ordered pairs a group
    verified, `pairs_verified` those of all groups together; `pairs_uncovered` lists the pairs of XCDs that appear in
    the records (as a hand-off writer and as a reader) and that `handoff` neither verified nor failed: a note, not a
    failure. `ticket_groups_bad` lists the ticket groups without exactly one last arriver, `atomic_bad` the indices of
    the atomic words unlike the host's. `ok` is false if and only if a group has a kind."""
    checked = list(result["checked"])
    records = list(result["records"])
    n = len(records)
    failed = {g: set() for g in checked}
    kinds = {g: set() for g in checked}
    first: dict = {}
    seen = {g: set() for g in checked}
    xcds: set[int] = set()

    def note_first(group, sec, at):
        try:
            f = _first(sec, at)
        except (ValueError, TypeError):
            kinds[group].add("record")
            return
        if f and (group not in first or (f[0], f[1]) < first[group][:2]):
            first[group] = f

    writers, readers = set(), set()
    for write, _read, _ticket, _atomic in records:
        if write is not None and 0 <= write[0] < XCDS:
            writers.add(write[0])
            xcds.add(write[0])
        if write is None or not 0 <= write[0] < XCDS or write[2]:
            for g in ("handoff", "ticket"):                   # both read what the write kernel left
                if g in kinds:
                    kinds[g].update(_kinds(write[2]) if _head_ok(write, 0b0010) else ["record"])
    if "handoff" in checked:
        for _write, read, _ticket, _atomic in records:
            if not _head_ok(read, 0b0111) or not 0 <= read[3] < 256 or not 0 <= read[4] < 256 or read[3] & read[4] \
                    or bool(read[2]) != bool(read[4] or read[2] & 2):
                kinds["handoff"].add("record")
                continue
            r = read[0]
            readers.add(r)
            xcds.add(r)
            kinds["handoff"].update(_kinds(read[2]))
            seen["handoff"].update((w, r) for w in range(XCDS) if read[3] >> w & 1)
            failed["handoff"].update((w, r) for w in range(XCDS) if read[4] >> w & 1)
            note_first("handoff", read, 6)
    bad_groups: list[int] = []
    if "ticket" in checked:
        lasts: dict[int, int] = {}
        for b, (_write, _read, tick, _atomic) in enumerate(records):
            g = b // GROUP_SIZE
            size = group_size(n, g)
            if not _head_ok(tick, 0b1011) or tick[3] not in (0, 1) or not 0 <= tick[6] < 256 or not 0 <= tick[7] < 256 \
                    or (tick[3] == 0 and (tick[5] or tick[6] or tick[7])) or tick[5] is None or not 0 <= tick[5] <= size - 1:
                kinds["ticket"].add("record")
                continue
            r = tick[0]
            xcds.add(r)
            kinds["ticket"].update(_kinds(tick[2]))
            if tick[3]:
                lasts[g] = lasts.get(g, 0) + 1
                if tick[5] != size - 1 and not tick[2]:
                    kinds["ticket"].add("record")         # fewer slices verified, and no failure to explain it
                seen["ticket"].update((w, r) for w in range(XCDS) if tick[6] >> w & 1)
                failed["ticket"].update((w, r) for w in range(XCDS) if tick[7] >> w & 1)
                note_first("ticket", tick, 8)
        bad_groups = [g for g in range(ticket_groups(n)) if lasts.get(g, 0) != 1]
        if bad_groups:
            kinds["ticket"].add("last")
    atomic_bad = [int(i) for i in result.get("atomic_bad", [])]
    if "atomic" in checked:
        for _write, _read, _ticket, atom in records:
            if not _head_ok(atom, 0b10010) or bool(atom[2] & 0x10) != bool(atom[3]):
                kinds["atomic"].add("record")
                continue
            xcds.add(atom[0])
            kinds["atomic"].update(_kinds(atom[2]))
        if atomic_bad:
            kinds["atomic"].add("words")
    order = list(KINDS) + ["words", "last", "record"]
    uncovered = sorted({(w, r) for w in writers for r in readers} - seen.get("handoff", set()) - failed.get("handoff", set())) \
        if "handoff" in checked else []
    every = set().union(*seen.values()) if seen else set()
    return {"checked": checked,
            "failed": {g: [list(p) for p in sorted(failed[g])] for g in checked},
            "kinds": {g: [k for k in order if k in kinds[g]] for g in checked if kinds[g]},
            "first": {g: first[g][2] for g in checked if g in first},
            "pairs_seen": {g: len(seen[g]) for g in checked},
            "pairs_verified": len(every),
            "pairs_uncovered": [list(p) for p in uncovered],
            "ticket_groups_bad": bad_groups, "atomic_bad": atomic_bad,
            "xcds": len(xcds), "blocks": n,
            "ok": not any(kinds.values())}


def _cu(c) -> str:
    return f"CU (xcc {c[0]}, key {c[1]:#x})"


_NOUN = {"handoff": "XCD hand-off", "ticket": "XCD ticket hand-off"}


def clauses(d: dict) -> list[str]:
    """The clauses of `describe_failure` for the report's `xcd` entry."""
    out = []
    for g in d.get("checked", []):
        kinds = d.get("kinds", {}).get(g)
        if not kinds:
            continue
        if g == "atomic":
            bad = d.get("atomic_bad", [])
            what = (f" at {atom_word_name(bad[0])}" + (f" and {len(bad) - 1} more" if len(bad) > 1 else "")) if bad else ""
            out.append(f"XCD atomics {'+'.join(kinds)} wrong{what}")
            continue
        f = d.get("first", {}).get(g)
        if f:
            out.append(f"{_NOUN[g]} {f['writer'][0]}->{f['reader'][0]} wrong at word {f['word']} of the slice of {_cu(f['writer'])}, "
                       f"read on {_cu(f['reader'])}" + (f", {len(d['failed'][g])} pairs failed" if len(d["failed"][g]) > 1 else ""))
        else:
            extra = f" in groups {d['ticket_groups_bad']}" if g == "ticket" and d.get("ticket_groups_bad") else ""
            out.append(f"{_NOUN[g]} {'+'.join(kinds)}{extra}")
    return out


NOTE_MISSING = "this probe has no xcd_check: nothing that crosses XCDs was checked"


def notes(d: dict) -> list[str]:
    """What is worth a note and no failure: pairs the placement left out, and a device with one XCD."""
    out = []
    if d.get("xcds", 0) <= 1:
        out.append("one XCD in the XCD check's records: nothing crosses XCDs here, the check ran CU to CU")
    if d.get("pairs_uncovered"):
        out.append(f"{len(d['pairs_uncovered'])} ordered pairs of XCDs not verified by the hand-off")
    return out


def run_xcd(P, device: int, mask: list[int], rounds: int, seed: int, names: list[str]) -> dict:
    """One `xcd_check` and its fold, as `DeepReport.xcd` keeps it."""
    res = P.xcd_check(device, mask, max(1, min(int(rounds), MAX_ROUNDS)), seed, names)
    return dict(fold_xcd(res), bytes=int(res.get("bytes", 0)), ms=float(res.get("ms", 0.0)),
                ms_kernels={k: float(v) for k, v in dict(res.get("ms_kernels", {})).items()})
