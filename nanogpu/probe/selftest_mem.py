"""Memory part of the deep self-test: the Python twin of native/include/nanogpu/selftest_mem_host.h.

`cu_sweep_mem` (native/hip/probe_mem.inc) makes all four waves of every CU run the memory pipeline: global
loads of every width and extension (`gload`), the whole 32 KiB table twice through the CU's L1 (`l1`),
global stores of every width over a background (`gstore`), raw buffer loads and stores with lanes in
and out of range (`buffer`), the LDS instruction forms (`lds`), the transposed LDS read (`ldstr`),
LDS-DMA (`ldsdma`) and atomics with return on global memory and LDS (`atomic`). Every result word a
lane gets is compared in the kernel with the value computed from its index.

This module computes the same words another way: it keeps the table, each wave's region of the
workgroup's slice and of LDS as byte arrays and executes every instruction on them from its
definition in the CDNA ISA (one function per instruction kind), never from a device's output. It
also folds the records by CU (`fold_mem`).

Operand corners whose definition is not established independently are kept out (the functions raise
on them) and are listed under "Not covered" in the README: what a d16 load leaves in the other half
of its register, sub-dword and 12-byte LDS-DMA, the `_tr_b8` / `_tr_b4` / `_tr_b6` reads, partly
out-of-range buffer accesses and whether soffset takes part in the range check, strided or swizzled
descriptors and typed formats, float and packed atomics, misaligned accesses.
"""
from __future__ import annotations

from .selftest_common import M32, Part, by_cu, mix32, named_failures, parse_names, simds_seen_min, tile_checksum

GROUPS = ("gload", "l1", "gstore", "buffer", "lds", "ldstr", "ldsdma", "atomic")   # bit order of the records
TABLE_GROUPS = ("gload", "l1", "ldsdma")         # their compared values come from the table
WAVES, LANES = 4, 64
MEM_WORDS = 8192
SALT = 0x3E3D7A11
SLICE_BYTES, WAVE_BYTES, LDS_WAVE_BYTES = 8192, 2048, 16384
RECORD_WORDS = 8
BUF_RECORDS, BUF_SOFFSET, BUF_IMM = 1024, 64, 48
LDS_UPPER = 4096
DMA_BG = 0xDEADD0D0
NO_Q = -1


def parse_mem(spec) -> list[str]:
    """`parse_names` over `GROUPS`: None / "" -> [], "all", "a,b" or a list of names; ValueError on an unknown one."""
    return parse_names(spec, GROUPS, "memory group")


def table_word(i: int) -> int:
    return mix32(i ^ SALT)


def val(tag: int, wave: int, lane: int, a: int, b: int) -> int:
    return mix32(tag ^ (wave << 28) ^ (lane << 20) ^ (a << 8) ^ b)


# ---- memory and the instructions ---------------------------------------------------------------
class Memory:
    """`size` bytes, little-endian."""

    def __init__(self, size: int, words=None):
        self.b = bytearray(size)
        for i, w in enumerate(words or ()):
            self.b[4 * i:4 * i + 4] = w.to_bytes(4, "little")

    def _range(self, at: int, n: int, align: int | None = None):
        align = (16 if n == 12 else n) if align is None else align
        if at % align:
            raise ValueError(f"a misaligned access ({n} bytes at {at}) is left out")
        if at < 0 or at + n > len(self.b):
            raise IndexError(f"{n} bytes at {at} leave the {len(self.b)} bytes")
        return slice(at, at + n)

    def load(self, at: int, n: int, align: int | None = None) -> int:
        return int.from_bytes(self.b[self._range(at, n, align)], "little")

    def store(self, at: int, n: int, value: int, align: int | None = None) -> None:
        self.b[self._range(at, n, align)] = (value & ((1 << (8 * n)) - 1)).to_bytes(n, "little")

    def words(self, at: int, n: int, align: int | None = None) -> list[int]:
        v = self.load(at, 4 * n, align)
        return [(v >> (32 * j)) & M32 for j in range(n)]


def sext(v: int, bits: int) -> int:
    return (v - (1 << bits) if v >> (bits - 1) else v) & M32


def load_ext(mem: Memory, at: int, n: int, signed: bool) -> int:
    """global_load_{u,s}{byte,short}, ds_read_{u,i}{8,16}: n bytes zero- or sign-extended to 32 bits."""
    v = mem.load(at, n)
    return sext(v, 8 * n) if signed else v


def load_d16(mem: Memory, at: int, n: int, signed: bool) -> int:
    """The 16 bits a d16 load writes into the half of the register it names: n bytes extended to 16 bits."""
    return load_ext(mem, at, n, signed) & 0xFFFF


def pack(words) -> int:
    return sum(w << (32 * j) for j, w in enumerate(words))


def buffer_lane(voffset: int, soffset: int, imm: int, n: int, num_records: int) -> bool:
    """Whether a raw (stride 0) buffer access of n bytes is in range. Raises where the definition is not established."""
    inside = voffset + imm + soffset + n <= num_records
    outside = voffset + imm >= num_records
    if inside == outside:
        raise ValueError("a partly out-of-range buffer access, or one that soffset alone decides, is left out")
    return inside


def tr_b16(mem: Memory, addrs) -> list[list[int]]:
    """ds_read_b64_tr_b16 on the wave's 64 lane addresses: per 16-lane group, lane 4q + p supplies row q, columns
    4p .. 4p + 3 of a 4 x 16 block of 16-bit elements; lane i receives column i, row q in element q."""
    if len(addrs) != LANES:
        raise ValueError("the transposed read with a lane masked off is left out")
    for a in addrs:
        mem.load(a, 8)                            # every lane's 8 bytes are aligned to 8 and inside
    out = []
    for lane in range(LANES):
        g, i = lane // 16, lane % 16
        elems = [mem.load(addrs[16 * g + 4 * q + i // 4] + 2 * (i % 4), 2) for q in range(4)]
        out.append([elems[0] | elems[1] << 16, elems[2] | elems[3] << 16])
    return out


def lds_dma_dest(base: int, lane: int, n: int) -> int:
    """Where LDS-DMA puts lane `lane`'s n bytes: the wave-uniform base + lane x n."""
    if n not in (4, 16):
        raise ValueError("LDS-DMA of 1, 2 or 12 bytes a lane is left out")
    return base + lane * n


ATOMIC32 = ("add", "sub", "smin", "umin", "smax", "umax", "and", "or", "xor", "inc", "dec", "swap", "cmpswap")
ATOMIC64 = ("add", "umax", "swap", "cmpswap")
ATOMICS = [(n, 32) for n in ATOMIC32] + [(n, 64) for n in ATOMIC64]


def atomic(op: str, bits: int, old: int, v: int, cmp: int = 0) -> int:
    """What the location holds after the atomic; it returns `old`. inc: old >= v ? 0 : old + 1. dec: old == 0 or
    old > v ? v : old - 1. cmpswap: old == cmp ? v : old."""
    m = (1 << bits) - 1
    sg = (lambda x: x - (1 << bits) if x >> (bits - 1) else x)
    return {"add": lambda: (old + v) & m, "sub": lambda: (old - v) & m,
            "smin": lambda: old if sg(old) < sg(v) else v, "umin": lambda: min(old, v),
            "smax": lambda: old if sg(old) > sg(v) else v, "umax": lambda: max(old, v),
            "and": lambda: old & v, "or": lambda: old | v, "xor": lambda: old ^ v,
            "inc": lambda: 0 if old >= v else old + 1, "dec": lambda: v if old == 0 or old > v else old - 1,
            "swap": lambda: v, "cmpswap": lambda: v if old == cmp else old}[op]()


# ---- the groups: the lane maps, as the header states them --------------------------------------
GLOAD_FORMS = ([("byte", False, s) for s in range(4)] + [("byte", True, s) for s in range(4)]
               + [("short", False, 0), ("short", False, 2), ("short", True, 0), ("short", True, 2)]
               + [("d16", 1, False, 1), ("d16", 1, False, 2), ("d16", 1, True, 3), ("d16", 1, True, 0), ("d16", 2, False, 2), ("d16", 2, False, 0)]
               + [("words", 1), ("words", 2), ("words", 3)] + [("words", 4)] * 5)     # the last four: nt, sc0, sc1, sc0 sc1


def gload_chunk(map_: int, wave: int, lane: int, f: int) -> int:
    if map_ == 0:
        return 16 * ((wave * 64 + lane + 61 * f) & 2047)
    return 128 * ((lane * 5 + wave * 64 + 3 * f) & 255) + 16 * ((lane + f) & 7)


def l1_chunk(pass_: int, step: int, lane: int) -> int:
    return step * 64 + lane if pass_ == 0 else (31 - step) * 64 + ((lane * 17 + step) & 63)


GSTORE_BYTES = (1, 2, 2, 4, 8, 12, 16)       # byte, short, short_d16_hi, dword, x2, x3, x4


def gstore_chunk(wave: int, lane: int, f: int) -> int:
    return 16 * ((lane * 13 + f * 7 + wave) & 63)


def gstore_sub(lane: int, f: int) -> int:
    return ((lane + 5) & 15, 2 * (lane & 7), 2 * ((lane + 3) & 7), 4 * (lane & 3), 8 * (lane & 1), 0, 0)[f]


BUF_BYTES = (1, 2, 4, 8, 12, 16)


def buf_stride(w: int) -> int:
    return 16 if w == 4 else BUF_BYTES[w]


def buf_operands(w: int, m: int, lane: int) -> tuple[int, int, int]:
    """(voffset, soffset, immediate) of width w in mode m (0 offen, 1 soffset, 2 immediate)."""
    s = buf_stride(w)
    addr = BUF_RECORDS - 32 * s + lane * s + (BUF_SOFFSET if m == 1 and lane >= 32 else 0)
    return (addr, 0, 0) if m == 0 else (addr - BUF_SOFFSET, BUF_SOFFSET, 0) if m == 1 else (addr - BUF_IMM, 0, BUF_IMM)


def lds_chunk(map_: int, lane: int) -> int:
    return (16 * lane, 16 * ((lane * 13 + 5) & 63), 128 * (lane & 31) + 16 * (lane >> 5))[map_]


LDS_READ_SUB = (lambda l: (l + 1) & 15, lambda l: (l * 3) & 15, lambda l: 2 * (l & 7), lambda l: 2 * ((l + 5) & 7), lambda l: 4 * (l & 3),
                lambda l: 8 * (l & 1), lambda l: 0, lambda l: 0)
LDS_WRITE_SUB = (lambda l: (l + 7) & 15, lambda l: 2 * ((l + 1) & 7), lambda l: 4 * ((l + 2) & 3), lambda l: 8 * ((l >> 1) & 1), lambda l: 0,
                 lambda l: 0)


def ldstr_addr(s: int, lane: int) -> int:
    return (4 * (lane >> 4) + ((lane >> 2) & 3)) * (32 + 16 * s) + 8 * (lane & 3)


def dma_src(wave: int, lane: int, f: int) -> int:
    return 16 * ((lane * 29 + wave * 512 + f * 64 + 3) & 2047)


DMA_BYTES = (4, 16, 4)            # global_load_lds_dword, _dwordx4, buffer_load_dword ... lds

T_GSTORE, T_GSTORE_BG, T_BUF, T_BUF_BG = 0x57012E00, 0x0B6B6000, 0x2BF00D00, 0x6A09E600
T_LDS, T_LDS_BG, T_LDSTR, T_ATOM = 0x1D5B6000, 0x4C1D5000, 0x7B160000, 0x00A70300

_TABLE: list = []


def table() -> Memory:
    if not _TABLE:
        _TABLE.append(Memory(4 * MEM_WORDS, [table_word(i) for i in range(MEM_WORDS)]))
    return _TABLE[0]


# ---- one wave of one group: {k: [64 lane words]} -----------------------------------------------
def wave_gload(wave: int) -> dict:
    t, out = table(), {}
    for map_ in range(2):
        k = 44 * map_
        for f, form in enumerate(GLOAD_FORMS):
            at = [gload_chunk(map_, wave, lane, f) for lane in range(LANES)]
            if form[0] in ("byte", "short"):
                n = 1 if form[0] == "byte" else 2
                out[k] = [load_ext(t, a + form[2], n, form[1]) for a in at]
                k += 1
            elif form[0] == "d16":
                out[k] = [load_d16(t, a + form[3], form[1], form[2]) for a in at]
                k += 1
            else:
                rows = [t.words(a, form[1]) for a in at]
                for j in range(form[1]):
                    out[k + j] = [r[j] for r in rows]
                k += form[1]
    return out


def wave_l1(wave: int) -> dict:
    t, out = table(), {}
    for p in range(2):
        for s in range(32):
            rows = [t.words(16 * l1_chunk(p, s, lane), 4) for lane in range(LANES)]
            for j in range(4):
                out[(p * 32 + s) * 4 + j] = [r[j] for r in rows]
    return out


def wave_gstore(wave: int) -> dict:
    out = {}
    for f, n in enumerate(GSTORE_BYTES):
        mem = Memory(WAVE_BYTES)
        for lane in range(LANES):                                    # the background: global_store_dwordx4
            mem.store(16 * lane, 16, pack(val(T_GSTORE_BG, wave, 0, f, 4 * lane + j) for j in range(4)))
        for lane in range(LANES):
            regs = [val(T_GSTORE, wave, lane, f, j) for j in range(4)]
            data = regs[0] >> 16 if f == 2 else pack(regs)           # short_d16_hi stores bits 31:16
            mem.store(gstore_chunk(wave, lane, f) + gstore_sub(lane, f), n, data)
        rows = [mem.words(gstore_chunk(wave, lane, f), 4) for lane in range(LANES)]
        for j in range(4):
            out[4 * f + j] = [r[j] for r in rows]
    return out


def _buf_background(wave: int, phase: int) -> Memory:
    return Memory(WAVE_BYTES, [val(T_BUF_BG, wave, 0, phase, i) for i in range(WAVE_BYTES // 4)])


def wave_buffer(wave: int) -> dict:
    out = {}
    first = (0, 1, 2, 3, 5, 8)
    mem = _buf_background(wave, 0)
    for w, n in enumerate(BUF_BYTES):
        for m in range(3):
            rows = []
            for lane in range(LANES):
                vo, so, imm = buf_operands(w, m, lane)
                inside = buffer_lane(vo, so, imm, n, BUF_RECORDS)
                rows.append([(mem.load(vo + so + imm, n) >> (32 * j)) & M32 if inside else 0 for j in range(max(1, n // 4))])
            for j in range(max(1, n // 4)):
                out[12 * m + first[w] + j] = [r[j] for r in rows]
    for w, n in enumerate(BUF_BYTES):
        for m in range(3):
            mem = _buf_background(wave, 1 + 3 * w + m)
            for lane in range(LANES):
                vo, so, imm = buf_operands(w, m, lane)
                if buffer_lane(vo, so, imm, n, BUF_RECORDS):          # an out-of-range store is dropped
                    mem.store(vo + so + imm, n, pack(val(T_BUF, wave, lane, 3 * w + m, j) for j in range(4)))
            rows = [mem.words(sum(buf_operands(w, m, lane)) & ~15, 4) for lane in range(LANES)]
            for j in range(4):
                out[36 + 4 * (3 * w + m) + j] = [r[j] for r in rows]
    return out


def wave_lds(wave: int) -> dict:
    out = {}

    def background(mem, map_, phase):
        for lane in range(LANES):
            for up in (0, LDS_UPPER):
                at = lds_chunk(map_, lane) + up
                mem.store(at, 16, pack(val(T_LDS_BG, wave, 0, phase, at // 4 + j) for j in range(4)))

    for map_ in range(3):
        mem = Memory(LDS_WAVE_BYTES)
        background(mem, map_, 0)
        k = 26 * map_
        at = [lds_chunk(map_, lane) for lane in range(LANES)]
        rows = {0: [[load_ext(mem, a + LDS_READ_SUB[0](l), 1, False)] for l, a in enumerate(at)],
                1: [[load_ext(mem, a + LDS_READ_SUB[1](l), 1, True)] for l, a in enumerate(at)],
                2: [[load_ext(mem, a + LDS_READ_SUB[2](l), 2, False)] for l, a in enumerate(at)],
                3: [[load_ext(mem, a + LDS_READ_SUB[3](l), 2, True)] for l, a in enumerate(at)],
                4: [mem.words(a + LDS_READ_SUB[4](l), 1) for l, a in enumerate(at)],
                5: [mem.words(a + LDS_READ_SUB[5](l), 2) for l, a in enumerate(at)],
                6: [mem.words(a, 3) for a in at],
                7: [mem.words(a, 4) for a in at],
                8: [mem.words(a, 1) + mem.words(a + 2 * 4, 1) for a in at],                      # read2_b32 offset0:0 offset1:2
                9: [mem.words(a, 2) + mem.words(a + 1 * 8, 2) for a in at],                      # read2_b64 offset0:0 offset1:1
                10: [mem.words(a, 1) + mem.words(a + 16 * 64 * 4, 1) for a in at],               # read2st64_b32 offset1:16
                11: [mem.words(a, 2) + mem.words(a + 8 * 64 * 8, 2) for a in at]}                # read2st64_b64 offset1:8
        for f in range(12):
            for j in range(len(rows[f][0])):
                out[k + j] = [r[j] for r in rows[f]]
            k += len(rows[f][0])
        k = 78 + 48 * map_
        for f in range(10):
            background(mem, map_, 1 + 10 * map_ + f)
            for lane, a in enumerate(at):
                v = [val(T_LDS, wave, lane, 16 * map_ + f, j) for j in range(4)]
                if f < 6:
                    n = (1, 2, 4, 8, 12, 16)[f]
                    mem.store(a + LDS_WRITE_SUB[f](lane), n, pack(v))
                elif f == 6:                                                                    # write2_b32 offset0:0 offset1:2
                    mem.store(a, 4, v[0]), mem.store(a + 2 * 4, 4, v[1])
                elif f == 7:                                                                    # write2_b64 offset0:0 offset1:1
                    mem.store(a, 8, pack(v[:2])), mem.store(a + 8, 8, pack(v[2:]))
                elif f == 8:                                                                    # write2st64_b32 offset1:16
                    mem.store(a, 4, v[0]), mem.store(a + 16 * 64 * 4, 4, v[1])
                else:                                                                           # write2st64_b64 offset1:8
                    mem.store(a, 8, pack(v[:2])), mem.store(a + 8 * 64 * 8, 8, pack(v[2:]))
            rows_w = [mem.words(a, 4) + (mem.words(a + LDS_UPPER, 4) if f >= 8 else []) for a in at]
            for j in range(len(rows_w[0])):
                out[k + j] = [r[j] for r in rows_w]
            k += len(rows_w[0])
    return out


def ldstr_elem(wave: int, s: int, row: int, col: int) -> int:
    return val(T_LDSTR, wave, 0, 16 * s + row, col) & 0xFFFF


def wave_ldstr(wave: int) -> dict:
    out = {}
    for s in range(2):
        mem = Memory(LDS_WAVE_BYTES)
        addrs = [ldstr_addr(s, lane) for lane in range(LANES)]
        for lane, a in enumerate(addrs):                             # ds_write_b64: the lane's 4 elements of its row
            row, col = 4 * (lane >> 4) + ((lane >> 2) & 3), 4 * (lane & 3)
            mem.store(a, 8, sum(ldstr_elem(wave, s, row, col + i) << (16 * i) for i in range(4)))
        got = tr_b16(mem, addrs)
        for j in range(2):
            out[2 * s + j] = [g[j] for g in got]
    return out


def wave_ldsdma(wave: int) -> dict:
    t, mem, out = table(), Memory(LDS_WAVE_BYTES, [DMA_BG] * (LDS_WAVE_BYTES // 4)), {}
    k = 0
    for f, n in enumerate(DMA_BYTES):
        for lane in range(LANES):
            mem.store(lds_dma_dest(1024 * f, lane, n), n, t.load(dma_src(wave, lane, f), n), align=4)
        for j in range(n // 4):
            out[k + j] = [mem.load(1024 * f + lane * n + 4 * j, 4) for lane in range(LANES)]
        k += n // 4
    return out


def atom_operands(m: int, wave: int, lane: int, i: int) -> tuple[int, int, int]:
    """(a, v, cmp) of operation i (its index in `ATOMICS`) on memory m: what the location holds, the operand, and
    cmpswap's compare value."""
    op, bits = ATOMICS[i]
    raw = [val(T_ATOM, wave, lane, 64 * m + i, 4 * which) | (val(T_ATOM, wave, lane, 64 * m + i, 4 * which + 1) << 32 if bits == 64 else 0)
           for which in range(2)]
    a, v = raw
    if op in ("inc", "dec"):
        v = (v & 0x7FFFFFFF) | 2
    if op == "inc":
        a = v >> 1 if lane & 1 else v
    if op == "dec":
        a = (0, v + 1, v >> 1, v >> 1)[lane & 3]
    return a, v, a ^ (0x10 if lane & 1 else 0)


def contended(m: int, wave: int) -> tuple[int, int]:
    return val(T_ATOM, wave, 0, 64 * m + 32, 0) & 0xFFFFFF, (val(T_ATOM, wave, 0, 64 * m + 32, 1) & 0xFFFFFF) | 1


def wave_atomic(wave: int) -> dict:
    out = {}
    for m in range(2):
        k = 46 * m
        for i, (op, bits) in enumerate(ATOMICS):
            n = bits // 32
            rows = []
            for lane in range(LANES):
                a, v, cmp = atom_operands(m, wave, lane, i)
                after = atomic(op, bits, a, v, cmp)
                rows.append([(a >> (32 * j)) & M32 for j in range(n)] + [(after >> (32 * j)) & M32 for j in range(n)])
            for j in range(2 * n):
                out[k + j] = [r[j] for r in rows]
            k += 2 * n
        b, c = contended(m, wave)
        word, returned = b, []
        for _lane in range(LANES):                                   # in some order: the set of returned values is the same
            returned.append(word)
            word = atomic("add", 32, word, c)
        qs = [(r - b) // c if r >= b and (r - b) % c == 0 and (r - b) // c < 64 else NO_Q for r in returned]
        flags = sum(1 << q for q in qs if q != NO_Q)
        out[k] = [int(q != NO_Q) for q in qs]
        out[k + 1], out[k + 2], out[k + 3] = [flags & M32] * LANES, [flags >> 32] * LANES, [word] * LANES
    return out


_WAVE = {"gload": wave_gload, "l1": wave_l1, "gstore": wave_gstore, "buffer": wave_buffer, "lds": wave_lds, "ldstr": wave_ldstr,
         "ldsdma": wave_ldsdma, "atomic": wave_atomic}
GROUP_WORDS = {"gload": 88, "l1": 256, "gstore": 28, "buffer": 108, "lds": 222, "ldstr": 4, "ldsdma": 6, "atomic": 92}
_CACHE: dict = {}


def group_indices(group: str) -> int:
    """The size of the space the record's index of `group` is in."""
    return MEM_WORDS if group == "l1" else GROUP_WORDS[group] * LANES


def group_lanes(group: str) -> list[int]:
    """What `mem_lanes(group)` returns on a sound device: every lane's result words, [wave][k][lane]."""
    if group not in _CACHE:
        out = []
        for wave in range(WAVES):
            words = _WAVE[group](wave)
            assert sorted(words) == list(range(GROUP_WORDS[group])), group
            for k in range(GROUP_WORDS[group]):
                out += words[k]
        _CACHE[group] = out
    return _CACHE[group]


def uncovered_bits(words) -> int:
    """Bits that are the same in every word."""
    ones = zeros = 0
    for w in words:
        ones |= w
        zeros |= ~w & M32
    return ~(ones & zeros) & M32


# ---- folding -----------------------------------------------------------------------------------
def fold_mem(records, groups, expected_cus) -> dict:
    """Folds `cu_sweep_mem` records `(xcc, hw_id, fail, simds, group_bits, bad_group, bad_index, bad_wave)` by CU;
    `groups` names the bits of `group_bits` in order. `failed` maps each failed group, or `record` (a garbled
    record), to its `[xcc, cu_key]` list; `cus` lists per failed CU its kinds, the waves (bit w: wave w) that saw any
    failure, and the first bad group with its lowest bad index and that index's wave. `uncovered` / `cus_uncovered`
    as in `fold_sweep`: not a failure."""
    groups = list(groups)
    cus = by_cu([tuple(r) for r in records])
    failures = []
    for k, visits in sorted(cus.items()):
        found, waves, first = set(), 0, None
        for fail, _simds, gbits, group, index, wave in visits:
            clean = fail == 0 and gbits == 0 and (group, index, wave) == (-1, -1, -1)
            located = (0 < fail < 1 << WAVES and 0 < gbits < 1 << len(groups) and 0 <= group < len(groups) and gbits >> group & 1
                       and not gbits & ((1 << group) - 1) and 0 <= wave < WAVES and fail >> wave & 1
                       and 0 <= index < group_indices(groups[group]))
            if not clean and not located:
                found.add("record")
                continue
            found.update(g for i, g in enumerate(groups) if gbits >> i & 1)
            waves |= fail
            if not clean and (first is None or (group, index, wave) < first):
                first = (group, index, wave)
        if found:
            kinds = [n for n in groups + ["record"] if n in found]
            failures.append((k, kinds, {"kinds": kinds, "waves": waves, "bad_group": groups[first[0]] if first else "",
                                        "bad_index": first[1] if first else -1, "bad_wave": first[2] if first else -1}))
    return dict(named_failures(cus, expected_cus, failures), simds_seen_min=simds_seen_min(cus, 1))


PART = Part(
    key="mem", names=GROUPS, noun="memory group", flag_noun="group", binding="cu_sweep_mem", names_key="groups",
    fold=fold_mem, kept=("cus", "table_words", "ms"), label="memory pipeline", detail=" ({table_words} table words, {ms:.3f} ms)",
    clauses=lambda d: [f"memory pipeline {'+'.join(c['kinds'])} on CU (xcc {c['xcc']}, key {c['cu_key']:#x})"
                       + (f", first in {c['bad_group']} at index {c['bad_index']}, wave {c['bad_wave']}" if c["bad_index"] >= 0 else "")
                       for c in d.get("cus", [])],
    note_missing="this probe has no cu_sweep_mem: no memory group was checked",
    note_unreached="{n} CUs not reached by the memory launches",
    help="memory-pipeline groups every CU also runs: 'all' or a comma-separated list",
    agent_help="the deep self-test also runs, on all four waves of every CU, global and buffer loads and stores of every "
               "width, the whole 32 KiB table through the CU's L1, the LDS instruction forms, the transposed LDS read, "
               "LDS-DMA and atomics with return: 'all' or a comma-separated list of gload, l1, gstore, buffer, lds, ldstr, "
               "ldsdma, atomic (implies --selftest-deep; start-up and periodic runs alike)",
    metric_help="memory-pipeline groups the last deep self-test ran on every CU",
    listed=False)


def twin_summary() -> dict:
    """What the stand-alone host program prints, from this module."""
    return {"groups": {g: [GROUP_WORDS[g], tile_checksum(group_lanes(g))] for g in GROUPS},
            "table_checksum": tile_checksum([table_word(i) for i in range(MEM_WORDS)]), "table_words": MEM_WORDS,
            "slice_bytes": SLICE_BYTES, "record_words": RECORD_WORDS}
