"""What is the same for every part of the deep self-test with a launch of its own, on a real MI355X, written
once over `PARTS` (the GPU sibling of tests/test_selftest_parts.py): the masked run, the flip that must not
outlive its sweep, and what the launch costs. What is specific to a part is in test_gpu_selftest_<part>.py.
Nothing here corrupts anything but the host's own upload."""
import statistics

import pytest

from gpu_harness import SEED, P, census_keys, record, sweep_all, unit_mask   # tests/ is on sys.path (no package)
from nanogpu.probe.selftest import PARTS
from nanogpu.probe.selftest_common import cu_key

pytestmark = pytest.mark.gpu

OWN_LAUNCH = [p for p in PARTS if not p.in_sweep]
each_part = pytest.mark.parametrize("part", OWN_LAUNCH, ids=[p.key for p in OWN_LAUNCH])

# part key -> (fact, the fields of the launch's result it holds)
REGS = {"scalar": ("selftest_scalar_regs", ("sreg_slots", "num_regs", "scratch_bytes")),
        "mem": ("selftest_mem_regs", ("num_regs", "scratch_bytes", "slice_bytes"))}

# (part key, group, what a flipped word 5 reports (AND and OR alike), a clean sweep, a flipped word 6)
FLIPS = [("valu", "fma32", (0xF, 1), (0, 0), (0xF, 1)),
         ("scalar", "add", (1, 1, -1), (0, 0, -1), (1, 1, -1)),
         ("scalar", "smem", (0x10, 0, 5), (0, 0, -1), (0x10, 0, 6)),
         ("mem", "l1", (0xF, 2, 1, 5), (0, 0, -1, -1), (0xF, 2, 1, 6))]


@each_part
def test_masked_to_one_unit(P, part):
    mask = unit_mask(5)
    r, f = sweep_all(P, part, part.names, mask=mask, cus=8)
    assert f["cus_seen"] == 8 and f["cus_uncovered"] == 0 and f["failed"] == {} and len(r["records"]) % 8 == 0
    assert sorted({rec[0] for rec in r["records"]}) == list(range(8))     # one CU per XCD
    ours = {(rec[0], cu_key(rec[1])) for rec in r["records"]}
    unit = census_keys(P, mask)
    assert len(unit) == 8 and ours == unit


@pytest.mark.parametrize("key,group,bad5,clean,bad6", FLIPS, ids=[f"{k}-{g}" for k, g, *_ in FLIPS])
def test_a_flipped_word_is_restored_before_the_next_flip(P, key, group, bad5, clean, bad6):
    """A word left corrupted would hide behind the next one's failure. A zero XOR of the word flipped before is
    clean on every record: the XOR starts from the host's word each time, and the host's table was not written. A
    zero XOR of another word is clean only if the word flipped before was put back; the words around both must
    still fail."""
    def words(flips):
        return [tuple(tuple(half) for half in w) for w in getattr(P, f"{key}_sensitivity")(0, group, flips)["words"]]

    want = [(bad5, bad5), (clean, clean), (bad6, bad6)]
    assert words([(5, 1 << 3), (5, 0), (6, 1 << 9)]) == want
    assert words([(5, 1 << 3), (6, 0), (6, 1 << 9)]) == want   # word 5 restored


@each_part
def test_cost_of_the_launch(P, part):
    """No threshold: the window in which a new grant could share CUs with the test is reported."""
    key = part.key
    plain, own, last = [], [], {}
    for _ in range(11):                                   # interleaved pairs in one process
        plain.append(P.cu_sweep(0, [], 4, SEED)["ms"])
        last = getattr(P, part.binding)(0, [], 4, SEED, list(part.names))
        own.append(last["ms"])
    facts = {"sweep_ms": statistics.median(plain), f"{key}_ms": statistics.median(own),
             f"sweep_plus_{key}_ms": statistics.median(a + b for a, b in zip(plain, own)), "pairs": len(plain)}
    print(key, "cost", facts)
    record(f"selftest_{key}_cost", facts)
    if key in REGS:
        fact, fields = REGS[key]
        record(fact, {k: last[k] for k in fields})
