"""That the deep self-test can fail (`pytest -m gpu`): every word of every expected tile is
compared, by all four waves, on every CU. The kernels and what they compute stay as they are;
the host's expected data is corrupted in one word before the upload (the `corrupt_expected` hook,
and `sweep_sensitivity`, its loop over words on one set of buffers), so a clean chip must report
exactly that check failed, on every record. A compare loop that skipped a register, a lane, a
wave or a tile word would leave some word unnoticed. Nothing here makes the device fault."""
import time

import pytest

pytestmark = pytest.mark.gpu

SEED = 0x1234ABCD
TILES = ("bf16", "f16", "fp8", "bf8", "i8", "mxfp8", "mxfp6", "mxfp4", "f32", "f64")


def record(key: str, value) -> None:
    """Measured facts for profiles/gpu_calibration.md, into the same file as test_gpu.py's."""
    from test_gpu import record as record_fact   # tests/ is on sys.path (no package)

    record_fact(key, value)


@pytest.fixture(scope="module")
def P():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU visible")
    from nanogpu.native import probe

    return probe(required=True)


def tile_words(name: str) -> int:
    return 512 if name == "f64" else 1024


def flips_of(name: str) -> list[tuple[int, int]]:
    """Every word w of the tile with bit w % 32 flipped: all 32 bit positions occur in each tile,
    and both words of every f64 value."""
    return [(w, 1 << (w % 32)) for w in range(tile_words(name))]


def expected_fields(name: str) -> tuple[int, int, int, int]:
    """(fail bits, lds_bad, failed-path bits, path waves) of every record when `name`'s tile is wrong."""
    from nanogpu.probe.selftest_paths import PATHS

    if name == "bf16":
        return (0xF, -1, 0, 0)          # all four waves, no LDS bit, no path
    return (0, -1, 1 << PATHS.index(name), 0xF)


@pytest.mark.parametrize("name", TILES)
def test_every_word_of_the_expected_tile_is_compared_by_all_four_waves(P, name):
    """One unmasked sweep of 1 round, all paths selected, per word of `name`'s tile."""
    from nanogpu.probe.selftest_paths import PATHS

    flips = flips_of(name)
    t0 = time.perf_counter()
    r = P.sweep_sensitivity(0, name, flips, list(PATHS), [], 1, SEED)
    wall = time.perf_counter() - t0
    want = expected_fields(name)
    missed = [(w, f) for (w, _x), f in zip(flips, r["words"]) if tuple(f[0]) != want or tuple(f[1]) != want]
    print(name, "words", len(flips), "records per sweep", r["records"], "loop s", round(r["seconds"], 3), "wall s",
          round(wall, 3), "missed", len(missed), missed[:4])
    record(f"selftest_sensitivity_{name}", {"words": len(flips), "records_per_sweep": r["records"],
                                            "loop_seconds": round(r["seconds"], 3), "wall_seconds": round(wall, 3),
                                            "missed": len(missed)})
    assert r["records"] == 256 and len(r["words"]) == len(flips)
    assert {x.bit_length() - 1 for _w, x in flips} == set(range(32))
    assert missed == []


def test_every_word_of_the_bf16_tile_is_compared_by_the_plain_sweep(P):
    """cu_sweep's own kernels (no paths): the same loop over all 1,024 words."""
    flips = flips_of("bf16")
    r = P.sweep_sensitivity(0, "bf16", flips, [], [], 1, SEED)
    print("plain bf16 words", len(flips), "loop s", round(r["seconds"], 3))
    record("selftest_sensitivity_bf16_plain", {"words": len(flips), "loop_seconds": round(r["seconds"], 3)})
    want = (0xF, -1, 0, 0)
    assert r["records"] == 256
    assert [(w, f) for (w, _x), f in zip(flips, r["words"]) if tuple(f[0]) != want or tuple(f[1]) != want] == []


def test_plain_cu_sweep_binding_notices_a_word_of_every_register_half_and_parity(P):
    """`cu_sweep(corrupt_expected=...)`, one Python call per word, at 64 words: the row of every
    accumulator register (0..15) in both k halves h (C row = (reg & 3) + 8 (reg >> 2) + 4 h), at
    an even and at an odd column. Every record: all four waves fail the MFMA check, the LDS is clean."""
    words = [((reg & 3) + 8 * (reg >> 2) + 4 * h) * 32 + 2 * ((2 * reg + 7 * h) % 16) + parity
             for reg in range(16) for h in range(2) for parity in range(2)]
    assert len(set(words)) == 64 and len({w // 32 for w in words}) == 32
    t0 = time.perf_counter()
    for w in words:
        r = P.cu_sweep(0, [], 1, SEED, None, (w, 1 << (w % 32)))
        assert len(r["records"]) == 256
        bad = [rec for rec in r["records"] if rec[2] != 0xF or rec[4] != -1]
        assert bad == [], (w, bad[:4])
    per_call_ms = (time.perf_counter() - t0) / len(words) * 1e3
    print("cu_sweep with corrupt_expected: ms per Python call", round(per_call_ms, 3))
    record("selftest_sensitivity_python_call_ms", round(per_call_ms, 3))


@pytest.mark.parametrize("name", TILES)
def test_the_python_hook_agrees_with_the_loop_and_a_zero_xor_is_clean(P, name):
    """`cu_sweep_paths(corrupt_expected=...)` on the tile's last word, every record; and the hook
    with nothing to flip reports a clean chip, so it is the flipped bit that fails the check."""
    from nanogpu.probe.selftest_paths import PATHS

    last = tile_words(name) - 1
    want = expected_fields(name)
    r = P.cu_sweep_paths(0, [], 1, SEED, list(PATHS), None, (name, last, 0x80000000))
    assert len(r["records"]) == 256
    bad = [rec for rec in r["records"] if (rec[2], rec[4], rec[5], rec[6]) != want]
    assert bad == [], bad[:4]
    r0 = P.cu_sweep_paths(0, [], 1, SEED, list(PATHS), None, (name, last, 0))
    assert [rec for rec in r0["records"] if (rec[2], rec[4], rec[5], rec[6]) != (0, -1, 0, 0)] == []


@pytest.mark.parametrize("name", ["bf16", "f16"])
def test_a_flipped_word_is_restored_before_the_next_flip(P, name):
    """Both uploads of the sweep's session (the bf16 tile; the path tiles), all paths selected: after
    word 5 was flipped, a zero XOR of word 6 is clean on every record only if word 5 was put back."""
    from nanogpu.probe.selftest_paths import PATHS

    r = P.sweep_sensitivity(0, name, [(5, 1 << 5), (6, 0), (6, 1 << 6)], list(PATHS), [], 1, SEED)
    fails, clean = (expected_fields(name),) * 2, ((0, -1, 0, 0),) * 2
    assert [tuple(tuple(half) for half in w) for w in r["words"]] == [fails, clean, fails]


def test_the_hook_rejects_a_word_beyond_the_tile_and_a_path_not_selected(P):
    from nanogpu.probe.selftest_paths import PATHS

    for bad in (("bf16", 1024, 1), ("f16", 1024, 1), ("f64", 512, 1), ("bf17", 0, 1)):
        with pytest.raises(ValueError):
            P.cu_sweep_paths(0, [], 1, SEED, list(PATHS), None, bad)
    with pytest.raises(ValueError):
        P.cu_sweep_paths(0, [], 1, SEED, ["f16", "i8"], None, ("fp8", 0, 1))
    with pytest.raises(ValueError):
        P.cu_sweep(0, [], 1, SEED, None, (1024, 1))
    with pytest.raises(ValueError):
        P.sweep_sensitivity(0, "f32", [(0, 1)], [], [], 1, SEED)          # a path tile, but the plain sweep
    with pytest.raises(ValueError):
        P.sweep_sensitivity(0, "f64", [(511, 1), (512, 1)], list(PATHS), [], 1, SEED)
    # f64's word 511 is inside, and bf16 needs no path selected
    assert len(P.cu_sweep_paths(0, [], 1, SEED, ["f64"], None, ("f64", 511, 1))["records"]) == 256
    assert len(P.cu_sweep_paths(0, [], 1, SEED, ["i8"], None, ("bf16", 1023, 1))["records"]) == 256
