"""Every operand code and every E8M0 scale, once, on a real MI355X (`pytest -m gpu`):
`matrix_tile` on the edge tiles of nanogpu.probe.selftest_paths.edge_tiles, bit-equal with the twin's
exact product. Every accumulator of such a tile has one term at most, so the result is exact in
any order and the tiles may hold what the sweep's generators exclude: zero, subnormals, the
largest normals, every code of the narrow formats, and scales 0..254 in every byte of the scale
register. tests/test_selftest_edge_tiles.py checks the tiles' own conditions on the host."""
import collections
import time

import pytest

pytestmark = pytest.mark.gpu


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


def code_class(path, code):
    from nanogpu.probe import selftest_paths as SP

    ebits, mbits, _bias = SP.PATH_FORMAT[path]
    if not ebits:
        return "int"
    mag = code & ((1 << (ebits + mbits)) - 1)
    return "zero" if mag == 0 else "subnormal" if mag >> mbits == 0 else "normal"


def describe(path, a, b, sa, sb, at):
    """(class of A's code, class of B's code) and the operands of accumulator `at`'s one term."""
    from nanogpu.probe import selftest_paths as SP

    dim = SP.path_dim(path)
    r, c = divmod(at, dim)
    ks = [k for k in range(SP.PATH_K[path]) if a[r][k] and b[k][c]]
    if not ks:
        return ("no term", "no term"), None
    k = ks[0]
    what = {"row": r, "col": c, "k": k, "a": hex(a[r][k]), "b": hex(b[k][c])}
    if sa is not None:
        what.update(sa=sa[r][k // 32], sb=sb[k // 32][c])
    return (code_class(path, a[r][k]), code_class(path, b[k][c])), what


@pytest.mark.parametrize("path", ["f16", "fp8", "bf8", "i8", "mxfp8", "mxfp6", "mxfp4", "f32", "f64"])
def test_matrix_tile_is_exact_on_every_code_and_every_scale(P, path):
    """The expected value is the OCP value of the one term; an accumulator without a term, or
    whose term is +-0, holds +0."""
    from nanogpu.probe import selftest_paths as SP

    per = 2 if path == "f64" else 1
    t0 = time.perf_counter()
    tiles = wrong_words = accumulators = 0
    by_class = collections.Counter()
    examples = []
    codes = [set(), set()]
    scales = [set(), set()]
    for a, b, sa, sb, opsel in SP.edge_tiles(path):
        want = SP.product_words(path, a, b, sa, sb)
        args = [] if sa is None else [[v for row in sa for v in row], [v for row in sb for v in row], opsel]
        got = SP.tile_words(path, P.matrix_tile(path, [c for row in a for c in row], [c for row in b for c in row], *args))
        assert len(got) == len(want)
        tiles += 1
        accumulators += len(want) // per
        codes[0].update(c for row in a for c in row)
        codes[1].update(c for row in b for c in row)
        if sa is not None:
            scales[0].update((v, opsel[0]) for row in sa for v in row)
            scales[1].update((v, opsel[1]) for row in sb for v in row)
        for i in sorted({i // per for i in range(len(want)) if want[i] != got[i]}):
            wrong_words += sum(want[per * i + j] != got[per * i + j] for j in range(per))
            cls, what = describe(path, a, b, sa, sb, i)
            by_class[cls] += 1
            if len(examples) < 12:
                examples.append((what, [hex(w) for w in want[per * i:per * i + per]], [hex(w) for w in got[per * i:per * i + per]]))
    wall = time.perf_counter() - t0
    facts = {"tiles": tiles, "accumulators": accumulators, "codes_in_a": len(codes[0]), "codes_in_b": len(codes[1]),
             "scale_bytes_a": len(scales[0]), "scale_bytes_b": len(scales[1]), "wrong_words": wrong_words,
             "wall_seconds": round(wall, 3)}
    print(path, facts, "wrong by (class of a, class of b):", dict(by_class))
    for e in examples:
        print("   ", e)
    record(f"selftest_edge_tiles_{path}", facts)
    assert wrong_words == 0, (path, dict(by_class), examples[:4])
