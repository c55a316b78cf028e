"""GPU parity of phase B of the dense image's build through the table of passes that backsolve_plan cuts for it
(spasm_amd/csrc/backsolve.hip): ring rows as pre-scaled 16-bit word offsets, both 16-bit coefficients in one word, rows with
more than two dependencies inside their chunk in passes of their own behind the ordinary passes of their level.
S = A_n - A_p R from spasm_hip_schur (the C ABI) is compared with spasm_schur's, entry for entry, for one modulus of each
arithmetic (signed 16-bit, unsigned 16-bit, 32-bit Montgomery) and every SPASM_HIP_BS_SHAPE.

The factors are LAYERED: the pivot rows come in layers, a row of layer l has one entry on a pivot of layer l + 1 and its others
on pivots of layers l + 1 .. l + 4, so that the elimination level of a row (longest path) is its layer and the plan meets
exactly the level widths and dependency counts written down here.  A few rows also reach a pivot some 1,400 rows further on:
outside any chunk (<= 1,260 rows), so that heads, chunk boundaries and dependencies across them are in every case.

No case hands a plan cut for one shape to the kernel of another: the plan and the launch both read the shape from the same
BsImage, the C ABI offers no way to make them disagree (the launcher's check dies on it, as on the other plan parameters)."""
import numpy as np
import pytest

import spasm_amd

pytestmark = pytest.mark.gpu

PRIMES = [42013, 65521, 4294967291]
SHAPES = ["0", "1", "2", "3", "4", "5"]
RINGS = {"0": 768, "1": 768, "2": 768, "3": 768, "4": 1260, "5": 1200}


def _as_product(A):
    return spasm_amd.Csr(A.n, A.m, A.p, A.j, A.x, A.prime)


def _layered(rng, p, widths, ndeps, nnon, nred, far_every=0):
    """pivot rows in layers of the given widths (first layer = first level); row j of a layer has ndeps(layer, j) entries on
    pivots of the next four layers (the first of them in the very next one: row j's is pivot j mod width there, so every
    pivot of a layer is somebody's dependency when the layer before is at least as wide), every far_every-th row one more
    on a pivot >= 1,400 rows further on, and two non-pivotal entries.  Returns the triplets and, per pivot row, its layer and
    its number of dependencies within the next four layers."""
    start = np.concatenate([[0], np.cumsum(widths)])
    npiv = int(start[-1])
    m = npiv + nnon
    ti, tj, tx = [], [], []
    layer_of, near_deps = [], []
    for l, w in enumerate(widths):
        for j in range(w):
            k = int(start[l]) + j
            cols = [k]
            nd = 0
            if l + 1 < len(widths):
                first = int(start[l + 1]) + j % widths[l + 1]
                pool_lo, pool_hi = int(start[l + 1]), int(start[min(l + 5, len(widths))])
                want = min(ndeps(l, j), pool_hi - pool_lo)
                others = [c for c in rng.permutation(np.arange(pool_lo, pool_hi))[:want + 1] if c != first][:want - 1]
                if want > 0:
                    cols += [first] + [int(c) for c in others]
                    nd = 1 + len(others)
            if far_every and k % far_every == 0 and k + 1400 < npiv:
                cols.append(int(rng.integers(k + 1400, npiv)))
            cols += [npiv + int(c) for c in rng.choice(nnon, size=2, replace=False)]
            layer_of.append(l)
            near_deps.append(nd)
            ti += [k] * len(cols)
            tj += cols
            tx += [1] + [int(v) for v in rng.integers(1, p, size=len(cols) - 1)]
    for k in range(nred):
        cols = rng.choice(m, size=6, replace=False)
        ti += [npiv + k] * 6
        tj += [int(c) for c in cols]
        tx += [int(v) for v in rng.integers(1, p, size=6)]
    sysm = (npiv + nred, m, np.array(ti, np.int32), np.array(tj, np.int32), np.array(tx, np.int64))
    return sysm, np.array(layer_of), np.array(near_deps)


_WANT = {}


def _check(oracle, monkeypatch, key, p, shape, sysm, env=()):
    monkeypatch.setenv("SPASM_HIP_BACKSOLVE", "1")
    monkeypatch.setenv("SPASM_HIP_BS_SHAPE", shape)
    for name, value in env:
        monkeypatch.setenv(name, value)
    spasm_amd.lib().spasm_hip_forget_cached_images()
    n, m, ti, tj, tx = sysm
    if (key, p) not in _WANT:          # the oracle's side does not depend on the shape: once per (case, modulus)
        A = oracle.compress(p, n, m, ti, tj, tx)
        npiv, perm, F = oracle.pivots_extract_structural(A, oracle.empty_fact(A.n, A.m, p))
        rows = perm[npiv:]
        want, p_out_want, _ = oracle.schur(A, rows, F)
        _WANT[(key, p)] = (A, npiv, F, rows, want, p_out_want)
    A, npiv, F, rows, want, p_out_want = _WANT[(key, p)]
    assert npiv == n - len(rows) and npiv >= (n * 4) // 5          # (the layered rows are pivots: the structure above is the factor's)
    S, p_out = spasm_amd.schur(_as_product(A), rows, spasm_amd.Fact(_as_product(F.U), F.qinv))
    assert np.array_equal(p_out, p_out_want)
    assert oracle.same_matrix(oracle.CSR(S.n, S.m, S.p, S.j, S.x, p), want)


def _mixed_case(p):
    """3,000 pivot rows in levels of 1 to 150 rows: 64 exactly, 65 and 150 (more than one pass of 64), 33 and 40 (more than one
    pass of 32), and narrow ones.  Row j of a level has (1, 2, 3, 1, 6, 2, 7, 9)[j mod 8] dependencies within the next four
    levels: ordinary and long rows side by side in every level wider than two, six and more (the list loop of four runs
    twice, nine: three times), and the next level draws its dependencies among both kinds.  Rows without a dependency inside
    their chunk are the ones at the top of every chunk.  More than 2 x 1,260 rows: at least two chunk boundaries for every
    shape, crossed by the rows next to them and by every 5th row's far entry."""
    rng = np.random.default_rng(4242)
    pattern = (1, 2, 3, 1, 6, 2, 7, 9)
    cycle = [1, 3, 64, 65, 150, 33, 32, 7, 40, 2, 64, 100]
    widths = []
    while sum(widths) < 3000:
        widths.append(cycle[len(widths) % len(cycle)])
    sysm, layer_of, near_deps = _layered(rng, p, widths, lambda l, j: pattern[j % 8], nnon=77, nred=200, far_every=5)
    # what the case is for, checked on the structure itself
    assert sysm[0] - 200 > 2 * max(RINGS.values())
    for count in (1, 2, 3, 6, 7, 9):
        assert np.any(near_deps == count)
    mixed = [l for l in range(len(widths)) if np.any(near_deps[layer_of == l] > 2) and np.any((near_deps[layer_of == l] > 0) & (near_deps[layer_of == l] <= 2))]
    assert len(mixed) > len(widths) // 2
    assert 64 in widths and max(widths) > 64 and any(32 < w < 64 for w in widths)
    return sysm


def _full_chunk_case(p):
    """2,700 pivot rows in nine levels of 300: few passes and few list entries per chunk, so nothing but the ring cuts the
    chunks and every chunk but the first one cut holds RING rows -- its last row sits in slot RING - 1, the largest
    pre-scaled offset, and (300 rows a level, row j of a level on pivot j of the next) is a dependency of a row of the level
    before.  Every 16th row is a long one (3 or 6 dependencies), the others have one or two."""
    rng = np.random.default_rng(777)
    sysm, _, near_deps = _layered(rng, p, [300] * 9, lambda l, j: (3 if j % 32 == 0 else 6) if j % 16 == 0 else 1 + j % 2, nnon=40, nred=150, far_every=7)
    assert np.count_nonzero(near_deps > 2) * 5 < 1024          # (list entries: well under the capacity of one chunk)
    return sysm


_CASES = {}


def _case(name, p):
    if (name, p) not in _CASES:
        _CASES[(name, p)] = {"mixed": _mixed_case, "full": _full_chunk_case}[name](p)
    return _CASES[(name, p)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("p", PRIMES)
def test_passes_mixed_levels_and_dependency_counts(oracle, monkeypatch, p, shape):
    _check(oracle, monkeypatch, "mixed", p, shape, _case("mixed", p))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("p", PRIMES)
def test_passes_full_chunks_last_slot(oracle, monkeypatch, p, shape):
    _check(oracle, monkeypatch, "full", p, shape, _case("full", p))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("p", PRIMES)
def test_passes_prefilled_rows(oracle, monkeypatch, p, shape):
    """the same mixed levels with R pre-filled by bs_init_kernel (SPASM_HIP_BS_SPARSE_INIT=0: the other start of the rows)."""
    _check(oracle, monkeypatch, "mixed", p, shape, _case("mixed", p), env=(("SPASM_HIP_BS_SPARSE_INIT", "0"),))
