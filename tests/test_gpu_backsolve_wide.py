"""The dense image's build with FOUR words of a row per lane in phases A and C (backsolve_kernel, spasm_amd/csrc/backsolve.hip:
BsGeom::WPL = 4 for the slabs of 12 and of 8 words, SPASM_HIP_BS_SHAPE=5 and =3).  The Schur complement must be the oracle's,
and it must be -- Sp, Sj and Sx, bit for bit -- what the same problem gives under a shape that keeps one word per lane
(SPASM_HIP_BS_SHAPE=0).

With four words per lane a row of a slab is 3 (2) lanes, a wave instruction covers 20 (32) rows, an iteration of the workgroup
240 (256) rows and a chunk 1,200 (768) rows in 5 (3) iterations.  The shapes sit on both sides of each of those counts, on
column counts around one slab (24 columns), on a last slab that is whole but padded (500), on a last slab of 12 words whose
second and third quads lie beyond the padded row (512: 256 words, the 22nd slab holds words 252..255 only) and on the
first width with a second 256-word block (513).  Pivot rows carry 0, 1, 2 or 5 entries at least 1,500 rows away (the two
slots of the head, an absent slot, the long list on top of the wide phase A) beside their two entries nearby.

Moduli without signed 16-bit entries (65521, 4294967291) have no kernel with four words per lane: asked for shape 5 they
take the slabs of 16 words, one word per lane, and are here for the code that kernel shares with the wide ones."""
import numpy as np
import pytest

import spasm_amd

pytestmark = pytest.mark.gpu

# (tests/conftest.py sets SPASM_HIP_EXPERIMENT=1: the switches are honoured)
P = 42013
NAMES = {"5": "backsolve_kernel<true,true,12,12,true,1200,64,44,1>", "3": "backsolve_kernel<true,true,8,8,true,768,64,31,2>",
         "0": "backsolve_kernel<true,true,32,16,true,768,32,80,1>"}
FAR = (0, 1, 2, 5)          # entries of a pivot row at least FAR_AWAY rows away, by row number mod 4
FAR_AWAY = 1500             # (beyond any chunk: 1,200 rows at the most)


def _product(C):
    return spasm_amd.Csr(C.n, C.m, C.p, C.j, C.x, C.prime)


def _system(rng, p, npiv, nnon, nred=150, reach=40, dep_every=1, np_per_row=3, red_np=2, extreme=False):
    """npiv pivot rows, then nred rows to reduce: row i of those has an entry on the pivotal columns i, i + nred, i + 2 nred,
    ... and on red_np trailing ones, so that every row of R goes into S.  Pivot row k: 1 on column k; when dep_every divides
    k, two entries within `reach` columns to the right; FAR[k % 4] entries at least FAR_AWAY columns to the right; np_per_row
    entries on the nnon trailing columns.  dep_every = 1 gives long chains of levels (chunks end where the pass table is
    full), dep_every = 7 a few wide levels (chunks end where the ring is full).  extreme: every entry but the pivots is (p - 1) / 2 or (p + 1) / 2."""
    m = npiv + nnon
    ti, tj, tx = [], [], []
    for k in range(npiv):
        cols = [k]
        room = min(reach, npiv - k - 1)
        if k % dep_every == 0 and room > 0:
            cols += [int(c) for c in k + 1 + rng.choice(room, size=min(2, room), replace=False)]
        room = npiv - (k + FAR_AWAY)
        if room > 0:
            far = [int(c) for c in k + FAR_AWAY + rng.choice(room, size=min(FAR[k % 4], room), replace=False)]
            cols += [c for c in far if c not in cols]
        cols += [int(c) for c in npiv + rng.choice(nnon, size=min(np_per_row, nnon), replace=False)]
        ti += [k] * len(cols)
        tj += cols
        tx += [1] + [int(v) for v in rng.integers(1, p, size=len(cols) - 1)]
    for k in range(nred):
        cols = list(range(k, npiv, nred)) + [int(c) for c in npiv + rng.choice(nnon, size=min(red_np, nnon), replace=False)]
        ti += [npiv + k] * len(cols)
        tj += cols
        tx += [int(v) for v in rng.integers(1, p, size=len(cols))]
    tx = np.array(tx, np.int64)
    if extreme:
        tx = np.where(tx == 1, 1, np.where(rng.integers(0, 2, size=len(tx)) == 0, (p - 1) // 2, (p + 1) // 2)).astype(np.int64)
    return npiv + nred, m, np.array(ti, np.int32), np.array(tj, np.int32), tx


def _problem(oracle, p, sysm, npiv):
    """(A, factor, rows to reduce, the oracle's S): the factor comes from the pivot rows alone, so that the non-pivotal
    columns are exactly the trailing ones"""
    n, m, ti, tj, tx = sysm
    A = oracle.compress(p, n, m, ti, tj, tx)
    top = ti < npiv
    Pm = oracle.compress(p, npiv, m, ti[top], tj[top], tx[top])
    found, _, F = oracle.pivots_extract_structural(Pm, oracle.empty_fact(Pm.n, Pm.m, p))
    assert found == npiv and F.U.n == npiv
    rows = np.arange(npiv, n, dtype=np.int32)
    want, _, _ = oracle.schur(A, rows, F)
    return A, F, rows, want


def _build_and_apply(monkeypatch, A, F, rows, shape, env):
    """S on the host from a fresh factor whose image is planned and built under SPASM_HIP_BS_SHAPE=shape, and the names of the
    two kernels of the dense image"""
    import torch
    monkeypatch.setenv("SPASM_HIP_BACKSOLVE", "1")
    monkeypatch.setenv("SPASM_HIP_BS_SIGNED", "1")
    monkeypatch.setenv("SPASM_HIP_BS_SHAPE", shape)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    dA = spasm_amd.DeviceCsr.from_host(_product(A))
    dF = spasm_amd.DeviceFact(spasm_amd.Fact(_product(F.U), F.qinv))
    W = spasm_amd.SchurWorkspace(len(rows), A.m, 1 << 22)
    S, st = spasm_amd.dschur(dA, torch.from_numpy(rows).cuda(), dF, W)
    assert st.status == 0 and st.used_backsolve == 1
    H = S.to_host()
    W.close()
    dF.close()
    return H, {st.kernel.decode(), st.kernel_other.decode()}


def _check(oracle, monkeypatch, p, sysm, npiv, shapes=("5", "3"), env=None, signed=True):
    env = env or {}
    A, F, rows, want = _problem(oracle, p, sysm, npiv)
    ref, names = _build_and_apply(monkeypatch, A, F, rows, "0", env)
    if signed:
        assert NAMES["0"] in names
    assert oracle.same_matrix(oracle.CSR(ref.n, ref.m, ref.p, ref.j, ref.x, p), want)
    for shape in shapes:
        H, names = _build_and_apply(monkeypatch, A, F, rows, shape, env)
        if signed:
            assert NAMES[shape] in names
        else:          # (no signed entries: the slabs of 16 words, one word per lane)
            assert any(n.startswith("backsolve_kernel<") and ",16,8," in n for n in names)
        assert oracle.same_matrix(oracle.CSR(H.n, H.m, H.p, H.j, H.x, p), want), "shape %s differs from the oracle" % shape
        assert np.array_equal(H.p, ref.p) and np.array_equal(H.j, ref.j) and np.array_equal(H.x, ref.x), \
            "shape %s differs from the one-word-per-lane build" % shape


@pytest.mark.parametrize("nnon", [1, 24, 25, 500, 512, 513])
def test_wide_column_counts(oracle, monkeypatch, nnon):
    """one slab, one slab and a column, a padded last slab, a last slab with two quads beyond the row, two 256-word blocks:
    2,500 pivot rows in long chains, with 0, 1, 2 and 5 entries beyond the chunk"""
    rng = np.random.default_rng(7000 + nnon)
    _check(oracle, monkeypatch, P, _system(rng, P, npiv=2500, nnon=nnon), 2500)


@pytest.mark.parametrize("npiv", [1, 19, 20, 21, 239, 240, 241, 767, 768, 769, 1199, 1200, 1201, 2500])
def test_wide_pivot_rows(oracle, monkeypatch, npiv):
    """both sides of a wave instruction (20 rows), of an iteration of the workgroup (240) and of a chunk (768 rows for the
    slabs of 8 words, 1,200 for those of 12), and three chunks; few levels, so that a chunk ends where the ring is full"""
    rng = np.random.default_rng(8000 + npiv)
    _check(oracle, monkeypatch, P, _system(rng, P, npiv=npiv, nnon=100, dep_every=7), npiv)


@pytest.mark.parametrize("dep_every", [1, 7])
def test_wide_reach_into_earlier_chunks(oracle, monkeypatch, dep_every):
    """the two nearby entries anywhere within 2,000 rows: inside the chunk, in the one before it and in the one before that"""
    rng = np.random.default_rng(9000 + dep_every)
    _check(oracle, monkeypatch, P, _system(rng, P, npiv=3600, nnon=100, reach=2000, dep_every=dep_every), 3600)


@pytest.mark.parametrize("p", [65521, 4294967291])
def test_wide_other_arithmetics(oracle, monkeypatch, p):
    """an unsigned 16-bit and a 32-bit modulus under the same requests"""
    rng = np.random.default_rng(p % 1000)
    _check(oracle, monkeypatch, p, _system(rng, p, npiv=2500, nnon=512), 2500, signed=False)


def test_wide_prefilled_rows(oracle, monkeypatch):
    """SPASM_HIP_BS_SPARSE_INIT=0: R is pre-filled and a lane loads its own four words with those of the dependencies"""
    rng = np.random.default_rng(31)
    _check(oracle, monkeypatch, P, _system(rng, P, npiv=2500, nnon=512), 2500, env={"SPASM_HIP_BS_SPARSE_INIT": "0"})


def test_wide_extreme_values(oracle, monkeypatch):
    """every entry of the pivot rows is (p - 1) / 2 or (p + 1) / 2, the balanced representatives of largest magnitude (the
    bound of test_backsolve_extreme_values), through the wide phase A of the slabs of 12 words"""
    rng = np.random.default_rng(77)
    _check(oracle, monkeypatch, P, _system(rng, P, npiv=2500, nnon=70, extreme=True), 2500, shapes=("5",))
