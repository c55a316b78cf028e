"""The dense image's CSR output (bs_apply_s16_csr_kernel, spasm_amd/csrc/backsolve.hip) against its staged output
(bs_apply_s16_kernel + bs_scan_lengths_kernel + bs_expand_kernel<0>): the same Sp, Sj and Sx, bit for bit.

The CSR output writes every row of S at its final place from the LDS buffer it was computed in; a row's offset comes from a
look-back over the lengths the rows before it published.  The cases aim at that: rows that reduce to nothing, input rows
without entries, fewer rows than a workgroup has waves, a single row, a pool that runs out in the middle of the batch, and a
batch large enough that every workgroup publishes many rows."""
import numpy as np
import pytest

import spasm_amd

pytestmark = pytest.mark.gpu

STAGED = {"SPASM_HIP_BS_CSR": "0"}          # (tests/conftest.py sets SPASM_HIP_EXPERIMENT=1: the switch is honoured)


def _product(C):
    return spasm_amd.Csr(C.n, C.m, C.p, C.j, C.x, C.prime)


def _system(rng, p, npiv, nnon, nred, deps=2, reach=40, np_per_row=3, red_entries=6, zero_rows=0, empty_rows=0):
    """npiv pivot rows (row k: pivot on column k, `deps` pivotal entries within `reach` columns to the right, np_per_row
    entries on the nnon trailing columns), then nred rows to reduce: the first zero_rows are copies of pivot rows (their rows
    of S are all zero), the next empty_rows have no entries at all."""
    m = npiv + nnon
    ti, tj, tx = [], [], []
    pivot_rows = []
    for k in range(npiv):
        cols = [k]
        room = min(reach, npiv - k - 1)
        d = min(deps, room)
        if d > 0:
            cols += [int(c) for c in k + 1 + rng.choice(room, size=d, replace=False)]
        cols += [int(c) for c in npiv + rng.choice(nnon, size=min(np_per_row, nnon), replace=False)]
        vals = [1] + [int(v) for v in rng.integers(1, p, size=len(cols) - 1)]
        pivot_rows.append((cols, vals))
        ti += [k] * len(cols)
        tj += cols
        tx += vals
    for k in range(nred):
        if k < zero_rows:
            cols, vals = pivot_rows[int(rng.integers(0, npiv))]
        elif k < zero_rows + empty_rows:
            continue
        else:
            cols = [int(c) for c in rng.choice(m, size=min(red_entries, m), replace=False)]
            vals = [int(v) for v in rng.integers(1, p, size=len(cols))]
        ti += [npiv + k] * len(cols)
        tj += cols
        tx += vals
    return npiv + nred, m, np.array(ti, np.int32), np.array(tj, np.int32), np.array(tx, np.int64)


def _problem(oracle, p, sysm, nrows=None):
    n, m, ti, tj, tx = sysm
    A = oracle.compress(p, n, m, ti, tj, tx)
    npiv, perm, F = oracle.pivots_extract_structural(A, oracle.empty_fact(A.n, A.m, p))
    rows = perm[npiv:] if nrows is None else perm[npiv:npiv + nrows]
    return A, F, np.ascontiguousarray(rows, np.int32)


def _run(monkeypatch, A, F, rows, pool, env):
    """the batch through the dense image under `env` on a fresh factor and workspace of `pool` entries: (S on the host or
    None, stats, device A, device factor, workspace)"""
    import torch
    monkeypatch.setenv("SPASM_HIP_BACKSOLVE", "1")
    monkeypatch.setenv("SPASM_HIP_BS_SIGNED", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        dA = spasm_amd.DeviceCsr.from_host(_product(A))
        dF = spasm_amd.DeviceFact(spasm_amd.Fact(_product(F.U), F.qinv))
        W = spasm_amd.SchurWorkspace(len(rows), A.m, pool)
        S, st = spasm_amd.dschur(dA, torch.from_numpy(rows).cuda(), dF, W)
    finally:
        for k in env:
            monkeypatch.delenv(k)
    assert st.used_backsolve == 1
    # which output ran: the staged one names its expansion kernel
    assert st.kernel_expand.decode() == ("bs_expand_kernel<0>" if env else "")
    return (S.to_host() if S is not None else None), st, dA, dF, W


def _both_identical(monkeypatch, A, F, rows, pool=1 << 22):
    H1, st1, _, _, _ = _run(monkeypatch, A, F, rows, pool, {})
    H2, st2, _, _, _ = _run(monkeypatch, A, F, rows, pool, STAGED)
    assert st1.status == st2.status == 0
    assert st1.nnz == st2.nnz
    assert np.array_equal(H1.p, H2.p)
    assert np.array_equal(H1.j, H2.j)
    assert np.array_equal(H1.x, H2.x)
    return H1, st1


@pytest.mark.parametrize("p", [3, 257, 42013, 44927])
def test_csr_output_matches_staged_at_the_signed_moduli(oracle, monkeypatch, p):
    """primes of the signed 16-bit path up to its largest, 44,927; the result is the oracle's as well"""
    rng = np.random.default_rng(p)
    A, F, rows = _problem(oracle, p, _system(rng, p, npiv=1500, nnon=300, nred=700))
    H, _ = _both_identical(monkeypatch, A, F, rows)
    want, _, _ = oracle.schur(A, rows, F)
    assert oracle.same_matrix(oracle.CSR(H.n, H.m, H.p, H.j, H.x, p), want)


def test_csr_output_zero_and_empty_rows(oracle, monkeypatch):
    """rows of S that are all zero (copies of pivot rows) and input rows without entries, among ordinary ones"""
    p = 42013
    rng = np.random.default_rng(3)
    A, F, rows = _problem(oracle, p, _system(rng, p, npiv=1200, nnon=200, nred=600, zero_rows=150, empty_rows=100))
    rng.shuffle(rows)
    H, _ = _both_identical(monkeypatch, A, F, rows)
    assert np.count_nonzero(np.diff(H.p) == 0) >= 250


@pytest.mark.parametrize("nrows", [1, 2, 5, 63])
def test_csr_output_fewer_rows_than_waves(oracle, monkeypatch, nrows):
    """one row, and fewer rows than the waves of a single workgroup"""
    p = 42013
    rng = np.random.default_rng(nrows)
    A, F, rows = _problem(oracle, p, _system(rng, p, npiv=800, nnon=500, nred=100), nrows=nrows)
    assert len(rows) == nrows
    _both_identical(monkeypatch, A, F, rows)


def test_csr_output_many_rows_per_workgroup(oracle, monkeypatch):
    """20,000 rows: every workgroup of the grid publishes and writes many rows"""
    p = 42013
    rng = np.random.default_rng(11)
    A, F, rows = _problem(oracle, p, _system(rng, p, npiv=2000, nnon=700, nred=20000, np_per_row=2, red_entries=4))
    _, st = _both_identical(monkeypatch, A, F, rows, pool=1 << 26)
    assert st.nnz > 20000


@pytest.mark.parametrize("where", [0.0, 0.5, 0.999])
def test_csr_output_pool_runs_out_mid_batch(oracle, monkeypatch, where):
    """a pool smaller than S: both outputs raise the overflow status and report the same total, and the workspace is intact
    afterwards (a row that fits the pool comes out as the oracle has it)"""
    import torch
    p = 42013
    rng = np.random.default_rng(23)
    A, F, rows = _problem(oracle, p, _system(rng, p, npiv=1500, nnon=400, nred=2000))
    want, _, _ = oracle.schur(A, rows, F)
    cap = max(1, int(want.nnz * where))
    one = rows[:1]
    want_one, _, _ = oracle.schur(A, one, F)
    for env in ({}, STAGED):
        S, st, dA, dF, W = _run(monkeypatch, A, F, rows, cap, env)
        assert S is None and st.status == 1 and st.nnz == want.nnz
        if want_one.nnz <= cap:
            S1, st1 = spasm_amd.dschur(dA, torch.from_numpy(one).cuda(), dF, W)
            assert st1.status == 0
            H = S1.to_host()
            assert oracle.same_matrix(oracle.CSR(H.n, H.m, H.p, H.j, H.x, p), want_one)
