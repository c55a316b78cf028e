"""The dense image's CSR output with the older pending row of a wave in registers (bs_apply_s16_csr_rowreg_kernel,
spasm_amd/csrc/backsolve.hip) against the same output with two LDS row buffers (bs_apply_s16_csr_kernel,
SPASM_HIP_BS_CSR_ROWREG=0) and against the staged output (SPASM_HIP_BS_CSR=0): the same Sp, Sj and Sx, bit for bit.

The register kernel is instantiated per number of 64-word tiles of a row, in steps of four tiles (512 columns), up to 40
tiles (5,120 columns); wider rows keep the two-buffer kernel.  The widths below sit on both sides of an instantiation
(511, 512, 513 non-pivotal columns), at the smallest row (1), on middle instantiations whose three and four tile groups take
every turn of the emit loop's rotation of column buffers (1,536 and 2,048), at the benchmark's width (4,952), at the last instantiation
with no padding and an entry in its last column (5,120) and one past it (5,121).  The batches aim at the hand-over of a
row from LDS to the registers: fewer rows than waves, rows that reduce to nothing, input rows without entries, 20,000
short rows (every wave hands over many rows and meets both places taken), a pool that runs out in mid-batch."""
import numpy as np
import pytest

import spasm_amd

pytestmark = pytest.mark.gpu

# (tests/conftest.py sets SPASM_HIP_EXPERIMENT=1: the switches are honoured)
ROWREG, TWO_BUFFERS, STAGED = {}, {"SPASM_HIP_BS_CSR_ROWREG": "0"}, {"SPASM_HIP_BS_CSR": "0"}
WIDEST = 5120          # non-pivotal columns of the widest instantiation of the register kernel


def _product(C):
    return spasm_amd.Csr(C.n, C.m, C.p, C.j, C.x, C.prime)


def _system(rng, p, npiv, nnon, nred, deps=2, reach=40, np_per_row=3, red_entries=6, zero_rows=0, empty_rows=0, last_col=False):
    """npiv pivot rows (row k: pivot on column k, `deps` pivotal entries within `reach` columns to the right, np_per_row
    entries on the nnon trailing columns), then nred rows to reduce: the first zero_rows are copies of pivot rows (their rows
    of S are all zero), the next empty_rows have no entries at all.  last_col: every other ordinary row to reduce has an
    entry in the last column."""
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
            if last_col and k % 2 == 0 and m - 1 not in cols:
                cols[-1] = m - 1
            vals = [int(v) for v in rng.integers(1, p, size=len(cols))]
        ti += [npiv + k] * len(cols)
        tj += cols
        tx += vals
    return npiv + nred, m, np.array(ti, np.int32), np.array(tj, np.int32), np.array(tx, np.int64)


def _problem(oracle, p, sysm, npiv, nrows=None):
    """The factor comes from the npiv pivot rows alone, so that the number of non-pivotal columns is exactly nnon (a search
    over the whole matrix would also take rows to reduce as pivots on the trailing columns and narrow S by as many columns);
    the rows to reduce are all the others, or the first nrows of them."""
    n, m, ti, tj, tx = sysm
    A = oracle.compress(p, n, m, ti, tj, tx)
    top = ti < npiv
    P = oracle.compress(p, npiv, m, ti[top], tj[top], tx[top])
    found, _, F = oracle.pivots_extract_structural(P, oracle.empty_fact(P.n, P.m, p))
    assert found == npiv and F.U.n == npiv
    rows = np.arange(npiv, n, dtype=np.int32)
    return A, F, np.ascontiguousarray(rows if nrows is None else rows[:nrows])


def _expected_names(env, nnon):
    """(name of the apply kernel, name of the expansion kernel) the statistics must report under `env`"""
    if env is STAGED:
        return "bs_apply_s16_kernel", "bs_expand_kernel<0>"
    if env is TWO_BUFFERS or nnon > WIDEST:
        return "bs_apply_s16_kernel<lds2>", ""
    return "bs_apply_s16_kernel", ""


def _schur(monkeypatch, env, dA, rows, dF, W, nnon):
    """one batch under `env` on the given factor and workspace: (S on the device or None, stats); asserts from the reported
    names which kernels ran"""
    import torch
    monkeypatch.setenv("SPASM_HIP_BACKSOLVE", "1")
    monkeypatch.setenv("SPASM_HIP_BS_SIGNED", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        S, st = spasm_amd.dschur(dA, torch.from_numpy(rows).cuda(), dF, W)
    finally:
        for k in env:
            monkeypatch.delenv(k)
    assert st.used_backsolve == 1
    apply_name, expand_name = _expected_names(env, nnon)
    assert apply_name in (st.kernel.decode(), st.kernel_other.decode())
    assert st.kernel_expand.decode() == expand_name
    return S, st


def _run(monkeypatch, A, F, rows, pool, env, nnon):
    """the batch through the dense image under `env` on a fresh factor and workspace of `pool` entries: (S on the host or
    None, stats, device A, device factor, workspace)"""
    monkeypatch.setenv("SPASM_HIP_BACKSOLVE", "1")          # (read when the factor's image is planned)
    monkeypatch.setenv("SPASM_HIP_BS_SIGNED", "1")
    dA = spasm_amd.DeviceCsr.from_host(_product(A))
    dF = spasm_amd.DeviceFact(spasm_amd.Fact(_product(F.U), F.qinv))
    W = spasm_amd.SchurWorkspace(len(rows), A.m, pool)
    S, st = _schur(monkeypatch, env, dA, rows, dF, W, nnon)
    return (S.to_host() if S is not None else None), st, dA, dF, W


def _three_identical(monkeypatch, A, F, rows, nnon, pool=1 << 22):
    H, st = _run(monkeypatch, A, F, rows, pool, ROWREG, nnon)[:2]
    assert st.status == 0
    for env in (TWO_BUFFERS, STAGED):
        H2, st2 = _run(monkeypatch, A, F, rows, pool, env, nnon)[:2]
        assert st2.status == 0
        assert st.nnz == st2.nnz
        assert np.array_equal(H.p, H2.p)
        assert np.array_equal(H.j, H2.j)
        assert np.array_equal(H.x, H2.x)
    return H, st


@pytest.mark.parametrize("p", [3, 42013, 44927])
@pytest.mark.parametrize("nnon", [1, 511, 512, 513, 1536, 2048, 4952, 5120, 5121])
def test_rowreg_every_instantiation_boundary(oracle, monkeypatch, nnon, p):
    """both sides of an instantiation, the benchmark's width, the last instantiation and the first width past it; at 5,120
    columns the result is the oracle's as well"""
    rng = np.random.default_rng(1000 * nnon + p % 1000)
    A, F, rows = _problem(oracle, p, _system(rng, p, npiv=600, nnon=nnon, nred=300, np_per_row=8, red_entries=10, last_col=True), 600)
    H, _ = _three_identical(monkeypatch, A, F, rows, nnon)
    assert H.j.max() == H.m - 1          # (an entry in the last column)
    if nnon == WIDEST:
        want, _, _ = oracle.schur(A, rows, F)
        assert oracle.same_matrix(oracle.CSR(H.n, H.m, H.p, H.j, H.x, p), want)


@pytest.mark.parametrize("nrows", [1, 2, 63])
def test_rowreg_fewer_rows_than_waves(oracle, monkeypatch, nrows):
    """one row (never handed over before the end), two, and fewer rows than the waves of a single workgroup"""
    p = 42013
    rng = np.random.default_rng(nrows)
    A, F, rows = _problem(oracle, p, _system(rng, p, npiv=800, nnon=500, nred=100), 800, nrows=nrows)
    assert len(rows) == nrows
    H, _ = _three_identical(monkeypatch, A, F, rows, 500)
    want, _, _ = oracle.schur(A, rows, F)
    assert oracle.same_matrix(oracle.CSR(H.n, H.m, H.p, H.j, H.x, p), want)


def test_rowreg_zero_and_empty_rows(oracle, monkeypatch):
    """rows of S that are all zero (copies of pivot rows) and input rows without entries, among ordinary ones"""
    p = 42013
    rng = np.random.default_rng(3)
    A, F, rows = _problem(oracle, p, _system(rng, p, npiv=1200, nnon=200, nred=600, zero_rows=150, empty_rows=100), 1200)
    rng.shuffle(rows)
    H, _ = _three_identical(monkeypatch, A, F, rows, 200)
    assert np.count_nonzero(np.diff(H.p) == 0) >= 250


def test_rowreg_many_short_rows(oracle, monkeypatch):
    """20,000 short rows: every wave hands many rows from LDS to its registers, and rows this short finish faster than their
    predecessors publish, so waves meet the state in which both places hold a pending row"""
    p = 42013
    rng = np.random.default_rng(11)
    A, F, rows = _problem(oracle, p, _system(rng, p, npiv=2000, nnon=700, nred=20000, np_per_row=2, red_entries=4), 2000)
    _, st = _three_identical(monkeypatch, A, F, rows, 700, pool=1 << 26)
    assert st.nnz > 20000


@pytest.mark.parametrize("where", [0.0, 0.5, 0.999])
def test_rowreg_pool_runs_out_mid_batch(oracle, monkeypatch, where):
    """a pool smaller than S: the three outputs raise the overflow status and report the same total, and the workspace is
    intact afterwards: one row that fits the pool comes out as the oracle has it, from the same kernel on the same
    workspace.  That row is an ordinary one, or with a pool of one entry the batch's first row, which reduces to nothing."""
    p = 42013
    rng = np.random.default_rng(23)
    A, F, rows = _problem(oracle, p, _system(rng, p, npiv=1500, nnon=400, nred=2000, zero_rows=1), 1500)
    want, _, _ = oracle.schur(A, rows, F)
    cap = max(1, int(want.nnz * where))
    one = rows[:1] if where == 0.0 else rows[1:2]
    want_one, _, _ = oracle.schur(A, one, F)
    assert want_one.nnz <= cap and (where == 0.0 or want_one.nnz > 0)
    for env in (ROWREG, TWO_BUFFERS, STAGED):
        S, st, dA, dF, W = _run(monkeypatch, A, F, rows, cap, env, 400)
        assert S is None and st.status == 1 and st.nnz == want.nnz
        S1, st1 = _schur(monkeypatch, env, dA, one, dF, W, 400)
        assert st1.status == 0 and st1.nnz == want_one.nnz
        H = S1.to_host()
        assert oracle.same_matrix(oracle.CSR(H.n, H.m, H.p, H.j, H.x, p), want_one)
