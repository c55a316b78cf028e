"""X.A = B on the GPU (spasm_amd/csrc/solve.hip): bit-identical to the compiled reference's spasm_gesv on the stored cases,
correct on the GPU's own factorizations, solve / Solver consistent with gesv across the edges of the 64-wide blocks, a
generated workload at scale, and tools/solve."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ALL_TEST_MATRICES, matrix_path
from test_solve_host import (CASES, as_product_fact, balanced, check_solution, csr_of_dense, dense, mulmod, ref_gesv, rhs_dense,
                             stored_case)

import spasm_amd

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _product(M):
    return spasm_amd.Csr(M.n, M.m, M.p, M.j, M.x, M.prime)


def _oracle_csr(oracle, M):
    return oracle.CSR(M.n, M.m, M.p, M.j, M.x, M.prime)


@pytest.mark.parametrize("name,p,complete", CASES)
def test_gesv_bit_identical_to_the_reference(oracle, name, p, complete):
    A, U, qinv, L, Lp, B, want = stored_case(oracle, name, p, complete)
    X, ok = spasm_amd.gesv(as_product_fact(U, qinv, L, Lp), _product(B))
    assert (X.n, X.m) == (int(want["n"]), int(want["m"]))
    assert np.array_equal(X.p, want["p"])
    assert np.array_equal(X.j, want["j"])
    assert np.array_equal(X.x, want["x"])
    assert np.array_equal(ok.astype(np.uint8), want["ok"])


def _gpu_fact(A, complete, dense_finish):
    o = spasm_amd.default_opts()
    o.L = True
    o.complete = complete
    if dense_finish:
        o.sparsity_threshold = -1.0
        o.dense_block_size = 41
    return spasm_amd.echelonize(_product(A), o)


@pytest.mark.parametrize("name", ALL_TEST_MATRICES)
@pytest.mark.parametrize("p", [257, 4294967291])
@pytest.mark.parametrize("complete,dense_finish", [(False, False), (True, False), (False, True), (True, True)])
def test_gesv_on_the_gpu_factorization(oracle, name, p, complete, dense_finish):
    A = oracle.load_sms(matrix_path(name), p)
    F = _gpu_fact(A, complete, dense_finish)
    B = csr_of_dense(rhs_dense(A, p, seed=11), p, oracle.CSR)
    X, ok = spasm_amd.gesv(F, _product(B))
    assert (X.n, X.m) == (B.n, A.n)
    assert ok[:A.n].all()
    Uo = _oracle_csr(oracle, F.U)
    check_solution(oracle, A, Uo, B, _oracle_csr(oracle, X), ok, Lp=F.Lp)
    if oracle.ref_available():
        Xr, okr = ref_gesv(oracle, Uo, F.qinv, _oracle_csr(oracle, F.L), F.Lp, B)
        assert np.array_equal(okr, ok)
        assert np.array_equal(Xr.p, X.p) and np.array_equal(Xr.j, X.j) and np.array_equal(Xr.x, X.x)


@pytest.mark.parametrize("k", [1, 63, 64, 65, 1000])
def test_solve_and_solver_agree_with_gesv(oracle, k):
    p = 42013
    A = oracle.load_sms(matrix_path("mat364.sms"), p)
    F = _gpu_fact(A, False, False)
    rng = np.random.default_rng(k)
    Ad = dense(A)

    def rhs(seed):
        r = np.random.default_rng(seed)
        coef = r.integers(0, p, size=(k, A.n), dtype=np.int64) * (r.random((k, A.n)) < 0.01)
        D = mulmod(coef, Ad, p)
        noise = (r.random((k, A.m)) < 0.002) * r.integers(1, p, size=(k, A.m), dtype=np.int64)
        D[1::2] = (D[1::2] + noise[1::2]) % p
        return csr_of_dense(D, p, spasm_amd.Csr)

    B1, B2 = rhs(1 + k), rhs(2 + k)
    X1, ok1 = spasm_amd.gesv(F, B1)
    X2, ok2 = spasm_amd.gesv(F, B2)
    with spasm_amd.Solver(F) as S:
        assert S.levels["forward"] >= 1 and S.levels["back"] >= 1
        for B, X, ok in ((B1, X1, ok1), (B2, X2, ok2)):
            Y, oky = S.gesv(B)
            assert np.array_equal(oky, ok)
            assert np.array_equal(Y.p, X.p) and np.array_equal(Y.j, X.j) and np.array_equal(Y.x, X.x)
    Xd = dense(X1) if X1.n else None
    Bd = dense(B1)
    for i in sorted(set(rng.choice(k, size=min(k, 5), replace=False).tolist()) | {0, k - 1}):
        x, okx = spasm_amd.solve(F, balanced(Bd[i], p))
        assert okx == ok1[i]
        assert np.array_equal(x.astype(np.int64) % p, Xd[i])
    check_solution(oracle, A, _oracle_csr(oracle, F.U), _oracle_csr(oracle, B1), _oracle_csr(oracle, X1), ok1,
                   rows=range(0, k, max(1, k // 16)))


def _sparse_rows_times(X, A, rows):
    """rows of X.A mod p, computed on the host with Python integers"""
    p = A.prime
    out = {}
    for i in rows:
        acc = {}
        for jx, vx in zip(*X.row(i)):
            for ja, va in zip(*A.row(int(jx))):
                acc[int(ja)] = (acc.get(int(ja), 0) + int(vx) * int(va)) % p
        out[i] = {c: v for c, v in acc.items() if v}
    return out


def test_gesv_at_scale_mk12_b3(oracle):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import workloads
    A, _ = workloads.load_matrix("mk12.b3")
    p = A.prime
    o = spasm_amd.default_opts()
    o.L = True
    F = spasm_amd.echelonize(A, o)
    k = 1024
    rng = np.random.default_rng(5)
    # half the rows: combinations of 3 rows of A (solvable); the other half: the same plus one entry in a column without a
    # pivot (a non-zero vector of the row space has an entry in some pivot column: these have no solution)
    free = np.flatnonzero(F.qinv < 0)
    assert len(free) > 0
    rows, cols, vals = [], [], []
    for t in range(k):
        acc = {}
        for i in rng.choice(A.n, size=3, replace=False):
            c = int(rng.integers(1, p))
            for j, v in zip(*A.row(int(i))):
                acc[int(j)] = (acc.get(int(j), 0) + c * int(v)) % p
        if t % 2:
            j = int(rng.choice(free))
            acc[j] = (acc.get(j, 0) + int(rng.integers(1, p))) % p
        for j in sorted(acc):
            if acc[j]:
                rows.append(t)
                cols.append(j)
                vals.append(acc[j])
    ptr = np.zeros(k + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=k), out=ptr[1:])
    B = spasm_amd.Csr(k, A.m, ptr, np.array(cols, np.int32), balanced(vals, p), p)
    X, ok = spasm_amd.gesv(F, B)
    assert ok[0::2].all() and not ok[1::2].any()
    sample = sorted(rng.choice(k, size=32, replace=False).tolist())
    prod = _sparse_rows_times(X, A, sample)
    for i in sample:
        want = {int(j): int(v) % p for j, v in zip(*B.row(i))}
        if ok[i]:
            assert prod[i] == want, i
        else:
            assert prod[i] != want, i
    if oracle.ref_available():
        sample = sorted(rng.choice(k, size=64, replace=False).tolist())
        Bs = oracle.CSR(len(sample), B.m, np.concatenate([[0], np.cumsum([B.p[i + 1] - B.p[i] for i in sample])]),
                        np.concatenate([B.row(i)[0] for i in sample]), np.concatenate([B.row(i)[1] for i in sample]), p)
        Xr, okr = ref_gesv(oracle, _oracle_csr(oracle, F.U), F.qinv, _oracle_csr(oracle, F.L), F.Lp, Bs)
        assert np.array_equal(okr, ok[sample])
        for t, i in enumerate(sample):
            a, b = Xr.row(t), X.row(i)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), i


@pytest.mark.parametrize("name", ["mat364.sms", "rectangular_l.sms"])
def test_solve_tool(oracle, name, tmp_path):
    tool = os.path.join(ROOT, "tools", "solve")
    if not os.path.exists(tool):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tools")], check=True)
    p = 42013
    A = oracle.load_sms(matrix_path(name), p)
    D = rhs_dense(A, p, seed=3)[A.n:]
    B = csr_of_dense(D, p, oracle.CSR)
    rhs = tmp_path / "rhs.sms"
    with open(rhs, "w") as f:
        f.write("%d %d M\n" % (B.n, B.m))
        for i in range(B.n):
            for j, v in zip(*B.row(i)):
                f.write("%d %d %d\n" % (i + 1, int(j) + 1, int(v)))
        f.write("0 0 0\n")
    out = tmp_path / "x.sms"
    env = dict(os.environ, SPASM_HIP_VERBOSE="0")
    res = subprocess.run([tool, "--matrix", matrix_path(name), "--modulus", str(p), "--rhs", str(rhs), "--output", str(out)],
                         capture_output=True, text=True, env=env, timeout=300)
    assert res.returncode == 0, res.stderr
    X = oracle.load_sms(str(out), p)
    assert (X.n, X.m) == (B.n, A.n)
    warned = {int(line.split()[-1]) for line in res.stderr.splitlines() if line.startswith("WARNING: no solution for row")}
    F = oracle.echelonize(A)
    ok = np.array([i not in warned for i in range(B.n)])
    check_solution(oracle, A, F.U, B, X, ok)
