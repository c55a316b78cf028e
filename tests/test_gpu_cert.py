"""Rank certificates on the GPU (spasm_amd/csrc/host_cert.cpp over spmv.hip and solve.hip): bit-identical to the compiled
reference's certificate on every stored case, the reference's verdict on the certificate and on each single mutation of it,
the checks of the GPU's own factorizations, x.A against numpy, tools/rank --certificate with tools/check_cert, and a
generated workload at scale."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import ALL_TEST_MATRICES, matrix_path
from test_cert_host import CERT_CASES, MUTATIONS, mutate, stored_cert_case
from test_solve_host import SOLVE_MODULI, as_product_fact, mulmod

import spasm_amd

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEEDS = (42, 1337, 21011984)          # tools/rank.c:107-109


def _product(M):
    return spasm_amd.Csr(M.n, M.m, M.p, M.j, M.x, M.prime)


@pytest.mark.parametrize("name,p", CERT_CASES)
def test_create_is_bit_identical_to_the_reference(oracle, name, p, tmp_path):
    A, hash, fact, want, _ = stored_cert_case(oracle, name, p, str(tmp_path))
    got = spasm_amd.certificate_rank_create(_product(A), hash, as_product_fact(*fact))
    assert got.r == want.r and got.prime == want.prime and got.hash == want.hash
    assert np.array_equal(got.i, want.i) and np.array_equal(got.j, want.j)
    assert np.array_equal(got.x, want.x), "x differs from the reference's"
    assert np.array_equal(got.y, want.y), "y differs from the reference's"


@pytest.mark.parametrize("name,p", CERT_CASES)
def test_verify_gives_the_references_verdicts(oracle, name, p, tmp_path):
    A, hash, fact, cert, stored = stored_cert_case(oracle, name, p, str(tmp_path))
    Ap = _product(A)
    v = stored["verdicts"]
    assert spasm_amd.certificate_rank_verify(Ap, hash, cert) is True
    for t, which in enumerate(MUTATIONS):
        c = mutate(cert, which, A.n)
        if c is None:
            continue
        assert int(spasm_amd.certificate_rank_verify(Ap, hash, c)) == int(v[1 + t]), which


def _gpu_fact(A, dense_finish):
    o = spasm_amd.default_opts()
    o.L = True
    if dense_finish:
        o.sparsity_threshold = -1.0
        o.dense_block_size = 41
    return spasm_amd.echelonize(_product(A), o)


def _bump(M, k):
    """a copy of M with entry k changed (+1 mod p)"""
    x = M.x.copy()
    w = (int(x[k]) + 1) % M.prime
    x[k] = w - M.prime if w > M.prime // 2 else w
    return spasm_amd.Csr(M.n, M.m, M.p.copy(), M.j.copy(), x, M.prime)


@pytest.mark.parametrize("name", ALL_TEST_MATRICES)
@pytest.mark.parametrize("p", [257, 4294967291])
@pytest.mark.parametrize("dense_finish", [False, True])
def test_gpu_factorization_checks_and_certifies(oracle, name, p, dense_finish):
    A = oracle.load_sms(matrix_path(name), p)
    Ap = _product(A)
    F = _gpu_fact(A, dense_finish)
    assert spasm_amd.factorization_verify(Ap, F, SEEDS) == [True, True, True]
    assert spasm_amd.factorization_verify(Ap, F, 7) is True
    hash = bytes(range(32))
    cert = spasm_amd.certificate_rank_create(Ap, hash, F)
    assert cert.r == F.U.n
    assert spasm_amd.certificate_rank_verify(Ap, hash, cert)
    if F.U.nnz:
        Fu = spasm_amd.Fact(_bump(F.U, F.U.nnz // 2), F.qinv, L=F.L, Lp=F.Lp)
        assert not all(spasm_amd.factorization_verify(Ap, Fu, SEEDS))
    # an entry of L on a pivotal row (x vanishes on the other rows: a change there is invisible by design)
    piv = set(np.asarray(F.Lp[:F.U.n]).tolist())
    ks = [k for i in sorted(piv) for k in range(int(F.L.p[i]), int(F.L.p[i + 1]))]
    if ks:
        Fl = spasm_amd.Fact(F.U, F.qinv, L=_bump(F.L, ks[len(ks) // 2]), Lp=F.Lp)
        assert not all(spasm_amd.factorization_verify(Ap, Fl, SEEDS))


def _edge_matrix(p, rng):
    """n = 300 rows: column 0 holds every row, columns 1..40 one entry each, columns 41..49 none, 50..249 random (2 to 60
    entries: both sides of the short / long split)"""
    n, m = 300, 250
    rows, cols = [np.arange(n)], [np.zeros(n, np.int64)]
    rows.append(rng.integers(0, n, 40))
    cols.append(np.arange(1, 41))
    for j in range(50, m):
        c = int(rng.integers(2, 61))
        rows.append(rng.choice(n, c, replace=False))
        cols.append(np.full(c, j))
    ti, tj = np.concatenate(rows), np.concatenate(cols)
    D = np.zeros((n, m), np.int64)
    D[ti, tj] = rng.integers(1, p, len(ti), dtype=np.int64)
    return D


def _csr(D, p):
    n, m = D.shape
    r, c = np.nonzero(D)
    ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=n), out=ptr[1:])
    v = D[r, c] % p
    return spasm_amd.Csr(n, m, ptr, c.astype(np.int32), np.where(v > p // 2, v - p, v).astype(np.int32), p)


@pytest.mark.parametrize("p", SOLVE_MODULI)
@pytest.mark.parametrize("k", [1, 2, 3, 63, 64])
def test_xApy_against_numpy(p, k):
    rng = np.random.default_rng(k * 1009 + p % 1000)
    D = _edge_matrix(p, rng)
    A = _csr(D, p)
    X = rng.integers(0, p, (k, A.n), dtype=np.int64)
    Y0 = rng.integers(0, p, (k, A.m), dtype=np.int64)
    got = spasm_amd.xApy(X, A, Y0)
    want = (mulmod(X, D, p) + Y0) % p
    assert np.array_equal(np.asarray(got, np.int64) % p, want)
    assert np.all(np.abs(got.astype(np.int64)) <= p // 2)
    st = spasm_amd.xApy_stats()
    assert st["k"] == k and st["long_columns"] >= 1 and st["short_columns"] >= 1
    if k == 1:
        assert np.array_equal(np.asarray(spasm_amd.xApy(X[0], A), np.int64) % p, mulmod(X[:1], D, p)[0])


@pytest.mark.parametrize("shape", [(0, 5), (5, 0), (0, 0), (7, 3)])
def test_xApy_on_empty_matrices(shape):
    p = 65537
    n, m = shape
    A = spasm_amd.Csr(n, m, np.zeros(n + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32), p)
    Y0 = np.arange(2 * m, dtype=np.int64).reshape(2, m)
    got = spasm_amd.xApy(np.ones((2, n), np.int64), A, Y0)
    assert got.shape == (2, m) and np.array_equal(got, Y0)


def _tool(name):
    path = os.path.join(ROOT, "tools", name)
    assert os.path.exists(path), "%s not built (make -C tools)" % path
    return path


@pytest.mark.parametrize("name", ["mat364.sms", "rectangular_l.sms"])
def test_rank_certificate_then_check_cert(name, tmp_path):
    cert = str(tmp_path / "c.cert")
    mat = matrix_path(name)
    r = subprocess.run([_tool("rank"), "--matrix", mat, "--modulus", "42013", "--certificate", "-o", cert], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "CORRECT certificate" in r.stderr and "INCORRECT" not in r.stderr
    c = subprocess.run([_tool("check_cert"), "--matrix", mat, "--modulus", "42013", "--certificate", cert], capture_output=True,
                       text=True, timeout=300)
    assert c.returncode == 0 and "CORRECT certificate" in c.stderr and "INCORRECT" not in c.stderr, c.stderr
    lines = open(cert).read().split("\n")
    xs = lines[5].split()
    xs[0] = str(int(xs[0]) + 1)                           # one value of x
    lines[5] = " ".join(xs) + " "
    bad = str(tmp_path / "bad.cert")
    with open(bad, "w") as fh:
        fh.write("\n".join(lines))
    c = subprocess.run([_tool("check_cert"), "--matrix", mat, "--modulus", "42013", "--certificate", bad], capture_output=True,
                       text=True, timeout=300)
    assert c.returncode == 1 and "INCORRECT certificate" in c.stderr, c.stderr


def test_certificate_at_scale_mk13_b5():
    """mk13.b5 (rank 134,211), generated: create + verify on the GPU factorization with L; times printed, not asserted"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import workloads
    A, source = workloads.load_matrix("mk13.b5")
    o = spasm_amd.default_opts()
    o.L = True
    t0 = time.perf_counter()
    F = spasm_amd.echelonize(A, o)
    t1 = time.perf_counter()
    hash = bytes(range(100, 132))
    assert spasm_amd.factorization_verify(A, F, SEEDS) == [True, True, True]
    t2 = time.perf_counter()
    cert = spasm_amd.certificate_rank_create(A, hash, F)
    t3 = time.perf_counter()
    assert cert.r == 134211
    assert spasm_amd.certificate_rank_verify(A, hash, cert)
    t4 = time.perf_counter()
    print("mk13.b5 (%s): echelonize with L %.2f s, factorization checks %.3f s, create %.3f s, verify %.3f s"
          % (source, t1 - t0, t2 - t1, t3 - t2, t4 - t3))
