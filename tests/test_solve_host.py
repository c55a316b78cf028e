"""X.A = B over the PLUQ factorization (spasm_gesv, spasm_solve.c:52): what the compiled reference returns on the suite's
matrices, stored in tests/golden/reference/gesv.npz, checked for what it must be (X.A == B on the rows with a solution, ok
false exactly where b leaves the row space of U); the exported symbols; the reference's own tools/solve.c linked against
the facade; the Python entry points refuse before they reach C.  The GPU side is tests/test_gpu_solve.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ALL_TEST_MATRICES, csr_arrays, matrix_path, reference_vectors

import spasm_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOLVE_MODULI = [3, 257, 42013, 65537, 4294967291]
REF_TREE = "/root/reference"


# ---- helpers shared with tests/test_gpu_solve.py ----
def mulmod(X, Y, p):
    """X . Y mod p for int64 matrices with entries in [0, p), p < 2^32, without overflow (Y split in 16-bit halves)."""
    X = np.asarray(X, np.int64) % p
    Y = np.asarray(Y, np.int64) % p
    if X.shape[1] == 0:
        return np.zeros((X.shape[0], Y.shape[1]), np.int64)
    lo, hi = Y & 0xFFFF, Y >> 16
    out = np.zeros((X.shape[0], Y.shape[1]), np.int64)
    for k0 in range(0, X.shape[1], 256):            # 256 terms of < 2^48 stay below 2^56
        Xs = X[:, k0:k0 + 256]
        a = (Xs @ lo[k0:k0 + 256]) % p
        b = (Xs @ hi[k0:k0 + 256]) % p
        out = (out + a + (b << 16) % p) % p
    return out


def dense(A):
    D = np.zeros((A.n, A.m), np.int64)
    for i in range(A.n):
        lo, hi = int(A.p[i]), int(A.p[i + 1])
        np.add.at(D[i], A.j[lo:hi].astype(np.int64), A.x[lo:hi].astype(np.int64))
    return D % A.prime


def balanced(v, p):
    v = np.asarray(v, np.int64) % p
    return np.where(v > p // 2, v - p, v).astype(np.int32)


def csr_of_dense(D, p, cls):
    D = np.asarray(D, np.int64) % p
    n, m = D.shape
    rows, cols = np.nonzero(D)
    ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=ptr[1:])
    return cls(n, m, ptr, cols.astype(np.int32), balanced(D[rows, cols], p), p)


def rhs_dense(A, p, seed):
    """the right-hand sides of a case (fixed seed): the rows of A, four random combinations of rows of A, four random sparse
    rows, a zero row, and the first combination again"""
    rng = np.random.default_rng(seed)
    Ad = dense(A)
    n, m = Ad.shape
    combos = np.zeros((4, m), np.int64)
    if n:
        for t in range(4):
            rows = rng.choice(n, size=min(n, 1 + t), replace=False)
            coef = rng.integers(1, p, size=(1, len(rows)), dtype=np.int64)
            combos[t] = mulmod(coef, Ad[rows], p)[0]
    sparse = np.zeros((4, m), np.int64)
    if m:
        for t in range(4):
            cols = rng.choice(m, size=min(m, 1 + 2 * t), replace=False)
            sparse[t, cols] = rng.integers(1, p, size=len(cols), dtype=np.int64)
    return np.vstack([Ad, combos, sparse, np.zeros((1, m), np.int64), combos[:1]])


def oracle_fact(oracle, A, complete):
    """deterministic CPU factorization with L (oracle.echelonize, opts.L = 1): (U, qinv, L as a CSR rows of A x rank, Lp)"""
    o = oracle.default_opts()
    o.L = 1
    o.complete = 1 if complete else 0
    F = oracle.echelonize(A, o)
    r = F.U.n
    Li, Lj, Lx = F.L if F.L is not None else (np.zeros(0, np.int32),) * 3
    L = oracle.compress(A.prime, A.n, r, np.asarray(Li), np.asarray(Lj), np.asarray(Lx))
    return F.U, F.qinv, L, np.ascontiguousarray(F.Lp[:r], np.int32)


def as_product_fact(U, qinv, L, Lp):
    P = lambda M: spasm_amd.Csr(M.n, M.m, M.p, M.j, M.x, M.prime)       # noqa: E731
    return spasm_amd.Fact(P(U), qinv, L=P(L), Lp=Lp)


def ref_gesv(oracle, U, qinv, L, Lp, B):
    """the compiled reference's spasm_gesv on this factorization: (X as an oracle.CSR, ok)"""
    R = oracle.ref()
    R.spasm_gesv.restype = C.POINTER(oracle._RefCsr)
    R.spasm_gesv.argtypes = [C.POINTER(oracle._RefLu), C.POINTER(oracle._RefCsr), C.POINTER(C.c_bool)]
    oracle.ref_set_threads(1)
    lu, up, q = oracle._ref_lu(oracle.Fact(U, qinv), 0)
    lp = oracle._ref_to(L)
    pp = np.ascontiguousarray(Lp, np.int32).copy() if len(Lp) else np.zeros(1, np.int32)
    lu.L = lp
    lu.p = pp.ctypes.data_as(C.POINTER(C.c_int))
    b = oracle._ref_to(B)
    ok = np.zeros(max(B.n, 1), np.bool_)
    saved = oracle._silence()
    try:
        x = R.spasm_gesv(C.byref(lu), b, ok.ctypes.data_as(C.POINTER(C.c_bool)))
    finally:
        oracle._unsilence(saved)
    X = oracle._ref_from(x)
    for ptr in (x, b, lp, up):
        R.spasm_csr_free(ptr)
    return X, ok[:B.n].copy()


def in_row_space(oracle, U, b, p):
    """rank([U; b]) == rank(U), by the oracle's own echelonization"""
    D = np.vstack([dense(U), np.asarray(b, np.int64).reshape(1, -1) % p]) if U.m else np.zeros((U.n + 1, 0), np.int64)
    S = csr_of_dense(D, p, oracle.CSR)
    return oracle.echelonize(S).U.n == U.n


def check_solution(oracle, A, U, B, X, ok, Lp=None, rows=None):
    """X.A == B on the rows with ok, ok == (b in the row space of U), the support of X inside Lp"""
    p = A.prime
    rows = range(B.n) if rows is None else rows
    Ad, Bd = dense(A), dense(B)
    for i in rows:
        lo, hi = int(X.p[i]), int(X.p[i + 1])
        if ok[i]:
            xa = np.zeros((1, A.n), np.int64)
            xa[0, X.j[lo:hi]] = X.x[lo:hi]
            assert np.array_equal(mulmod(xa, Ad, p)[0], Bd[i]), "row %d: x.A != b" % i
        assert bool(ok[i]) == in_row_space(oracle, U, Bd[i], p), "row %d: ok is wrong" % i
        if Lp is not None:
            assert set(X.j[lo:hi].tolist()) <= set(np.asarray(Lp).tolist())
        assert np.all(np.diff(X.j[lo:hi]) > 0), "row %d: columns not increasing" % i


def stored_case(oracle, name, p, complete):
    """(A, U, qinv, L, Lp, B, {X arrays, ok}) of one stored case"""
    A = oracle.load_sms(matrix_path(name), p)
    U, qinv, L, Lp = oracle_fact(oracle, A, complete)
    B = csr_of_dense(rhs_dense(A, p, seed=(sum(map(ord, name)) * 7919 + p) % 2**32), p, oracle.CSR)

    def live():
        X, ok = ref_gesv(oracle, U, qinv, L, Lp, B)
        return dict(csr_arrays(X), ok=ok.astype(np.uint8), rank=np.int64(U.n))

    want = reference_vectors(oracle, "gesv", "%s|%d|%d" % (name, p, int(complete)), live)
    return A, U, qinv, L, Lp, B, want


CASES = [(name, p, complete) for name in ALL_TEST_MATRICES for p in SOLVE_MODULI for complete in (False, True)]


@pytest.mark.parametrize("name,p,complete", CASES)
def test_stored_gesv_solves_the_system(oracle, name, p, complete):
    A, U, qinv, L, Lp, B, want = stored_case(oracle, name, p, complete)
    assert int(want["rank"]) == U.n
    X = oracle.CSR(int(want["n"]), int(want["m"]), want["p"], want["j"], want["x"], p)
    assert (X.n, X.m) == (B.n, A.n)
    ok = want["ok"].astype(bool)
    assert ok[:A.n].all()                                   # B = A: every row of A lies in the row space
    Xd = dense(X) if X.n else np.zeros((0, A.n), np.int64)
    assert np.array_equal(mulmod(Xd[:A.n], dense(A), p), dense(A))
    zero = A.n + 8
    assert ok[zero] and X.p[zero] == X.p[zero + 1]          # the zero row: x = 0
    assert ok[zero + 1] == ok[A.n] and np.array_equal(Xd[zero + 1], Xd[A.n])   # a repeated row, the same answer
    check_solution(oracle, A, U, B, X, ok, Lp=Lp, rows=range(A.n, B.n))


def test_library_exports_the_solve_entry_points():
    out = subprocess.run(["nm", "-D", "--defined-only", spasm_amd.LIB_PATH], check=True, capture_output=True, text=True).stdout
    names = {line.split()[-1] for line in out.splitlines()}
    for sym in ("spasm_hip_solve", "spasm_hip_gesv", "spasm_hip_solver_create", "spasm_hip_solver_gesv", "spasm_hip_solver_destroy",
                "spasm_hip_solver_levels", "spasm_hip_solver_stats"):
        assert sym in names, sym
    facade = os.path.join(os.path.dirname(spasm_amd.LIB_PATH), "libspasm_hip_facade.so")
    out = subprocess.run(["nm", "-D", "--defined-only", facade], check=True, capture_output=True, text=True).stdout
    names = {line.split()[-1] for line in out.splitlines()}
    assert "spasm_gesv" in names
    # spasm_solve stays the reference's: its certificate code calls it from inside its own library (facade.c)
    assert "spasm_solve" not in names


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF_TREE, "tools")), reason="the reference tree is not on this machine")
def test_reference_solve_c_links_against_the_facade(tmp_path):
    """the reference's own tools/solve.c + common.c, unmodified, against the facade (spasm_echelonize, spasm_gesv from the GPU
    library) and the reference's library (the rest): every spasm_* symbol resolves"""
    ref_lib_dir = os.path.join(ROOT, "oracle", "_ref")
    if not os.path.exists(os.path.join(ref_lib_dir, "libspasm_ref.so")):
        pytest.skip("oracle/_ref/libspasm_ref.so not built")
    hip_dir = os.path.dirname(spasm_amd.LIB_PATH)
    exe = str(tmp_path / "ref_solve_facade")
    subprocess.run(["gcc", "-O2", "-std=gnu99", "-I" + os.path.join(REF_TREE, "src"), os.path.join(REF_TREE, "tools", "solve.c"),
                    os.path.join(REF_TREE, "tools", "common.c"), "-o", exe, "-L" + hip_dir, "-lspasm_hip_facade",
                    "-L" + ref_lib_dir, "-lspasm_ref", "-lm", "-fopenmp", "-Wl,-rpath," + hip_dir, "-Wl,-rpath," + ref_lib_dir,
                    "-Wl,--no-undefined"], check=True, capture_output=True)
    need = {line.split()[-1] for line in subprocess.run(["nm", "-D", "--undefined-only", exe], check=True, capture_output=True,
                                                         text=True).stdout.splitlines() if "spasm" in line}
    facade = os.path.join(hip_dir, "libspasm_hip_facade.so")
    have = set()
    for lib in (facade, os.path.join(ref_lib_dir, "libspasm_ref.so")):
        have |= {line.split()[-1] for line in subprocess.run(["nm", "-D", "--defined-only", lib], check=True, capture_output=True,
                                                             text=True).stdout.splitlines()}
    assert "spasm_gesv" in need and need <= have, need - have
    out = subprocess.run(["ldd", exe], check=True, capture_output=True, text=True).stdout
    assert "not found" not in out


def test_python_entry_points_refuse_before_c(oracle):
    """a Fact without L, a B of the wrong width or modulus: ValueError; without a GPU: RuntimeError -- never an exit"""
    p = 42013
    A = oracle.load_sms(matrix_path("mat364.sms"), p)
    U, qinv, L, Lp = oracle_fact(oracle, A, False)
    F = as_product_fact(U, qinv, L, Lp)
    B = csr_of_dense(rhs_dense(A, p, 1)[-6:], p, spasm_amd.Csr)
    with pytest.raises(ValueError):
        spasm_amd.gesv(spasm_amd.Fact(F.U, F.qinv), B)
    with pytest.raises(ValueError):
        spasm_amd.solve(spasm_amd.Fact(F.U, F.qinv), np.zeros(A.m, np.int32))
    with pytest.raises(ValueError):
        spasm_amd.gesv(F, spasm_amd.Csr(B.n, B.m + 1, B.p, B.j, B.x, p))
    with pytest.raises(ValueError):
        spasm_amd.gesv(F, spasm_amd.Csr(B.n, B.m, B.p, B.j, B.x, 257))
    with pytest.raises(ValueError):
        spasm_amd.Solver(spasm_amd.Fact(F.U, F.qinv))
    if spasm_amd.device_count() == 0:
        with pytest.raises(RuntimeError):
            spasm_amd.gesv(F, B)
        with pytest.raises(RuntimeError):
            spasm_amd.solve(F, np.zeros(A.m, np.int32))
        with pytest.raises(RuntimeError):
            spasm_amd.Solver(F)
