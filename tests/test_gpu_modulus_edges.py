"""The kernels on both sides of every modulus switch (tests/modulus_edges.py), with data that takes each arithmetic to its
bound: sums of thousands of equal residues into one entry, operands of magnitude (p - 1) / 2 in the dense updates.  Every
answer is checked against Python integers or the CPU oracle, never against another GPU path, and every test asserts
through the statistics that the path it aims at is the one that ran."""
import numpy as np
import pytest

from conftest import matrix_path
from modulus_edges import MAXDEG_PAIRS, dense_of_sparse_rows, half, narrow_dense, star, star_factor, _sgn_ok
from test_gpu_dense import _extend_and_check
from test_solve_host import csr_of_dense, mulmod

import spasm_amd

pytestmark = pytest.mark.gpu

ROWS_ONLY = {"SPASM_HIP_BACKSOLVE": "0", "SPASM_HIP_SPARSE_IMAGE": "0"}


def _product(M):
    return spasm_amd.Csr(M.n, M.m, M.p, M.j, M.x, M.prime)


def _star_on_device(oracle, monkeypatch, env, p, K, C, nred, x=1, u=1, a_seed=1):
    """the star's Schur complement through spasm_hip_dschur under `env`: checked against the closed form, returns the stats"""
    import torch
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    n, m, ti, tj, tx, want = star(p, K, C=C, nred=nred, x=x, u=u, a_seed=a_seed)
    A, F, rows = star_factor(oracle, p, n, m, K, ti, tj, tx)
    dA = spasm_amd.DeviceCsr.from_host(_product(A))
    dF = spasm_amd.DeviceFact(spasm_amd.Fact(_product(F.U), F.qinv))
    W = spasm_amd.SchurWorkspace(nred, m, 4 * nred * C + (1 << 20))
    S, st = spasm_amd.dschur(dA, torch.from_numpy(rows).cuda(), dF, W)
    assert st.status == 0 and st.rows == nred
    H = S.to_host()
    assert np.all(np.abs(H.x.astype(np.int64)) <= p // 2)
    assert np.array_equal(dense_of_sparse_rows(H, K, C), want)
    return st


def _kernel_names(st):
    return {st.kernel.decode(), st.kernel_other.decode()}


# --------------------------------------------------------------------------
# 1. row-by-row Schur: LDS tables (narrow below p * 6146 = 2^32) and dense accumulators (narrow below 2p(maxdeg + 3) = 2^32)
# --------------------------------------------------------------------------
@pytest.mark.parametrize("p", [698821, 698827, 2147483659, 4294967291])
def test_small_lds_table_star(oracle, monkeypatch, p):
    """440 terms of p - 1 into one slot of the small table (its pending list holds 448 labels)"""
    st = _star_on_device(oracle, monkeypatch, ROWS_ONLY, p, K=440, C=2, nred=64)
    assert st.rows_lds == 64 and st.rows_lds_big == 0 and st.rows_dense == 0


@pytest.mark.parametrize("p", [698821, 698827, 800011, 1100009, 4294967291])
def test_large_lds_table_star(oracle, monkeypatch, p):
    """4,000 terms of p - 1 into one slot of the large table: from 1,073,742 on their exact sum passes 2^32, so narrow
    32-bit sums there would wrap"""
    st = _star_on_device(oracle, monkeypatch, dict(ROWS_ONLY, SPASM_HIP_FORCE_TIER="1"), p, K=4000, C=2, nred=16)
    assert st.rows_lds_big == 16 and st.rows_lds == 0 and st.rows_dense == 0


@pytest.mark.parametrize("p,K", MAXDEG_PAIRS)
@pytest.mark.parametrize("mode", ["dense_tier", "group"])
def test_dense_accumulators_at_the_maxdeg_bound(oracle, monkeypatch, p, K, mode):
    """a star of K pivot rows has column degree K: the narrow / wide accumulators flip between K = 8 and 9 at 195,225,781;
    the last pairs are wide with K (p - 1) >= 2^32"""
    wide = "false" if narrow_dense(p, K) else "true"
    env = dict(ROWS_ONLY, **({"SPASM_HIP_FORCE_TIER": "2"} if mode == "dense_tier" else {"SPASM_HIP_GROUP": "1"}))
    st = _star_on_device(oracle, monkeypatch, env, p, K=K, C=3, nred=128)
    if mode == "dense_tier":
        assert st.kernel.decode() == "schur_wave_dense_kernel<%s>" % wide
        assert st.rows_dense == 128 and st.used_group_kernel == 0
    else:
        assert st.used_group_kernel == 1 and st.group_aborted == 0
        assert st.kernel.decode().startswith("schur_group_kernel<%s," % wide)


# --------------------------------------------------------------------------
# 2. back-substituted (dense) image and sparse image: 3,000-term dot products of +-(p - 1)/2
# --------------------------------------------------------------------------
IMAGE_PRIMES = [42013, 44927, 44939, 46337, 65521, 65537, 2147483647, 2147483659, 4294967291]


@pytest.mark.parametrize("p", IMAGE_PRIMES)
@pytest.mark.parametrize("path", ["backsolve_signed", "backsolve_unsigned", "sparse_image"])
@pytest.mark.parametrize("sign", [1, -1])
def test_images_long_dot_products_of_extreme_values(oracle, monkeypatch, p, path, sign):
    """every entry of S is a_c - 3000 x u with x = sign (p - 1)/2 and u = (p - 1)/2: 3,000 products of one sign"""
    h = half(p)
    if path == "sparse_image":
        env = {"SPASM_HIP_SPARSE_IMAGE": "1"}
    else:
        env = {"SPASM_HIP_SPARSE_IMAGE": "0", "SPASM_HIP_BACKSOLVE": "1",
               "SPASM_HIP_BS_SIGNED": "1" if path == "backsolve_signed" else "0"}
    st = _star_on_device(oracle, monkeypatch, env, p, K=3000, C=40, nred=200, x=sign * h, u=h, a_seed=p % 1000)
    if path == "sparse_image":
        assert st.used_sparse_image == 1 and st.used_backsolve == 0
        return
    assert st.used_backsolve == 1 and st.used_sparse_image == 0
    names = _kernel_names(st)
    if p < 65536 and _sgn_ok(p) and path == "backsolve_signed":
        assert "bs_apply_s16_kernel" in names
    else:
        apply = [k for k in names if k.startswith("bs_apply_kernel<")]
        assert len(apply) == 1 and apply[0].endswith(",%s>" % ("true" if p < 65536 else "false"))


# --------------------------------------------------------------------------
# 3. the dense tail: RREF, LU, row-panel echelon extend, dense Schur rows
# --------------------------------------------------------------------------
DENSE_PRIMES = [3, 251, 257, 44927, 44939, 46337, 46349, 65269, 65287, 65521, 65537, 2147483647, 2147483659]
N_ID, N_LOW, W_RIGHT = 512, 96, 160


def _adversarial(p, case):
    """[I B; M C]: an identity block of 512 columns (a full multi-panel update of the rows below it), B and M all (p - 1)/2
    (or B = -(p - 1)/2: a negative sum), C random -- every entry of C - M B is a 512-term sum of products of one sign"""
    h = half(p)
    M = np.zeros((N_ID + N_LOW, N_ID + W_RIGHT), np.int64)
    M[:N_ID, :N_ID] = np.eye(N_ID, dtype=np.int64)
    M[:N_ID, N_ID:] = h if case == "same_sign" else (p - h) % p
    M[N_ID:, :N_ID] = h
    M[N_ID:, N_ID:] = np.random.default_rng(p % 9973).integers(0, p, size=(N_LOW, W_RIGHT))
    return M


def _low_rank(p, n, m, rank, seed):
    rng = np.random.default_rng(seed)
    L = rng.integers(0, p, size=(n, rank), dtype=np.int64)
    R = rng.integers(0, p, size=(rank, m), dtype=np.int64)
    M = mulmod(L, R, p)
    M[:, : m // 7] = 0
    return M


_CASES = {}


def _case(oracle, p, case):
    """(M, oracle rank, R, q), computed once per prime and case"""
    if (p, case) not in _CASES:
        M = _low_rank(p, 300, 520, 200, p % 1013) if case == "low_rank" else _adversarial(p, case)
        _CASES[(p, case)] = (M,) + tuple(oracle.dense_rref(p, M))
    return _CASES[(p, case)]


@pytest.mark.parametrize("p", DENSE_PRIMES)
@pytest.mark.parametrize("case", ["low_rank", "same_sign", "negative_sum"])
@pytest.mark.parametrize("mfma,lookahead", [("1", "1"), ("1", "0"), ("0", "1"), ("0", "0")])
def test_rref_at_the_modulus_edges(oracle, monkeypatch, p, case, mfma, lookahead):
    monkeypatch.setenv("SPASM_HIP_RREF_MFMA", mfma)
    monkeypatch.setenv("SPASM_HIP_RREF_LOOKAHEAD", lookahead)
    M, r_want, R_want, q_want = _case(oracle, p, case)
    r, R, q = spasm_amd.ffpack_rref(p, M)
    assert r == r_want
    assert np.array_equal(q, q_want)
    assert np.array_equal(np.mod(R[:r], p), np.mod(R_want[:r], p))
    assert not np.any(R[r:])


def _check_lu(p, M, r_want):
    """L U == M mod p: L and U rebuilt from the packed result (tests/dense_lu_ffpack.c:80-170), products exact in int64"""
    n, m = M.shape
    r, R, P, Q = spasm_amd.ffpack_LU(p, M)
    assert r == r_want
    assert sorted(P.tolist()) == list(range(n)) and sorted(Q.tolist()) == list(range(m))
    R = np.mod(np.asarray(R, np.int64), p)
    Lm = np.zeros((n, r), np.int64)
    Um = np.zeros((r, m), np.int64)
    Lm[P] = np.where(np.tril(np.ones((n, r), bool)), R[:, :r], 0)
    Um[:, Q] = np.where(np.triu(np.ones((r, m), bool), 1), R[:r, :], 0) + np.eye(r, m, dtype=np.int64)
    assert np.array_equal(mulmod(Lm, Um, p), np.mod(M, p))


@pytest.mark.parametrize("p,blocked", [(p, b) for p in DENSE_PRIMES for b in (("1", "0") if p <= 65279 else ("1",))])
@pytest.mark.parametrize("case", ["low_rank", "same_sign", "negative_sum"])
def test_LU_at_the_modulus_edges(oracle, monkeypatch, p, case, blocked):
    """blocked steps (64 pivots per round, trailing update on the matrix cores) up to 65,279, single steps everywhere"""
    monkeypatch.setenv("SPASM_HIP_LU_BLOCKED", blocked)
    M, r_want, _, _ = _case(oracle, p, case)
    _check_lu(p, M, r_want)


@pytest.mark.parametrize("p", [3, 251, 257, 44927, 44939, 46337, 46349, 65269])
@pytest.mark.parametrize("case", ["same_sign", "negative_sum", "low_rank"])
def test_echelon_extend_at_the_modulus_edges(oracle, p, case):
    """the row-panel echelon extend (p <= 65,279; below 256 without the 24-bit Barrett quotient): the [I B] rows first, then
    the [M C] rows that the 512 pivots of the first block reduce -- against the oracle's RREF of the stack"""
    import torch
    M, _, _, _ = _case(oracle, p, case)
    T = torch.from_numpy(M.astype(np.int32)).cuda()
    cut = N_ID if case != "low_rank" else 150
    _extend_and_check(p, [T[:cut], T[cut:]], M.shape[1], oracle)


@pytest.mark.parametrize("p", DENSE_PRIMES + [4294967291])
@pytest.mark.parametrize("sign", [1, -1])
def test_schur_dense_star(oracle, p, sign):
    h = half(p)
    K, C, nred = 2000, 70, 130
    n, m, ti, tj, tx, want = star(p, K, C=C, nred=nred, x=sign * h, u=h, a_seed=7)
    A, F, rows = star_factor(oracle, p, n, m, K, ti, tj, tx)
    S, q, p_out = spasm_amd.schur_dense(_product(A), rows, spasm_amd.Fact(_product(F.U), F.qinv))
    assert np.array_equal(np.asarray(q, np.int64), np.arange(K, K + C)) and np.array_equal(p_out, rows)
    assert np.array_equal(np.mod(np.asarray(S, np.int64), p), want)


# --------------------------------------------------------------------------
# 4. x.A and solve with p around 2^31 and at the largest prime below 2^32
# --------------------------------------------------------------------------
BIG = [2147483647, 2147483659, 4294967291]


@pytest.mark.parametrize("p", BIG)
def test_xA_long_column_of_extreme_values(p):
    """a column of 100,000 entries p - 1 (one wave per long column), one of (p - 1)/2, one of -(p - 1)/2, and short columns"""
    n, h = 100000, half(p)
    cols = [np.zeros(n, np.int64), np.ones(n, np.int64), np.full(n, 2, np.int64), 3 + np.arange(n) % 5]
    vals = [np.full(n, p - 1, np.int64), np.full(n, h, np.int64), np.full(n, p - h, np.int64), np.full(n, p - 1, np.int64)]
    j = np.stack(cols, 1).ravel().astype(np.int32)
    x = np.stack(vals, 1).ravel()
    x = np.where(x > p // 2, x - p, x).astype(np.int32)
    A = spasm_amd.Csr(n, 8, np.arange(0, 4 * n + 1, 4, dtype=np.int64), j, x, p)
    X = np.stack([np.full(n, p - 1, np.int64), np.full(n, h, np.int64)])
    got = np.mod(np.asarray(spasm_amd.xApy(X, A), np.int64), p)
    for k, xk in enumerate((p - 1, h)):
        want = [n * xk * (p - 1) % p, n * xk * h % p, n * xk * (p - h) % p] + [(n // 5) * xk * (p - 1) % p] * 5
        assert got[k].tolist() == want
    st = spasm_amd.xApy_stats()
    assert st["long_columns"] >= 3 and st["k"] == 2


@pytest.mark.parametrize("p", BIG)
def test_gesv_on_a_star(oracle, p):
    """X.A = B on the GPU's factorization of a star with values (p - 1)/2: B made of combinations of the rows of A with
    coefficients p - 1 and random ones; X.A == B checked exactly"""
    h = half(p)
    K, C, nred = 300, 4, 50
    n, m, ti, tj, tx, _ = star(p, K, C=C, nred=nred, x=h, u=h, a_seed=3)
    A = oracle.compress(p, n, m, ti, tj, tx)
    o = spasm_amd.default_opts()
    o.L = True
    F = spasm_amd.echelonize(_product(A), o)
    assert F.U.n == oracle.echelonize(A).U.n
    Ad = A.to_dense()
    rng = np.random.default_rng(p % 101)
    X0 = rng.integers(0, p, size=(6, n), dtype=np.int64)
    X0[0] = p - 1
    B = csr_of_dense(mulmod(X0, Ad, p), p, spasm_amd.Csr)
    X, ok = spasm_amd.gesv(F, B)
    assert ok[:B.n].all()
    Xd = np.zeros((B.n, n), np.int64)
    for i in range(B.n):
        lo, hi = int(X.p[i]), int(X.p[i + 1])
        Xd[i, X.j[lo:hi]] = np.mod(X.x[lo:hi].astype(np.int64), p)
    assert np.array_equal(mulmod(Xd, Ad, p), mulmod(X0, Ad, p))


# --------------------------------------------------------------------------
# 5. end to end on reference matrices at the new primes
# --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mat364.sms", "medium.sms", "trefethen_500.sms", "singular.sms", "rectangular_l.sms", "dm.sms",
                                  "BIOMD0000000424.int.mpl.sms", "cc.sms"])
@pytest.mark.parametrize("p", [44939, 46337, 65287, 65521, 698827, 2147483659])
def test_echelonize_and_rref_at_new_primes(oracle, name, p):
    A = oracle.load_sms(matrix_path(name), p)
    F = spasm_amd.echelonize(_product(A))
    assert F.U.n == oracle.echelonize(A).U.n
    R, Rq = spasm_amd.rref(F)
    R_want, Rq_want = oracle.rref(oracle.Fact(oracle.CSR(F.U.n, F.U.m, F.U.p, F.U.j, F.U.x, p), F.qinv))
    assert np.array_equal(Rq, Rq_want)
    assert oracle.same_matrix(oracle.CSR(R.n, R.m, R.p, R.j, R.x, p), R_want)
