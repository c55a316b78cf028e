"""Stable transposition and kernel bases without the reference: the numpy model of the order, matrices built to reach every
route of spasm_amd/csrc/transpose.hip, factors (U, qinv) built by hand, and an exact-integer model of the kernel basis.

model_transpose(A) is spasm_transpose (spasm_transpose.c:5) as one stable argsort; tests/test_kernel_cases_host.py holds it
against the host spasm_amd.transpose.  TRANSPOSE_CASES are the shapes of tests/test_gpu_transpose.py, each with the switches it
runs under and the routes it claims to reach (the columns of the short and of the long route, the row chunks of the long
route).  FACTOR_CASES are the factors of tests/test_gpu_kernel_basis.py; model_kernel(F) is the kernel basis of F.U from a dense
reduced row echelon form in exact integers.  No GPU is needed here.
"""
import numpy as np

import spasm_amd

# the constants of transpose.hip the shapes are built around (test_kernel_cases_host.py checks they are still there)
TR_SHORT, TR_CHUNK = 256, 262144
SOURCE_EXPRESSIONS = ["TR_SHORT_DEFAULT = %d;" % TR_SHORT, "TR_CHUNK_MAX = %d;" % TR_CHUNK]      # the two numeric defaults
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
GOLDEN_FOR_TRANSPOSE = ["rectangular_l.sms", "rectangular_h.sms", "trefethen_500.sms", "mat364.sms"]


# ---- transposition ----
def model_transpose(A, keep_values=True):
    """(p, j, x) of A^T in the stable order: entries of a row by increasing row of A.  x is None without values."""
    nnz = A.nnz
    rows = np.repeat(np.arange(A.n, dtype=np.int32), np.diff(A.p))
    j = np.asarray(A.j[:nnz], np.int64)
    order = np.argsort(j, kind="stable")
    p = np.zeros(A.m + 1, np.int64)
    p[1:] = np.cumsum(np.bincount(j, minlength=A.m)[:A.m]) if A.m else 0
    x = A.x[:nnz][order] if keep_values and A.x is not None else None
    return p, rows[order], x


def from_columns(n, m, columns, seed=0, values=None, prime=42013):
    """the n x m Csr whose column c holds the rows columns[c]; the entries of a row in a shuffled order (a CSR row need not be
    sorted), values from `values` (cycled) or pseudo-random int32"""
    rng = np.random.default_rng(seed)
    ti = np.concatenate([np.asarray(r, np.int64) for r in columns] + [np.zeros(0, np.int64)])
    tj = np.concatenate([np.full(len(r), c, np.int64) for c, r in enumerate(columns)] + [np.zeros(0, np.int64)])
    assert len(set(zip(ti.tolist(), tj.tolist()))) == len(ti), "a repeated (i, j)"
    assert not len(ti) or (ti.min() >= 0 and ti.max() < n and tj.max() < m)
    shuffle = rng.permutation(len(ti))
    ti, tj = ti[shuffle], tj[shuffle]
    order = np.argsort(ti, kind="stable")
    ti, tj = ti[order], tj[order]
    if values is None:
        tx = rng.integers(INT32_MIN, INT32_MAX, len(ti), dtype=np.int64, endpoint=True)
    else:
        tx = np.resize(np.asarray(values, np.int64), len(ti))
    p = np.zeros(n + 1, np.int64)
    p[1:] = np.cumsum(np.bincount(ti, minlength=n)[:n]) if n else 0
    return spasm_amd.Csr(n, m, p, tj.astype(np.int32), tx.astype(np.int32), prime)


def _pick(rng, n, k, must=()):
    """k distinct rows of [0, n) that include `must`"""
    rest = np.setdiff1d(np.arange(n), np.asarray(must, np.int64))
    return np.sort(np.concatenate([np.asarray(must, np.int64), rng.choice(rest, k - len(must), replace=False)]))


def transpose_cases():
    """[(name, A, env, routes)]: env the switches of the case, routes = (short columns, long columns, row chunks) it must report"""
    rng = np.random.default_rng(20240611)
    out = []

    def add(name, A, env=None, short_max=TR_SHORT, chunk=TR_CHUNK):
        env = dict(env or {})
        lens = np.diff(model_transpose(A)[0])
        nlong = int(np.sum(lens > short_max))
        routes = (int(np.sum((lens > 0) & (lens <= short_max))), nlong, -(-A.n // chunk) if nlong else 0)
        out.append((name, A, env, routes))

    add("0x0", from_columns(0, 0, []))
    add("0x5", from_columns(0, 5, [[]] * 5))
    add("5x0", from_columns(5, 0, []))
    add("empty_rows", from_columns(5, 7, [[]] * 7))
    add("1x1", from_columns(1, 1, [[0]]))
    for n in (1, 63, 64, 65, 4097):
        add("one_column_%d_rows" % n, from_columns(n, 1, [np.arange(n)], seed=n))
    add("one_row_4097_columns", from_columns(1, 4097, [[0]] * 4097))
    # the threshold between the routes: a column of exactly L - 1, L and L + 1 entries
    L = TR_SHORT
    add("threshold_default", from_columns(300, 3, [_pick(rng, 300, L - 1), _pick(rng, 300, L), _pick(rng, 300, L + 1)], seed=1))
    add("threshold_4", from_columns(9, 3, [_pick(rng, 9, 3), _pick(rng, 9, 4), _pick(rng, 9, 5)], seed=2),
        {"SPASM_HIP_TRANSPOSE_SHORT": "4"}, short_max=4)
    # long columns over 1, 2 and 3 bitmap chunks of c rows; entries on both sides of every chunk boundary
    c = 128
    sw = {"SPASM_HIP_TRANSPOSE_SHORT": "3", "SPASM_HIP_TRANSPOSE_CHUNK": str(c)}
    add("chunks_1", from_columns(c, 2, [_pick(rng, c, 9, [0, c - 1]), _pick(rng, c, 2)], seed=3), sw, 3, c)
    add("chunks_2", from_columns(2 * c, 2, [_pick(rng, 2 * c, 9, [c - 1, c, 2 * c - 1]), [c - 1, c, 2 * c - 1, 0]], seed=4), sw, 3, c)
    add("chunks_3", from_columns(2 * c + 1, 4, [_pick(rng, c, 6, [0, c - 1]),                   # inside the first chunk
                                                 _pick(rng, 2 * c, 7, [c - 1, c, 2 * c - 1]),    # over two
                                                 [c - 1, c, 2 * c - 1, 2 * c],                   # first and last entry on boundaries
                                                 _pick(rng, 2 * c + 1, 40, [c - 1, c, 2 * c - 1, 2 * c])], seed=5), sw, 3, c)
    # every row, alternating rows, only the last row -- under the default switches and chunk by chunk
    n = 1000
    cols = [np.arange(n), np.arange(0, n, 2), [n - 1]]
    add("full_alternating_last", from_columns(n, 3, cols, seed=6))
    add("full_alternating_last_chunked", from_columns(n, 3, cols, seed=7), {"SPASM_HIP_TRANSPOSE_CHUNK": "128"}, TR_SHORT, 128)
    # values are carried as the 32-bit words they are
    edge = [INT32_MIN, INT32_MAX, 0, -1]
    add("edge_values_short", from_columns(6, 5, [_pick(rng, 6, k) for k in (4, 1, 6, 2, 3)], seed=8, values=edge))
    add("edge_values_long", from_columns(600, 2, [_pick(rng, 600, 400), _pick(rng, 600, 7)], seed=9, values=edge))
    # a random sparse matrix: several workgroups of short columns, shuffled rows
    add("random_sparse", from_columns(700, 900, [_pick(rng, 700, int(k)) for k in rng.integers(0, 12, 900)], seed=10))
    return out


def _mulmod(a, b, p):
    """a * b mod p entry by entry, exact: int64 where the product fits, Python integers (object arrays) otherwise"""
    if (p - 1) * (p - 1) < 2 ** 63:
        return a * b % p
    return np.asarray(a.astype(object) * b.astype(object) % p, object).astype(np.int64)


# ---- the column-major image through its other users (tests/test_gpu_colmajor.py) ----
COLMAJOR_MODULI = [42013, 4294967291]
XA_LONG = 32             # spmv.hip: a column with more entries goes to the long list of x.A


def with_prime(A, p):
    """the same arrays as a matrix mod p"""
    return spasm_amd.Csr(A.n, A.m, A.p, A.j, A.x, p)


def model_xApy(X, A, Y0):
    """Y0 + X.A mod A.prime as residues in [0, p), exact, entry by entry: every product is reduced before it is added, and a
    column adds up fewer than 2^31 terms below 2^32"""
    p = A.prime
    rows = np.repeat(np.arange(A.n), np.diff(A.p))
    vals = np.asarray(A.x[:A.nnz], np.int64) % p
    prod = _mulmod(np.asarray(X, np.int64)[:, rows] % p, vals[None, :], p)
    out = (np.asarray(Y0, np.int64) % p).T.copy()
    np.add.at(out, A.j[:A.nnz], prod.T)
    return (out % p).T


def xa_inputs(A, k, seed):
    """seeded X (k x n) and Y0 (k x m) of residues"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, A.prime, (k, A.n), dtype=np.int64), rng.integers(0, A.prime, (k, A.m), dtype=np.int64)


# ---- kernel bases ----


def dense(A, p):
    """the matrix as an int64 array of residues in [0, p); repeated entries add up"""
    M = np.zeros((A.n, A.m), np.int64)
    rows = np.repeat(np.arange(A.n), np.diff(A.p))
    np.add.at(M, (rows, A.j[:A.nnz]), np.asarray(A.x[:A.nnz], np.int64) % p)
    return M % p


def matmul_mod(A, B, p):
    """A . B mod p for int64 arrays of residues, exact"""
    out = np.zeros((A.shape[0], B.shape[1]), np.int64)
    for k in range(A.shape[1]):
        out = (out + _mulmod(A[:, k:k + 1], B[k:k + 1, :], p)) % p
    return out


def rref(M, p):
    """(R, pivot columns) of the reduced row echelon form of M mod p (zero rows dropped), exact"""
    M = M.copy() % p
    pivots, r = [], 0
    for c in range(M.shape[1]):
        nz = np.flatnonzero(M[r:, c]) if r < M.shape[0] else []
        if len(nz) == 0:
            continue
        M[[r, r + nz[0]]] = M[[r + nz[0], r]]
        inv = pow(int(M[r, c]), -1, p)
        M[r] = _mulmod(M[r], np.full(M.shape[1], inv, np.int64), p)
        f = M[:, c:c + 1].copy()
        f[r] = 0
        M = (M - _mulmod(f, M[r:r + 1, :], p)) % p
        pivots.append(c)
        r += 1
    return M[:r], pivots


def balanced(M, p):
    M = np.asarray(M, np.int64) % p
    return np.where(M > p // 2, M - p, M)


def model_kernel(F):
    """the kernel basis of F.U as a dense int64 array of balanced residues: row k for the k-th non-pivotal column j is
    -e_j + sum_i R[i][j] e_pivot(i), R the reduced row echelon form -- what spasm_kernel returns, as a dense matrix"""
    p, m, r = F.U.prime, F.U.m, F.U.n
    # the pivots are the factor's (the first entry of each row), not the leftmost ones: reduce with those columns in front
    piv = [int(F.U.j[F.U.p[i]]) for i in range(r)]
    nonpiv = [j for j in range(m) if j not in set(piv)]
    R, lead = rref(dense(F.U, p)[:, piv + nonpiv], p)
    assert lead == list(range(r)), "the pivot columns of U do not carry a unit triangular block"
    K = np.zeros((len(nonpiv), m), np.int64)
    for k, j in enumerate(nonpiv):
        K[k, j] = p - 1
        K[k, piv] = R[:, r + k]
    return balanced(K, p)


def build_factor(r, m, p, seed, shuffle=False, fill=0.5, coupling=3, dense_column=None):
    """Fact(U, qinv): r rows on m columns mod p, each row a unit pivot then its other entries; a row may hold entries on the
    pivot columns of later rows only (so the rows can be eliminated in order), and on the non-pivotal columns with probability
    `fill` -- or, with dense_column = k, on the k-th non-pivotal column in every row and on no other.  shuffle: the pivot columns
    in a random order over the rows (rows of U not in pivot-column order)."""
    rng = np.random.default_rng(seed)
    cols = rng.permutation(m) if shuffle else np.arange(m)
    piv = cols[:r] if shuffle else np.sort(rng.choice(m, r, replace=False))
    if shuffle:
        piv = rng.permutation(piv)
    nonpiv = np.setdiff1d(np.arange(m), piv)
    Up, Uj, Ux = [0], [], []
    lo, hi = p // 2 - p + 1, p // 2

    def value():
        v = 0
        while v == 0:
            v = int(rng.integers(lo, hi, endpoint=True))
        return v

    for i in range(r):
        Uj.append(int(piv[i]))
        Ux.append(1)
        later = piv[i + 1:]
        pick = rng.choice(later, min(coupling, len(later)), replace=False) if len(later) else []
        if dense_column is not None:
            free = [nonpiv[dense_column]]
        else:
            free = nonpiv[rng.random(len(nonpiv)) < fill]
        for c in rng.permutation(np.concatenate([np.asarray(pick, np.int64), np.asarray(free, np.int64)])):
            Uj.append(int(c))
            Ux.append(value())
        Up.append(len(Uj))
    qinv = np.full(m, -1, np.int32)
    qinv[piv] = np.arange(r)
    U = spasm_amd.Csr(r, m, np.array(Up, np.int64), np.array(Uj, np.int32), np.array(Ux, np.int32), p)
    return spasm_amd.Fact(U, qinv)


BIG, TINY = 4294967291, 3


def factor_cases():
    """[(name, F, env, wants a pool retry)]"""
    out = [
        ("m_0", build_factor(0, 0, 42013, 14), {}, False),
        ("rank_0", build_factor(0, 7, 42013, 1), {}, False),
        ("rank_0_p3", build_factor(0, 5, TINY, 2), {}, False),
        ("full_column_rank", build_factor(9, 9, 42013, 3), {}, False),
        ("corank_1_r1", build_factor(1, 2, 42013, 4, fill=1.0), {}, False),
        ("corank_1_r64", build_factor(64, 65, 257, 5), {}, False),
        ("corank_1_r65_big", build_factor(65, 66, BIG, 6), {}, False),
        ("corank_1_r300", build_factor(300, 301, 42013, 7), {}, False),
        ("shuffled_rows", build_factor(40, 55, 42013, 8, shuffle=True), {}, False),
        ("shuffled_rows_p3", build_factor(40, 55, TINY, 9, shuffle=True), {}, False),
        ("shuffled_rows_big", build_factor(40, 55, BIG, 10, shuffle=True), {}, False),
        ("one_dense_column", build_factor(70, 75, 42013, 11, dense_column=2), {}, False),
        ("pivots_only", build_factor(12, 20, 42013, 12, fill=0.0, coupling=0), {}, False),
        ("pool_retry", build_factor(200, 260, 42013, 13, fill=0.6), {"SPASM_HIP_KERNEL_POOL": "2048"}, True),
    ]
    return out
