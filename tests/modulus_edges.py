"""The moduli at which the kernels change their arithmetic, and inputs whose exact answers are known in closed form.

Every elimination kernel picks its number representation from the prime, and relies on a bound on how many terms it adds
before it reduces.  REGIMES lists each such switch: the file and the exact source expression that makes it, the same
predicate in Python, and the two primes on either side of it.  tests/test_modulus_edges_host.py checks that the table still
matches the sources; tests/test_gpu_modulus_edges.py runs the kernels on both sides of every line.

star() builds factors whose Schur complement is a long sum of equal terms: K pivot rows, each with a unit pivot and the same
entry u on every one of C shared non-pivotal columns, and rows to reduce that hold x on every pivot column.  Every entry of S
is then a_c - K x u mod p, a sum of K equal products; with x = u = 1 every term a kernel adds is p - 1, the largest residue.
(A plain helper module: no fixtures, no tests.)"""
import numpy as np

TWO32 = 1 << 32


def is_prime(n):
    """deterministic trial division (n < 2^32: at most 32,768 odd divisors)"""
    n = int(n)
    if n < 2:
        return False
    if n % 2 == 0:
        return n == 2
    d = 3
    while d * d <= n:
        if n % d == 0:
            return False
        d += 2
    return True


def _sgn_ok(p):
    """sgn_dev.h: signed 16-bit entries with deferred reduction, |entry| <= B = p/2 + p/64 + 1, 4 B^2 + B < 2^31"""
    B = p // 2 + p // 64 + 1
    return p >= 3 and B <= 32767 and 4 * B * B + B <= 0x7FFFFFFF


# (name, file under spasm_amd/csrc, exact source expression, predicate: True on the `below` side, (below, above))
REGIMES = [
    ("signed 16-bit entries, deferred reduction", "sgn_dev.h",
     "return prime >= 3 && B <= 32767 && 4 * B * B + B <= 0x7FFFFFFFll;", _sgn_ok, (44927, 44939)),
    ("back-substituted image: signed entries", "backsolve.hip",
     "B.sgn = B.plain && sgn_eligible(P.prime) && env_int(\"SPASM_HIP_BS_SIGNED\", 1) != 0;", _sgn_ok, (44927, 44939)),
    ("sparse image: 8-byte entries beyond the signed bound", "sparse_image.hip",
     "S.wide = !sgn_eligible(P.prime) || env_int(\"SPASM_HIP_SPARSE_IMAGE_WIDE\", 0) != 0;", _sgn_ok, (44927, 44939)),
    ("dense RREF: fast 64 x 64 try inversion", "dense_kernels.hip",
     "bool fast_try = small_prime && (4 * (prime / 2 + prime / 64 + 1) * (prime / 2 + prime / 64 + 1) + "
     "(prime / 2 + prime / 64 + 1) <= 0x7FFFFFFFll);", _sgn_ok, (44927, 44939)),
    ("dense RREF: 24-bit panel multiplies", "dense_kernels.hip",
     "const bool small_prime = prime < 46341;", lambda p: 2 * p * p < TWO32, (46337, 46349)),
    ("dense RREF: int8 digits on the matrix cores", "dense_kernels.hip",
     "const bool mfma_ok = use_mfma && prime <= 65279;", lambda p: p <= 65279, (65269, 65287)),
    ("blocked LU: int8 digits on the matrix cores", "dense_kernels.hip",
     "bool blocked = prime <= 65279 && ld % 4 == 0", lambda p: p <= 65279, (65269, 65287)),
    ("row-panel echelon extend: matrix cores only", "dense_kernels.hip",
     "if (prime > 65279)", lambda p: p <= 65279, (65269, 65287)),
    ("back-substituted image: packed 16-bit R, plain coefficients", "backsolve.hip",
     "B.plain = P.prime < 65536;", lambda p: p < 1 << 16, (65521, 65537)),
    ("dense RREF: SMALL16 paths", "dense_kernels.hip",
     "const bool small16 = prime < 65536;", lambda p: p < 1 << 16, (65521, 65537)),
    ("row-panel extend: Barrett quotient through __umul24", "dense_kernels.hip",
     "const bool q24 = F.p >= 256;", lambda p: p < 256, (251, 257)),
    ("row-by-row Schur: narrow LDS tables", "schur_api.hip",
     "wide_lds = ((double) F->prime * 6146.0 >= 4294967296.0);", lambda p: p * 6146 < TWO32, (698821, 698827)),
    ("row-by-row Schur: 6,144 + 1 terms per LDS slot", "schur_kernels.hip",
     "constexpr int CAPK = (H * 3) / 4 - 64;", lambda p: p * 6146 < TWO32, (698821, 698827)),
    ("x.A, solve: Montgomery products of any odd p < 2^32", "spmv.hip",
     "if (prime < 3 || prime > 0xfffffffbLL || (prime & 1) == 0)", lambda p: p < 1 << 31, (2147483647, 2147483659)),
]

# the narrow / wide dense accumulators depend on the factor as well: a column of the factor receives at most maxdeg + 1
# terms below 2p (maxdeg = the largest number of rows of U that hold one non-pivotal column)
MAXDEG_SOURCES = [
    ("schur_api.hip", "wide_dense = (2.0 * (double) F->prime * ((double) F->maxdeg + 3.0) >= 4294967296.0);"),
    ("dense_api.hip", "const bool wide = (2.0 * (double) F->prime * ((double) F->maxdeg + 3.0) >= 4294967296.0);"),
    ("schur_kernels.hip", "prod[q] = WIDE ? montmul(w_neg, val, F) : montmul_lazy(w_neg, val, F);"),
]


def narrow_dense(p, maxdeg):
    return 2 * p * (maxdeg + 3) < TWO32


# (p, K): a star of K pivot rows has maxdeg = K.  Pairs at one p straddle 2p(K + 3) = 2^32; the last ones are wide with
# K (p - 1) >= 2^32, so that a narrow 32-bit sum of the K terms would wrap and give a wrong residue.
MAXDEG_PAIRS = [(195225781, 8), (195225781, 9), (1000000007, 8), (2147483647, 3), (4294967291, 2)]

# the modulus edges as a whole: both sides of every switch, the smallest odd prime and the largest prime below 2^32
EDGE_PRIMES = sorted({q for r in REGIMES for q in r[4]} | {3, 4294967291})


def star(p, K, C=1, nred=4, x=1, u=1, a_seed=None):
    """A star factor: rows 0..K-1 are pivot rows (row k: 1 on column k, u on columns K..K+C-1), rows K..K+nred-1 are rows to
    reduce (x on every pivot column, a_i,c on the non-pivotal columns; a = 0 without a_seed, else random residues).
    Returns (n, m, ti, tj, tx, want): triplets with values in [0, p) and want = the nred x C dense Schur complement on the
    non-pivotal columns, from Python integers: S[i, c] = a_i,c - K x u mod p."""
    m = K + C
    piv = np.arange(K, dtype=np.int64)
    ti = [np.repeat(piv, 1 + C)]
    tj = [np.concatenate([piv[:, None], K + np.tile(np.arange(C, dtype=np.int64), (K, 1))], axis=1).ravel()]
    tx = [np.tile(np.array([1] + [u % p] * C, dtype=np.int64), K)]
    a = np.zeros((nred, C), dtype=np.int64)
    if a_seed is not None:
        a = np.random.default_rng(a_seed).integers(0, p, size=(nred, C), dtype=np.int64)
    for i in range(nred):
        cols = np.concatenate([piv, K + np.flatnonzero(a[i])])
        ti.append(np.full(len(cols), K + i, np.int64))
        tj.append(cols)
        tx.append(np.concatenate([np.full(K, x % p, np.int64), a[i][a[i] != 0]]))
    want = np.array([[(int(a[i, c]) - K * (x % p) * (u % p)) % p for c in range(C)] for i in range(nred)], dtype=np.int64)
    return (K + nred, m, np.concatenate(ti).astype(np.int32), np.concatenate(tj).astype(np.int32), np.concatenate(tx), want)


def star_factor(oracle, p, n, m, K, ti, tj, tx):
    """(A, F, rows) with oracle types: F is the star's own pivot rows (row k pivots on column k), rows the rows to reduce"""
    A = oracle.compress(p, n, m, ti, tj, tx)
    top = ti < K
    U = oracle.compress(p, K, m, ti[top], tj[top], tx[top])
    qinv = np.full(m, -1, np.int32)
    qinv[:K] = np.arange(K, dtype=np.int32)
    return A, oracle.Fact(U, qinv), np.arange(K, n, dtype=np.int32)


def dense_of_sparse_rows(S, K, C):
    """the non-pivotal columns K..K+C-1 of a Schur complement as an int64 array of residues"""
    out = np.zeros((S.n, C), np.int64)
    for i in range(S.n):
        lo, hi = int(S.p[i]), int(S.p[i + 1])
        out[i, np.asarray(S.j[lo:hi], np.int64) - K] = np.asarray(S.x[lo:hi], np.int64) % S.prime
    return out


def half(p):
    """(p - 1) / 2: the balanced representative of largest magnitude"""
    return (p - 1) // 2
