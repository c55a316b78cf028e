"""Dulmage-Mendelsohn decompositions without the reference: a checker, a canonical form, generators whose answer is known.

check_dm(A, dm, size) proves a result right on its own terms:
  - p and q are bijections, p[t] is matched to q[cc[1] + t] for t < rr[3] and every such pair is an entry of A;
  - the coarse blocks are upper triangular (the reference's tests/dm.c), and R1 u R2 u C3 is a vertex cover of size
    rr[2] + cc[4] - cc[3] == size: by Koenig's theorem the matching is maximum, so R0 and C0 (outside it) are unmatched rows
    and columns of a maximum matching;
  - the fine blocks (H, the blocks of S, V) are block upper triangular (tests/scc.c), every block of S is square with its
    matched pairs on the diagonal and strongly connected: the decomposition is the finest there is.
canonical(dm) keeps what is unique for a matrix: the sets R1, C0 u C1, R2, C2, R0 u R3, C3 and the set of fine blocks (C0 and C1
on their own are not unique, neither are R0 and R3, nor the order of the fine blocks).
"""
import hashlib

import numpy as np

try:
    import scipy.sparse as _sp
    import scipy.sparse.csgraph as _csgraph
except ImportError:       # pragma: no cover - the checker falls back to a plain search
    _sp = None


def _is_perm(v, k):
    v = np.asarray(v)
    return v.shape == (k,) and np.array_equal(np.sort(v), np.arange(k))


def _coo(A):
    rows = np.repeat(np.arange(A.n, dtype=np.int64), np.diff(np.asarray(A.p, np.int64)))
    return rows, np.asarray(A.j[:A.nnz] if hasattr(A, "nnz") else A.j, np.int64)


def _strongly_connected(k, src, dst):
    """is the digraph on 0 .. k-1 with arcs src -> dst strongly connected"""
    if k <= 1:
        return True
    if _sp is not None:
        G = _sp.csr_matrix((np.ones(len(src), np.int8), (src, dst)), shape=(k, k))
        return _csgraph.connected_components(G, directed=True, connection="strong")[0] == 1
    for a, b in ((src, dst), (dst, src)):
        adj = [[] for _ in range(k)]
        for u, v in zip(a.tolist(), b.tolist()):
            adj[u].append(v)
        seen, todo = {0}, [0]
        while todo:
            for v in adj[todo.pop()]:
                if v not in seen:
                    seen.add(v)
                    todo.append(v)
        if len(seen) != k:
            return False
    return True


def check_dm(A, dm, size):
    n, m = A.n, A.m
    p, q = np.asarray(dm.p), np.asarray(dm.q)
    rr, cc = [int(v) for v in dm.rr], [int(v) for v in dm.cc]
    assert _is_perm(p, n), "p is not a permutation"
    assert _is_perm(q, m), "q is not a permutation"
    assert rr[0] == 0 and rr[4] == n and cc[0] == 0 and cc[4] == m
    assert all(rr[t] <= rr[t + 1] for t in range(4)) and all(cc[t] <= cc[t + 1] for t in range(4))
    # the matching: R1 | R2 | R3 against C1 | C2 | C3
    assert rr[1] == cc[2] - cc[1] and rr[2] - rr[1] == cc[3] - cc[2] and rr[3] - rr[2] == cc[4] - cc[3]
    assert rr[3] == size == rr[2] + cc[4] - cc[3], (rr, cc, size)
    rows, cols = _coo(A)
    pinv = np.empty(n, np.int64)
    pinv[p] = np.arange(n)
    qinv = np.empty(m, np.int64)
    qinv[q] = np.arange(m)
    I, J = pinv[rows], qinv[cols]               # entries of A(p, q)
    keys = I * max(m, 1) + J
    pairs = np.arange(rr[3], dtype=np.int64)
    assert np.all(np.isin(pairs * max(m, 1) + cc[1] + pairs, keys)), "a matched pair is not an entry of A"
    # coarse blocks upper triangular (tests/dm.c), and Koenig: R1 u R2 u C3 covers every entry
    assert not np.any((I >= rr[1]) & (I < rr[2]) & (J < cc[2])), "a row of R2 has entries in C0 u C1"
    assert not np.any((I >= rr[2]) & (J < cc[3])), "a row of R3 u R0 has entries in C0, C1 or C2"
    # fine blocks
    nb = int(dm.nb)
    r, c = np.asarray(dm.r[:nb + 1], np.int64), np.asarray(dm.c[:nb + 1], np.int64)
    assert nb >= 2 and r[0] == 0 and c[0] == 0 and r[1] == rr[1] and c[1] == cc[2]
    assert r[nb - 1] == rr[2] and c[nb - 1] == cc[3] and r[nb] == n and c[nb] == m
    assert np.all(np.diff(r) >= 0) and np.all(np.diff(c) >= 0)
    assert np.array_equal(r[1:nb] - rr[1], c[1:nb] - cc[2]), "a block of S is not square"
    assert np.all(np.diff(r[1:nb]) > 0), "an empty block inside S"
    blk_of_row = np.searchsorted(r, I, side="right") - 1
    assert np.all(J >= c[blk_of_row]), "A(p, q) is not block upper triangular"
    inside = (blk_of_row >= 1) & (blk_of_row <= nb - 2) & (J < c[np.minimum(blk_of_row + 1, nb)])
    bi, bs, bd = blk_of_row[inside], I[inside] - rr[1], J[inside] - cc[2]
    order = np.argsort(bi, kind="stable")
    bi, bs, bd = bi[order], bs[order], bd[order]
    starts = np.searchsorted(bi, np.arange(1, nb - 1))
    ends = np.searchsorted(bi, np.arange(1, nb - 1), side="right")
    for k in range(1, nb - 1):
        lo, hi = starts[k - 1], ends[k - 1]
        if r[k + 1] - r[k] > 1:
            base = r[k] - rr[1]
            assert _strongly_connected(int(r[k + 1] - r[k]), bs[lo:hi] - base, bd[lo:hi] - base), "block %d is not strongly connected" % k


def fine_blocks(dm, n, m):
    """(rows, columns) of every fine block, H and V included; a reference result with an empty S (nb = 0) gets them from rr / cc"""
    p, q = np.asarray(dm.p), np.asarray(dm.q)
    rr, cc = [int(v) for v in dm.rr], [int(v) for v in dm.cc]
    if int(dm.nb) == 0:
        r, c = [0, rr[1], n], [0, cc[2], m]
    else:
        r, c = [int(v) for v in dm.r[:dm.nb + 1]], [int(v) for v in dm.c[:dm.nb + 1]]
    return [(p[r[k]:r[k + 1]], q[c[k]:c[k + 1]]) for k in range(len(r) - 1)]


def canonical(dm, n, m):
    """a dict of int32 arrays: the six coarse sets, and the fine blocks (each sorted inside, the blocks sorted) as two
    concatenated lists with their pointers"""
    p, q = np.asarray(dm.p), np.asarray(dm.q)
    rr, cc = [int(v) for v in dm.rr], [int(v) for v in dm.cc]
    out = {
        "R1": np.sort(p[:rr[1]]), "C01": np.sort(q[:cc[2]]), "R2": np.sort(p[rr[1]:rr[2]]),
        "C2": np.sort(q[cc[2]:cc[3]]), "R03": np.sort(p[rr[2]:]), "C3": np.sort(q[cc[3]:]),
    }
    blocks = [(np.sort(a), np.sort(b)) for a, b in fine_blocks(dm, n, m) if len(a) or len(b)]
    blocks.sort(key=lambda rc: (int(rc[0][0]) if len(rc[0]) else -1, int(rc[1][0]) if len(rc[1]) else -1))
    out["fine_rows"] = np.concatenate([a for a, _ in blocks] + [np.zeros(0, np.int64)]).astype(np.int32)
    out["fine_cols"] = np.concatenate([b for _, b in blocks] + [np.zeros(0, np.int64)]).astype(np.int32)
    out["fine_rows_ptr"] = np.cumsum([0] + [len(a) for a, _ in blocks]).astype(np.int32)
    out["fine_cols_ptr"] = np.cumsum([0] + [len(b) for _, b in blocks]).astype(np.int32)
    return {k: np.asarray(v, np.int32) for k, v in out.items()}


CANONICAL_KEYS = ("R1", "C01", "R2", "C2", "R03", "C3", "fine_rows", "fine_cols", "fine_rows_ptr", "fine_cols_ptr")


def digest(canon):
    h = hashlib.sha256()
    for k in CANONICAL_KEYS:
        h.update(k.encode())
        h.update(np.ascontiguousarray(canon[k], np.int32).tobytes())
    return h.hexdigest()


def same_canonical(a, b):
    return all(np.array_equal(a[k], b[k]) for k in CANONICAL_KEYS)


def permuted_pattern(A, p, q, cls, prime):
    """A(p, q) (row i is row p[i] of A, column j is column q[j]) as cls(n, m, p, j, x, prime), columns sorted in each row"""
    rows, cols = _coo(A)
    pinv = np.empty(A.n, np.int64)
    pinv[p] = np.arange(A.n)
    qinv = np.empty(A.m, np.int64)
    qinv[q] = np.arange(A.m)
    return csr_of(cls, A.n, A.m, pinv[rows], qinv[cols], prime)


def csr_of(cls, n, m, rows, cols, prime):
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    key = np.unique(rows * max(m, 1) + cols)
    rows, cols = key // max(m, 1), key % max(m, 1)
    ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=ptr[1:])
    return cls(n, m, ptr, cols.astype(np.int32), np.ones(len(cols), np.int32), prime)


def transpose_of(A, cls):
    rows, cols = _coo(A)
    return csr_of(cls, A.m, A.n, cols, rows, A.prime)


# ---- generators with a known answer ----
class Known:
    """a generated matrix and its canonical sets: rows / columns of H, S (its blocks) and V, the matching size"""

    def __init__(self, A, H, blocks, V, size):
        self.A, self.H, self.blocks, self.V, self.size = A, H, blocks, V, size

    def canonical(self):
        return canonical(_Fake(self.A.n, self.A.m, self.H, self.blocks, self.V), self.A.n, self.A.m)


class _Fake:
    """a DM laid out from known sets (for canonical())"""

    def __init__(self, n, m, H, blocks, V):
        (hr, hc), (vr, vc) = H, V
        parts_r = [hr] + [a for a, _ in blocks] + [vr]
        parts_c = [hc] + [b for _, b in blocks] + [vc]
        self.p = np.concatenate(parts_r).astype(np.int32)
        self.q = np.concatenate(parts_c).astype(np.int32)
        self.r = np.cumsum([0] + [len(a) for a in parts_r]).astype(np.int32)
        self.c = np.cumsum([0] + [len(b) for b in parts_c]).astype(np.int32)
        self.nb = len(parts_r)
        s = sum(len(a) for a, _ in blocks)
        self.rr = [0, len(hr), len(hr) + s, n, n]          # only rr[1], rr[2] and cc[2], cc[3] matter to canonical()
        self.cc = [0, 0, len(hc), len(hc) + s, m]


def generate(cls, prime, h_rows, s_sizes, v_cols, extra=2, seed=0):
    """H: h_rows rows with two private columns each (one of them always free); S: square blocks, each a diagonal plus a cycle
    (strongly connected), random entries only towards later blocks and V; V: v_cols columns with two private rows each.  H
    rows also get random entries anywhere.  Random row and column permutations on top."""
    rng = np.random.default_rng(seed)
    s_total = int(sum(s_sizes))
    n = h_rows + s_total + 2 * v_cols
    m = 2 * h_rows + s_total + v_cols
    R, Cc = [], []
    # H: rows 0 .. h_rows-1, columns 0 .. 2 h_rows - 1
    h = np.arange(h_rows)
    R += [h, h]
    Cc += [2 * h, 2 * h + 1]
    if h_rows:
        hx = np.repeat(h, extra)
        R.append(hx)
        Cc.append(rng.integers(0, m, len(hx)))
    # S: rows / columns from h_rows / 2 h_rows on
    starts = np.cumsum([0] + list(s_sizes))
    s_row0, s_col0, v_col0 = h_rows, 2 * h_rows, 2 * h_rows + s_total
    if s_total:
        sizes = np.asarray(s_sizes, np.int64)
        blk = np.repeat(np.arange(len(sizes)), sizes)
        t = np.arange(s_total)
        nxt = np.where(t + 1 < starts[blk + 1], t + 1, starts[blk])      # the cycle inside the block
        R += [s_row0 + t, s_row0 + t]
        Cc += [s_col0 + t, s_col0 + nxt]
        tx = np.repeat(t, extra)
        later = starts[blk[tx] + 1]                                     # first column after the block (in S, or V beyond)
        span = (s_total + v_cols) - later
        ok = span > 0
        tgt = later[ok] + (rng.random(ok.sum()) * span[ok]).astype(np.int64)
        R.append(s_row0 + tx[ok])
        Cc.append(s_col0 + tgt)
    # V: columns v_col0 .. m-1, rows from h_rows + s_total on, two private rows per column
    v = np.arange(v_cols)
    v_row0 = h_rows + s_total
    R += [v_row0 + 2 * v, v_row0 + 2 * v + 1]
    Cc += [v_col0 + v, v_col0 + v]
    if v_cols:
        vx = np.repeat(np.arange(2 * v_cols), extra)
        R.append(v_row0 + vx)
        Cc.append(v_col0 + rng.integers(0, v_cols, len(vx)))
    rows = np.concatenate(R + [np.zeros(0, np.int64)]).astype(np.int64)
    cols = np.concatenate(Cc + [np.zeros(0, np.int64)]).astype(np.int64)
    # random relabelling: new row prow[i] for old row i
    prow, pcol = rng.permutation(n), rng.permutation(m)
    A = csr_of(cls, n, m, prow[rows], pcol[cols], prime)
    H = (prow[:h_rows], pcol[:2 * h_rows])
    blocks = [(prow[s_row0 + starts[k]:s_row0 + starts[k + 1]], pcol[s_col0 + starts[k]:s_col0 + starts[k + 1]])
              for k in range(len(s_sizes))]
    V = (prow[v_row0:], pcol[v_col0:])
    return Known(A, H, blocks, V, h_rows + s_total + v_cols)


def chain(cls, prime, n):
    """an upper-bidiagonal n x n chain, columns reversed, that defeats a greedy matching taking the smallest free column:
    row i has columns n-1-i and n-2-i.  Greedy leaves row n-1 and column n-1 free; the one augmenting path has length n.
    Its decomposition: S is everything, n blocks of size 1."""
    i = np.arange(n)
    rows = np.concatenate([i, i[:-1]])
    cols = np.concatenate([n - 1 - i, n - 2 - i[:-1]])
    A = csr_of(cls, n, n, rows, cols, prime)
    blocks = [(np.array([k]), np.array([n - 1 - k])) for k in range(n)] if n <= 2000 else None
    return Known(A, (np.zeros(0, np.int64), np.zeros(0, np.int64)), blocks, (np.zeros(0, np.int64), np.zeros(0, np.int64)), n)
