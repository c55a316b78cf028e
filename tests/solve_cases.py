"""X.A = B without the reference: an exact model of its two loops, factorizations built to a level structure, and the plan
the solver must make of them.

model_gesv(U, qinv, L, Lp, B, p) is spasm_gesv (spasm_solve.c:52, spasm_triangular.c:21-87) written plainly and vectorised over
the right-hand sides; tests/test_solve_cases_host.py holds it against every stored result of the compiled reference.
layered() builds U and L whose forward and back sweeps have the level widths and dependency counts a test asks for, with
the things the reference tolerates (rows of U out of order, rows of L without a pivot, entries right of the diagonal,
repeated entries) as options.  planned() recomputes what finish_sweep (spasm_amd/csrc/solve.hip) decides: levels, launches,
which launches step through a run of thin levels and which share their lists over a workgroup.  CASES are the shapes of
tests/test_gpu_solve_shapes.py with what each claims to reach.  No GPU is needed here.
"""
import numpy as np

import spasm_amd
from test_solve_host import balanced, dense, mulmod

# the constants of solve.hip the shapes are built around (test_solve_cases_host.py checks they are still there)
SV_WAVES, SV_TAIL_WAVES, SV_THIN, SV_RUN, SV_SPLIT = 4, 16, 16, 2, 64
SCAN_CHUNK = 1024
SOURCE_EXPRESSIONS = [
    "constexpr int SV_WAVES = 4;", "constexpr int SV_TAIL_WAVES = 16;", "constexpr int SV_THIN = 16;", "constexpr int SV_RUN = 2;",
    "constexpr int SV_SPLIT = 64;",
    "S.lptr[e + 1] - S.lptr[e] <= SV_THIN", "if (e - l < SV_RUN)", "deps >= SV_SPLIT * nodes",
    "launch_pointer_scan(d_len, kb, d_Xp, stream);",
    "std::max(1, std::min(256, S->r / 512))", "std::max(1, std::min(512, (nc + 7) / 8))",
    "for (; d + 4 <= e; d += 4)", "n * w / SV_TAIL_WAVES", "n * (w + 1) / SV_TAIL_WAVES",
    "(s < v || s >= F.p)", "env_int(\"SPASM_HIP_SOLVE_BATCH\", 0)",
]
# ... and of the scan of the row lengths, which the emit path shares with the column-major images (colmajor.hip)
SCAN_EXPRESSIONS = ["for (int base = 0; base < n; base += 1024)", "__shared__ int64_t s[1024];"]
SMALL_PRIMES = [3, 42013, 65537, 4294967291]


def emit_chunks(r):
    return max(1, min(256, r // 512))


def check_waves(nc):
    return max(1, min(512, (nc + 7) // 8))


# ---- the model ----
def _mul(c, v, p):
    """c * v mod p, exact in int64: c, v arrays (or c an int) with entries in [0, p), p < 2^32; v split in 16-bit halves
    where the plain product could pass 2^63"""
    if (p - 1) * (p - 1) < 2 ** 63:
        return c * v % p
    return (c * (v & 0xFFFF) + ((c * (v >> 16)) % p << 16)) % p


def _rows_with_a_repeated_column(M):
    rows = np.repeat(np.arange(M.n, dtype=np.int64), np.diff(np.asarray(M.p, np.int64)))
    key = np.sort(rows * max(M.m, 1) + np.asarray(M.j, np.int64)[:len(rows)])
    out = np.zeros(M.n, bool)
    out[key[1:][key[1:] == key[:-1]] // max(M.m, 1)] = True
    return out


def _subtract_row(b, cols, vals, x, p, repeated):
    """b[c] -= x * v for every entry (c, v) of a row; x and the lines of b run over the right-hand sides"""
    if repeated:
        for c, v in zip(cols.tolist(), vals.tolist()):
            b[c] = (b[c] - _mul(v, x, p)) % p
    else:
        b[cols] = (b[cols] - _mul(vals[:, None], x[None, :], p)) % p


def model_gesv(U, qinv, L, Lp, B, p):
    """(X, ok) of spasm_gesv on Fact(U, qinv, L, Lp) and the rows of B, in exact integer arithmetic"""
    p = int(p)
    k, m, r, n = B.n, U.m, U.n, L.n
    Up, Uj, Ux = np.asarray(U.p, np.int64), np.asarray(U.j, np.int64), np.asarray(U.x, np.int64) % p
    Lq, Lj, Lx = np.asarray(L.p, np.int64), np.asarray(L.j, np.int64), np.asarray(L.x, np.int64) % p
    qinv = np.asarray(qinv, np.int64)
    q = np.zeros(r, np.int64)
    q[qinv[qinv >= 0]] = np.flatnonzero(qinv >= 0)
    # spasm_scatter of each row of B: repeated columns add up
    b = np.zeros((m, k), np.int64)
    nzb = int(B.p[k])
    np.add.at(b, (np.asarray(B.j, np.int64)[:nzb], np.repeat(np.arange(k), np.diff(np.asarray(B.p, np.int64)))),
              np.asarray(B.x, np.int64)[:nzb] % p)
    b %= p
    # spasm_dense_forward_solve: the rows of U in order
    z = np.zeros((r, k), np.int64)
    rep = _rows_with_a_repeated_column(U)
    for i in range(r):
        zi = b[q[i]].copy()
        if not zi.any():
            continue
        z[i] = zi
        _subtract_row(b, Uj[Up[i]:Up[i + 1]], Ux[Up[i]:Up[i + 1]], zi, p, rep[i])
    ok = ~b.any(axis=0)
    # spasm_dense_back_solve: the pivots of L from the last one
    x = np.zeros((n, k), np.int64)
    rep = _rows_with_a_repeated_column(L)
    for j in range(r - 1, -1, -1):
        i = int(Lp[j])
        cols, vals = Lj[Lq[i]:Lq[i + 1]], Lx[Lq[i]:Lq[i + 1]]
        at = np.flatnonzero(cols == j)
        assert len(at) and vals[at[0]] != 0, "row Lp[%d] = %d of L has no diagonal" % (j, i)
        if not z[j].any():
            continue
        xi = _mul(pow(int(vals[at[0]]), -1, p), z[j], p)
        _subtract_row(z, cols, vals, xi, p, rep[i])
        x[i] = xi
    xt = np.ascontiguousarray(x.T)
    rows, cols = np.nonzero(xt)
    ptr = np.zeros(k + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=k), out=ptr[1:])
    return spasm_amd.Csr(k, n, ptr, cols.astype(np.int32), balanced(xt[rows, cols], p), p), ok


# ---- generators ----
def _distinct(rng, npop, c, rows):
    """rows x c draws from range(npop), distinct within a row"""
    if c == 0 or rows == 0:
        return np.zeros((rows, c), np.int64)
    assert c <= npop
    if c * 4 >= npop or rows < 32:
        return np.stack([rng.permutation(npop)[:c] for _ in range(rows)]).astype(np.int64)
    out = rng.integers(0, npop, size=(rows, c), dtype=np.int64)
    while True:
        s = np.sort(out, axis=1)
        bad = np.flatnonzero((s[:, 1:] == s[:, :-1]).any(axis=1))
        if len(bad) == 0:
            return out
        out[bad] = rng.integers(0, npop, size=(len(bad), c), dtype=np.int64)


def _structure(rng, widths, deps):
    """unknowns in solve order 0 .. r-1 with the given level widths and dependency counts (an int or one count per unknown
    for each level; level 0 has none): (t, i) pairs "t depends on i", i before t.  The first dependency of an unknown of
    level l lies in level l-1 (that pins its level), the others anywhere before; the solve order is a random topological one."""
    assert len(widths) == len(deps) and np.all(np.asarray(deps[0]) == 0)
    starts = np.concatenate([[0], np.cumsum(widths)]).astype(np.int64)
    r = int(starts[-1])
    key = np.zeros(r)
    key[:widths[0]] = rng.random(widths[0])
    T, I = [], []
    for l in range(1, len(widths)):
        w, lo = widths[l], int(starts[l])
        cnt = np.broadcast_to(np.asarray(deps[l], np.int64), (w,))
        assert cnt.min() >= 1 and cnt.max() <= lo, "level %d: between 1 and %d dependencies" % (l, lo)
        first = rng.integers(int(starts[l - 1]), lo, size=w, dtype=np.int64)
        t, i = [np.arange(lo, lo + w)], [first]
        for c in np.unique(cnt):
            who = np.flatnonzero(cnt == c)
            rest = _distinct(rng, lo - 1, int(c) - 1, len(who))
            rest += rest >= first[who, None]                    # (anything before but `first`)
            t.append(np.repeat(lo + who, int(c) - 1))
            i.append(rest.ravel())
        t, i = np.concatenate(t), np.concatenate(i)
        top = np.zeros(w)
        np.maximum.at(top, t - lo, key[i])
        key[lo:lo + w] = top + 1e-6 + rng.random(w)
        T.append(t)
        I.append(i)
    pos = np.empty(r, np.int64)
    pos[np.argsort(key, kind="stable")] = np.arange(r)
    if not T:
        return r, np.zeros(0, np.int64), np.zeros(0, np.int64)
    return r, pos[np.concatenate(T)], pos[np.concatenate(I)]


def _values(rng, p, count):
    return rng.integers(1, p, size=count, dtype=np.int64)


def _csr(n, m, rows, cols, vals, order, p):
    """entries sorted by (row, order)"""
    at = np.lexsort((order, rows))
    ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=ptr[1:])
    return spasm_amd.Csr(n, m, ptr, cols[at].astype(np.int32), balanced(vals[at], p), p)


def upper(rng, p, widths, deps, ncheck=0, check_used=1.0, check_per_row=2, row_order=None):
    """U (r x (r + ncheck), unit pivots first in their rows) and qinv: "z_t depends on z_i" is an entry U[i, q_t], i < t.
    The pivot columns are a random injection; the first check_used of the ncheck other columns carry check_per_row entries
    per row.  row_order "reversed" / "half": all rows / a random half of them in reverse order, so that earlier pivot
    columns are touched by later rows."""
    r, t, i = _structure(rng, widths, deps)
    m = r + ncheck
    perm = rng.permutation(m).astype(np.int64)
    q, free = perm[:r], perm[r:]
    used = free[:int(np.ceil(ncheck * check_used))]
    pick = _distinct(rng, len(used), min(check_per_row, len(used)), r)
    rows = np.concatenate([np.arange(r), i, np.repeat(np.arange(r), pick.shape[1])])
    cols = np.concatenate([q, q[t], used[pick].ravel() if pick.size else np.zeros(0, np.int64)])
    vals = np.concatenate([np.ones(r, np.int64), _values(rng, p, len(rows) - r)])
    order = np.concatenate([np.full(r, -1.0), rng.random(len(rows) - r)])
    new = np.arange(r)
    if row_order == "reversed":
        new = r - 1 - new
    elif row_order == "half":
        some = np.sort(rng.permutation(r)[:r // 2])
        new[some] = some[::-1]
    else:
        assert row_order is None
    qinv = np.full(m, -1, np.int32)
    qinv[q] = new
    return _csr(r, m, new[rows], cols, vals, order, p), qinv


def lower(rng, p, widths, deps, extra_rows=0, nonpivot=False, above=False, repeat=False):
    """L ((r + extra_rows) x r) and Lp (a random injection): the unknown solved s-th is y_j, j = r-1-s, "y_j depends on y_j'"
    is an entry L[Lp[j'], j], j' > j; random non-zero diagonals anywhere in their rows.  nonpivot: the rows outside Lp hold
    entries; above: entries of rows Lp[j] in columns > j; repeat: some (row, column) below the diagonal twice, and a second
    entry on one diagonal (the reference takes the first)."""
    r, t, i = _structure(rng, widths, deps)
    n = r + extra_rows
    Lp = rng.permutation(n)[:r].astype(np.int64)
    jt, ji = r - 1 - t, r - 1 - i
    rows, cols = [Lp, Lp[ji]], [np.arange(r), jt]
    order = [rng.random(r), rng.random(len(t))]
    if repeat and len(t):
        twice = rng.permutation(len(t))[:5]
        rows += [Lp[ji[twice]], Lp[r // 2:r // 2 + 1]]
        cols += [jt[twice], np.array([r // 2])]
        order += [rng.random(len(twice)), order[0][r // 2:r // 2 + 1] + 1.0]
    if above and r > 1:
        some = rng.permutation(r - 1)[:(r + 1) // 2]
        rows.append(Lp[some])
        cols.append(rng.integers(some + 1, r))
        order.append(rng.random(len(some)))
    if nonpivot and extra_rows:
        others = np.setdiff1d(np.arange(n), Lp)
        pick = _distinct(rng, r, min(3, r), len(others))
        rows.append(np.repeat(others, pick.shape[1]))
        cols.append(pick.ravel())
        order.append(rng.random(pick.size))
    rows, cols, order = np.concatenate(rows), np.concatenate(cols).astype(np.int64), np.concatenate(order)
    return _csr(n, r, rows, cols, _values(rng, p, len(rows)), order, p), Lp.astype(np.int32)


def layered(rng, p, widths, deps, lwidths=None, ldeps=None, ncheck=0, check_used=1.0, check_per_row=2, row_order=None,
            extra_rows=0, nonpivot=False, above=False, repeat=False):
    """(U, qinv, L, Lp): U's sweep from (widths, deps), L's from (lwidths, ldeps) (default: the same lists, drawn anew)"""
    lwidths, ldeps = (widths, deps) if lwidths is None else (lwidths, ldeps)
    assert sum(widths) == sum(lwidths)
    U, qinv = upper(rng, p, widths, deps, ncheck, check_used, check_per_row, row_order)
    L, Lp = lower(rng, p, lwidths, ldeps, extra_rows, nonpivot, above, repeat)
    return U, qinv, L, Lp


def _sparse_rows(M, p):
    Mp, Mj, Mx = np.asarray(M.p).tolist(), np.asarray(M.j).tolist(), (np.asarray(M.x, np.int64) % p).tolist()
    return lambda i: zip(Mj[Mp[i]:Mp[i + 1]], Mx[Mp[i]:Mp[i + 1]])


def right_hand_sides(rng, p, U, qinv, L, k, dense_rows=True, unbalanced=False, extra_cols=None, combine=3):
    """k rows of B: combinations of rows of L.U (every third of all rows, the others of 1 to 17 rows, so the lengths differ;
    dense_rows=False: of `combine` rows, through sparse products); the odd ones with one more entry in a column without a pivot
    (extra_cols: which ones); for k >= 4 row k-2 is zero and row k-1 holds one of its columns twice, the second time at the
    end of the row.  unbalanced: the values are stored in [0, p) (p < 2^31)."""
    n, m = L.n, U.m
    free = np.flatnonzero(np.asarray(qinv) < 0) if extra_cols is None else np.asarray(extra_cols)
    lines = []
    if dense_rows:
        X0 = np.zeros((k, n), np.int64)
        for t in range(k):
            some = np.arange(n) if t % 3 == 0 else rng.permutation(n)[:1 + (5 * t) % 17]
            X0[t, some] = rng.integers(1, p, size=len(some), dtype=np.int64)
        D = mulmod(mulmod(X0, dense(L), p), dense(U), p) if k else np.zeros((0, m), np.int64)
        for t in range(k):
            cols = np.flatnonzero(D[t])
            lines.append(dict(zip(cols.tolist(), D[t, cols].tolist())))
    else:
        Lrow, Urow = _sparse_rows(L, p), _sparse_rows(U, p)
        for t in range(k):
            y, b = {}, {}
            for i in rng.permutation(n)[:combine].tolist():
                c = int(rng.integers(1, p))
                for j, v in Lrow(i):
                    y[j] = (y.get(j, 0) + c * v) % p
            for i, c in y.items():
                if c:
                    for j, v in Urow(i):
                        b[j] = (b.get(j, 0) + c * v) % p
            lines.append({j: v for j, v in b.items() if v})
    ptr, cols, vals = [0], [], []
    for t, b in enumerate(lines):
        if t % 2 and len(free):
            c = int(rng.choice(free))
            b[c] = (b.get(c, 0) + int(rng.integers(1, p))) % p
        if k >= 4 and t == k - 2:
            b = {}
        row = [(c, b[c]) for c in sorted(b) if b[c]]
        if k >= 4 and t == k - 1:
            if not row:
                row = [(0, 1)]
            c, v = row[len(row) // 2]
            a = int(rng.integers(1, p))
            row[len(row) // 2] = (c, a)
            row.append((c, (v - a) % p))
        cols += [c for c, _ in row]
        vals += [v for _, v in row]
        ptr.append(len(cols))
    x = np.asarray(vals, np.int64).astype(np.int32) if unbalanced else balanced(np.asarray(vals, np.int64), p)
    return spasm_amd.Csr(k, m, np.asarray(ptr, np.int64), np.asarray(cols, np.int32), x, p)


# ---- the plan ----
def _levels(r, t, i, order):
    """level of every unknown: 0 without dependencies, else 1 + the highest level it depends on (`order`: the solve order)"""
    at = np.argsort(t, kind="stable")
    ptr = np.zeros(r + 1, np.int64)
    np.cumsum(np.bincount(t, minlength=r), out=ptr[1:])
    ptr, on = ptr.tolist(), i[at].tolist()
    level = [0] * r
    for u in order:
        if ptr[u] < ptr[u + 1]:
            level[u] = 1 + max(level[d] for d in on[ptr[u]:ptr[u + 1]])
    return np.asarray(level, np.int64), np.diff(np.asarray(ptr))


def _sweep(r, t, i, order):
    """what finish_sweep makes of the dependencies (t on i): levels, launches, and how many of them split / are runs"""
    level, ndeps = _levels(r, t, i, order)
    nlev = int(level.max()) + 1 if r else 0
    width = np.bincount(level, minlength=nlev)
    deps = np.bincount(level, weights=ndeps, minlength=nlev).astype(np.int64)
    steps, l = [], 0
    while l < nlev:
        e = l
        while e < nlev and width[e] <= SV_THIN:
            e += 1
        if e - l < SV_RUN:
            e = l + 1
        steps.append((l, e, bool(deps[l:e].sum() >= SV_SPLIT * width[l:e].sum())))
        l = e
    return {"levels": nlev, "launches": len(steps), "split": sum(s[2] for s in steps), "run": sum(s[1] - s[0] > 1 for s in steps),
            "steps": steps}


def planned(U, qinv, L, Lp):
    """the solver's plan for Fact(U, qinv, L, Lp): {"F": sweep, "B": sweep, "checked": checked columns, "late": pivot columns
    among them, "check_waves", "emit_chunks"}; a sweep is {"levels", "launches", "split", "run", "steps": [(first level, last
    + 1, split)]}"""
    r = U.n
    qinv = np.asarray(qinv, np.int64)
    rows = np.repeat(np.arange(r, dtype=np.int64), np.diff(np.asarray(U.p, np.int64)))
    cols, vals = np.asarray(U.j, np.int64)[:len(rows)], np.asarray(U.x)[:len(rows)]
    rest = np.ones(len(rows), bool)
    rest[np.asarray(U.p, np.int64)[:-1]] = False                # (the pivot comes first)
    rest &= vals != 0
    t = qinv[cols]
    fwd = rest & (t > rows)
    F = _sweep(r, t[fwd], rows[fwd], range(r))
    late = np.unique(cols[rest & (t >= 0) & (t < rows)])
    checked = int((qinv < 0).sum()) + len(late)
    jof = np.full(L.n, -1, np.int64)
    jof[np.asarray(Lp, np.int64)] = np.arange(r)
    rows = np.repeat(np.arange(L.n, dtype=np.int64), np.diff(np.asarray(L.p, np.int64)))
    cols, vals = np.asarray(L.j, np.int64)[:len(rows)], np.asarray(L.x)[:len(rows)]
    back = (jof[rows] >= 0) & (cols < jof[rows]) & (vals != 0)
    B = _sweep(r, cols[back], jof[rows][back], range(r - 1, -1, -1))
    return {"F": F, "B": B, "checked": checked, "late": len(late), "check_waves": check_waves(checked), "emit_chunks": emit_chunks(r)}


def summary(sweep):
    return {k: sweep[k] for k in ("levels", "launches", "split", "run")}


# ---- the shapes of tests/test_gpu_solve_shapes.py ----
def _cycle(values, w, start=0):
    return [values[(start + t) % len(values)] for t in range(w)]


_COUNTS = [1, 2, 3, 4, 5, 7, 8, 63]                 # around the unrolling by 4 (tails 0..3) and just below the split
STRUCTURES = {
    # one level per launch: widths above thin that are no multiple of 4 waves; a single thin level between wide ones
    "sweep": ([64, 17, 18, 21, 5, 33], [0, _cycle(_COUNTS, 17), _cycle(_COUNTS, 18, 3), _cycle(_COUNTS, 21, 5), _cycle(_COUNTS, 5, 2),
                                        _cycle(_COUNTS, 33)]),
    # runs of 2, 3 and 2 levels of widths 1, 15, 16; 17 and 18 break them; the last run ends at the last level
    "runs": ([43, 1, 16, 17, 15, 16, 1, 18, 16, 15], [0, 1, _cycle(_COUNTS[:7], 16), 3, _cycle(_COUNTS[:7], 15, 2), 2, 5,
                                                      _cycle(_COUNTS[:7], 18), 4, _cycle(_COUNTS[:7], 15, 4)]),
    # a wide level, then a chain of 200 thin ones in one launch
    "chain": ([290] + ([1] * 6 + [16, 15]) * 25, [0] + [1, 2, 1, 3, 1, 4, _cycle(_COUNTS[:7], 16), _cycle(_COUNTS[:7], 15, 1)] * 25),
    # split, one level: averages of exactly 63 (stays whole) and exactly 64 (splits); lists of 64, 65, 100 and 1,003; lists of
    # 5 and 17 (waves with empty slices) next to long ones, in a wide level and in a thin level on its own
    "split": ([1100, 17, 20, 17, 18, 3, 40], [0, [64, 62] + [63] * 15, [64] * 16 + [65, 63, 100, 28], [1003] + [64] * 16,
                                              [5, 17, 1130] + [64] * 15, [5, 17, 300], _cycle(_COUNTS[:7], 40)]),
    # split, a run of three thin levels
    "split_run": ([400, 1, 3, 2], [0, 300, [70, 150, 299], [71, 200]]),
    "split_run2": ([400, 2, 1, 3], [0, [299, 70], 300, [100, 75, 180]]),
}
CLAIMS = {
    "sweep": {"levels": 6, "launches": 6, "split": 0, "run": 0},
    "runs": {"levels": 10, "launches": 6, "split": 0, "run": 3},
    "chain": {"levels": 201, "launches": 2, "split": 0, "run": 1},
    "split": {"levels": 7, "launches": 7, "split": 4, "run": 0},
    "split_run": {"levels": 4, "launches": 2, "split": 1, "run": 1},
    "split_run2": {"levels": 4, "launches": 2, "split": 1, "run": 1},
}
# (U's structure, L's structure): each as U's and as L's, two different ones in a case
PAIRS = [("sweep", "runs"), ("runs", "sweep"), ("split", "chain"), ("chain", "split"), ("split_run", "split_run2"),
         ("split_run2", "split_run")]


def pair_case(u, l, p, seed=0, **options):
    rng = np.random.default_rng([seed, p % 65521, sorted(STRUCTURES).index(u), sorted(STRUCTURES).index(l)])
    return layered(rng, p, *STRUCTURES[u], *STRUCTURES[l], **options), rng


def flat(r, depth=3):
    """a cheap structure of r unknowns: `depth` levels, 1 to 3 dependencies"""
    w = [r - (depth - 1) * (r // (depth + 1))] + [r // (depth + 1)] * (depth - 1)
    return w, [0] + [_cycle([1, 2, 3], x) for x in w[1:]]


K_VALUES = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2049]       # around a block of 64 and the scan's chunk of 1,024 (carry: 1,025, 2,049)
K_RANK = 1120                                               # 2 emit chunks
EMIT_RANKS = {1023: 1, 1024: 2, 1535: 2, 2563: 5}           # rank: emit chunks (2,563 / 5: uneven bounds, more chunks than waves)
WIDE_RANK = 131072 + 700                                    # 257 -> the cap of 256 chunks
CHECK_COLUMNS = {0: 1, 1: 1, 8: 1, 9: 2, 4100: 512}         # columns without a pivot: waves of the check
ODDITIES = ["nonpivot", "above", "repeat", "row_order", "all"]


def flat_case(r, p, seed=1, **options):
    rng = np.random.default_rng([seed, r, p % 65521])
    return layered(rng, p, *flat(r), **options), rng


def check_case(nc, p, row_order=None, check_used=1.0):
    rng = np.random.default_rng([2, nc, p % 65521, {None: 0, "reversed": 1, "half": 2}[row_order], int(check_used * 100)])
    return layered(rng, p, [40, 30, 20], [0, _cycle([1, 2, 5], 30), _cycle([1, 3, 4], 20)], ncheck=nc, check_used=check_used,
                   check_per_row=min(nc, 10), row_order=row_order), rng


def oddity_case(which, p):
    rng = np.random.default_rng([3, ODDITIES.index(which), p % 65521])
    every = which == "all"
    return layered(rng, p, *STRUCTURES["runs"], *STRUCTURES["sweep"], ncheck=7, extra_rows=9, nonpivot=every or which == "nonpivot",
                   above=every or which == "above", repeat=every or which == "repeat",
                   row_order="half" if every or which == "row_order" else None), rng
