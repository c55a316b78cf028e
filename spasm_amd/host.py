"""Host-pointer entry points: same names, argument meaning and results as the reference's C API."""
import ctypes as C

import numpy as np

from ._lib import lib, require_gpu
from .matrix import Csr, Fact, CLu, CCertificate, EchelonizeOpts, view_csr, copy_csr

_libc = C.CDLL(None)
_libc.fopen.restype = C.c_void_p
_libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
_libc.fclose.argtypes = [C.c_void_p]
_libc.free.argtypes = [C.c_void_p]


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def load(path, prime, transpose_if_wide=False, with_hash=False):
    """spasm_triplet_load + spasm_compress (spasm_io.c:60, spasm_triplet.c:97) of an SMS / MatrixMarket file.
    with_hash: returns (A, hash), hash the 32-byte SHA-256 digest of the file that spasm_triplet_load computes (bytes)."""
    L = lib()
    f = _libc.fopen(path.encode(), b"r")
    if not f:
        raise OSError("cannot open %s" % path)
    digest = (C.c_uint8 * 32)()
    try:
        T = L.spasm_hip_triplet_load(f, prime, digest if with_hash else None)
    finally:
        _libc.fclose(f)
    if transpose_if_wide and T.contents.n < T.contents.m:
        L.spasm_hip_triplet_transpose(T)
    A = L.spasm_hip_compress(T)
    out = copy_csr(A)
    L.spasm_hip_csr_free(A)
    L.spasm_hip_triplet_free(T)
    return (out, bytes(digest)) if with_hash else out


def compress(prime, n, m, ti, tj, tx):
    """triplets (0-based) -> Csr through spasm_hip_add_entry / spasm_hip_compress."""
    L = lib()
    T = L.spasm_hip_triplet_alloc(n, m, max(len(ti), 1), prime, True)
    for a, b, c in zip(np.asarray(ti).tolist(), np.asarray(tj).tolist(), np.asarray(tx).tolist()):
        L.spasm_hip_add_entry(T, a, b, c)
    A = L.spasm_hip_compress(T)
    out = copy_csr(A)
    L.spasm_hip_csr_free(A)
    L.spasm_hip_triplet_free(T)
    return out


def transpose(A):
    L = lib()
    a = view_csr(A)
    t = L.spasm_hip_transpose(C.byref(a), 1)
    out = copy_csr(t)
    L.spasm_hip_csr_free(t)
    return out


def empty_fact(m, prime):
    return Fact(Csr(0, m, np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32), prime),
                np.full(m, -1, np.int32))


def _lu_for(F, extra_rows, extra_nz):
    """library-owned struct spasm_lu initialised from a Fact, with room to grow."""
    L = lib()
    U = F.U
    up = L.spasm_hip_csr_alloc(U.n + extra_rows, U.m, max(U.nnz + extra_nz, 1), U.prime, True)
    s = up.contents
    C.memmove(s.p, U.p.ctypes.data, 8 * (U.n + 1))
    if U.nnz:
        C.memmove(s.j, U.j.ctypes.data, 4 * U.nnz)
        C.memmove(s.x, U.x.ctypes.data, 4 * U.nnz)
    up.contents.n = U.n
    qinv = F.qinv.copy()
    lu = CLu()
    lu.r = U.n
    lu.complete = False
    lu.L = None
    lu.U = up
    lu.qinv = _ip(qinv)
    lu.p = None
    lu.Ltmp = None
    if getattr(F, "L", None) is not None and getattr(F, "Lp", None) is not None:
        # L and p of an echelonization with opts.L: views of F's arrays, kept alive by lu
        lu._keep = (F.L, view_csr(F.L), np.ascontiguousarray(F.Lp, np.int32))
        lu.L = C.pointer(lu._keep[1])
        lu.p = _ip(lu._keep[2])
    return lu, up, qinv


def pivots_extract_structural(A, F, greedy=True):
    """spasm_pivots_extract_structural (spasm_pivots.c:369): returns (npiv, p, F + new pivotal rows)."""
    L = lib()
    a = view_csr(A)
    lu, up, qinv = _lu_for(F, A.n, A.nnz)
    opts = EchelonizeOpts()
    opts.enable_greedy_pivot_search = bool(greedy)
    p = np.zeros(max(A.n, 1), np.int32)
    npiv = L.spasm_hip_pivots_extract_structural(C.byref(a), None, C.byref(lu), _ip(p), C.byref(opts))
    out = Fact(copy_csr(lu.U), qinv)
    L.spasm_hip_csr_free(lu.U)
    return npiv, p[:A.n], out


def schur(A, p, F, p_in=None, want_L=False):
    """spasm_schur (spasm_schur.c:61) on the GPU: returns (S, p_out), or (S, p_out, (Li, Lj, Lx)) with
    want_L: the elimination coefficients as triplets (row, index of the pivot row in U, value)."""
    require_gpu("schur")
    L = lib()
    a = view_csr(A)
    lu, up, qinv = _lu_for(F, 0, 0)
    p = np.ascontiguousarray(p, np.int32)
    n = len(p)
    p_out = np.zeros(max(n, 1), np.int32)
    pin = _ip(np.ascontiguousarray(p_in, np.int32)) if p_in is not None else None
    T = L.spasm_hip_triplet_alloc(max(A.n, 1), max(F.U.n, 1), 16, A.prime, True) if want_L else None
    s = L.spasm_hip_schur(C.byref(a), _ip(p), n, C.byref(lu), -1.0, T, pin, _ip(p_out))
    S = copy_csr(s)
    L.spasm_hip_csr_free(s)
    L.spasm_hip_csr_free(up)
    if not want_L:
        return S, p_out[:n]
    t = T.contents
    nz = int(t.nz)
    trip = tuple(np.ctypeslib.as_array(arr, shape=(max(nz, 1),))[:nz].copy() for arr in (t.i, t.j, t.x))
    L.spasm_hip_triplet_free(T)
    return S, p_out[:n], trip


class ResidentSchur:
    """spasm_hip_schur_resident on fixed arguments, call after call: spasm_hip_schur the way spasm_hip_echelonize calls it between
    two rounds (entries of S left on the device, the installed communicator in force) -- what bench.py times on several GPUs.
    forget=True: the cached factor images drop R before every call, so that a call pays for all of spasm_schur."""

    def __init__(self, A, p, F):
        require_gpu("ResidentSchur")
        self._a = view_csr(A)
        self._lu, self._up, self._qinv = _lu_for(F, 0, 0)
        self._p = np.ascontiguousarray(p, np.int32)
        self._keep = (A, F)

    def __call__(self, forget=True, est_density=-1.0):
        L = lib()
        if forget:
            L.spasm_hip_forget_cached_images()
        return int(L.spasm_hip_schur_resident(C.byref(self._a), _ip(self._p), len(self._p), C.byref(self._lu), est_density))

    def close(self):
        if self._up is not None:
            lib().spasm_hip_csr_free(self._up)
            self._up = None


SPASM_DOUBLE, SPASM_FLOAT, SPASM_I64 = 0, 1, 2      # spasm_datatype (spasm.h:139)
_NP_OF = {SPASM_DOUBLE: np.float64, SPASM_FLOAT: np.float32, SPASM_I64: np.int64}


def schur_dense(A, p, F, p_in=None, datatype=SPASM_I64):
    """spasm_schur_dense (spasm_schur.c:257) on the GPU: returns (S [n, Sm], q, p_out)."""
    require_gpu("schur_dense")
    L = lib()
    a = view_csr(A)
    lu, up, qinv = _lu_for(F, 0, 0)
    p = np.ascontiguousarray(p, np.int32)
    n = len(p)
    Sm = A.m - F.U.n
    S = np.zeros(max(n * Sm, 1), _NP_OF[datatype])
    q = np.zeros(max(Sm, 1), np.int32)
    p_out = np.zeros(max(n, 1), np.int32)
    pin = _ip(np.ascontiguousarray(p_in, np.int32)) if p_in is not None else None
    L.spasm_hip_schur_dense(C.byref(a), _ip(p), n, pin, C.byref(lu), S.ctypes.data, datatype, _ip(q), _ip(p_out))
    L.spasm_hip_csr_free(up)
    return S[:n * Sm].reshape(n, Sm), q[:Sm], p_out[:n]


def ffpack_rref(prime, M, datatype=SPASM_I64):
    """spasm_ffpack_rref (spasm_ffpack.cpp:88) on the GPU, on a copy of M: returns (rank, R, qinv)."""
    require_gpu("ffpack_rref")
    L = lib()
    M = np.ascontiguousarray(M, _NP_OF[datatype]).copy()
    n, m = M.shape
    qinv = np.zeros(max(m, 1), np.uint64)
    r = L.spasm_hip_ffpack_rref(prime, n, m, M.ctypes.data, m, datatype, qinv.ctypes.data_as(C.POINTER(C.c_size_t)))
    return r, M, qinv[:m].astype(np.int64)


def ffpack_LU(prime, M, datatype=SPASM_I64):
    """spasm_ffpack_LU (spasm_ffpack.cpp:137) on the GPU, on a copy of M: returns (rank, packed LU, P, Qinv)."""
    require_gpu("ffpack_LU")
    L = lib()
    M = np.ascontiguousarray(M, _NP_OF[datatype]).copy()
    n, m = M.shape
    P = np.zeros(max(n, 1), np.uint64)
    Q = np.zeros(max(m, 1), np.uint64)
    r = L.spasm_hip_ffpack_LU(prime, n, m, M.ctypes.data, m, datatype, P.ctypes.data_as(C.POINTER(C.c_size_t)),
                              Q.ctypes.data_as(C.POINTER(C.c_size_t)))
    return r, M, P[:n].astype(np.int64), Q[:m].astype(np.int64)


def default_opts():
    o = EchelonizeOpts()
    lib().spasm_hip_echelonize_init_opts(C.byref(o))
    return o


def echelonize(A, opts=None):
    """spasm_echelonize (spasm_echelonize.c:473): returns Fact(U, qinv) with rank = U.n."""
    require_gpu("echelonize")
    L = lib()
    a = view_csr(A)
    lu = L.spasm_hip_echelonize(C.byref(a), C.byref(opts) if opts is not None else None)
    s = lu.contents
    U = copy_csr(s.U)
    qinv = np.ctypeslib.as_array(s.qinv, shape=(max(A.m, 1),))[:A.m].copy()
    F = Fact(U, qinv)
    F.L, F.Lp = None, None
    if bool(s.L):                       # opts.L: A == L * U, pivot j of L sits on row Lp[j]
        F.L = copy_csr(s.L)
        F.Lp = np.ctypeslib.as_array(s.p, shape=(max(U.n, 1),))[:U.n].copy()
    L.spasm_hip_lu_free(lu)
    return F


def echelonize_profile():
    """seconds of the last echelonize() call: dict(total, pivot_search, density_estimates, sparse_schur, dense_finish,
    sparse_rounds, structural_finish)."""
    out = (C.c_double * 8)()
    lib().spasm_hip_echelonize_profile(out)
    return {"total": out[0], "pivot_search": out[1], "density_estimates": out[2], "sparse_schur": out[3],
            "dense_finish": out[4], "sparse_rounds": int(out[5]), "structural_finish": out[6], "uploads_so_far": int(out[7])}


COUNTER_NAMES = ("pool_retries", "pools_sized_from_a_sample", "sparse_image_chunk_extensions", "sparse_image_build_aborts",
                 "block_cache_misses", "block_cache_miss_bytes", "factor_plans", "pivot_visits", "pivot_visits_of_searches_with_a_pivot",
                 "pivot_cascade_items", "pivot_rows_with_a_pivot", "pivot_rows_without", "pivots_accepted_on_labels_alone",
                 "pivot_rows_deferred_to_the_ticket_search", "schur_complements_kept_as_column_slabs", "column_slabs_gathered_into_whole_rows")


def echelonize_counters():
    """events since the last echelonize() call started that its time split does not show (spasm_hip_echelonize_counters):
    pool retries, extensions of the sparse image, block-cache misses, factor plans, visits of the pivot search by outcome."""
    out = (C.c_longlong * len(COUNTER_NAMES))()
    lib().spasm_hip_echelonize_counters(out, len(COUNTER_NAMES))
    return {k: int(out[t]) for t, k in enumerate(COUNTER_NAMES)}


def rref(F):
    """spasm_rref (spasm_rref.c:25): returns (R, Rqinv)."""
    require_gpu("rref")
    L = lib()
    lu, up, qinv = _lu_for(F, 0, 0)
    Rq = np.zeros(max(F.U.m, 1), np.int32)
    r = L.spasm_hip_rref(C.byref(lu), _ip(Rq))
    R = copy_csr(r)
    L.spasm_hip_csr_free(r)
    L.spasm_hip_csr_free(up)
    return R, Rq[:F.U.m]


def kernel(F):
    """spasm_kernel (spasm_kernel.c:9): basis of the right kernel, one vector per row."""
    require_gpu("kernel")
    L = lib()
    lu, up, qinv = _lu_for(F, 0, 0)
    k = L.spasm_hip_kernel(C.byref(lu))
    K = copy_csr(k)
    L.spasm_hip_csr_free(k)
    L.spasm_hip_csr_free(up)
    return K


def kernel_basis(F):
    """spasm_hip_kernel_basis: the array kernel(F) returns, with the reduced rows of U, their transpose and K formed on the GPU."""
    require_gpu("kernel_basis")
    L = lib()
    lu, up, qinv = _lu_for(F, 0, 0)
    k = L.spasm_hip_kernel_basis(C.byref(lu))
    K = copy_csr(k)
    L.spasm_hip_csr_free(k)
    L.spasm_hip_csr_free(up)
    return K


def kernel_stats():
    """spasm_hip_kernel_stats: the last kernel_basis() call, stage by stage (ms), and its counts"""
    out = (C.c_double * 9)()
    lib().spasm_hip_kernel_stats(out, 9)
    keys = ("image_ms", "reduce_ms", "transpose_ms", "assemble_ms", "download_ms", "total_ms", "nnz", "pool_retries", "rows")
    return {k: out[t] for t, k in enumerate(keys)}


def transpose_device(A, keep_values=True):
    """spasm_hip_transpose_device: A^T formed on the GPU, equal to transpose(A) array for array (entries of a row by increasing
    row of A).  A.x may be None (a pattern); the result's x is None then, and with keep_values=False."""
    if A.p[0] != 0 or np.any(np.diff(A.p) < 0) or len(A.j) < A.nnz:
        raise ValueError("spasm_amd.transpose_device: the row pointers of A are malformed")
    require_gpu("transpose_device")
    L = lib()
    a = view_csr(A)
    t = L.spasm_hip_transpose_device(C.byref(a), 1 if keep_values else 0)
    out = copy_csr(t)
    L.spasm_hip_csr_free(t)
    return out


def transpose_stats():
    """spasm_hip_transpose_stats: the last device transposition: ms per stage, columns per route, the longest column, row chunks"""
    out = (C.c_double * 9)()
    lib().spasm_hip_transpose_stats(out, 9)
    keys = ("upload_ms", "count_scan_ms", "fill_ms", "order_ms", "download_ms", "short_columns", "long_columns", "longest_column",
            "row_chunks")
    return {k: out[t] for t, k in enumerate(keys)}


def _check_solvable(F, m, prime, what):
    if getattr(F, "L", None) is None or getattr(F, "Lp", None) is None:
        raise ValueError("spasm_amd.%s needs a factorization with L (echelonize with opts.L = True)" % what)
    if F.L.m != F.U.n or len(F.Lp) < F.U.n:
        raise ValueError("spasm_amd.%s: L has %d columns and %d pivot rows, U has %d rows" % (what, F.L.m, len(F.Lp), F.U.n))
    if F.L.prime != F.U.prime:
        raise ValueError("spasm_amd.%s: L is mod %d, U mod %d" % (what, F.L.prime, F.U.prime))
    if m != F.U.m:
        raise ValueError("spasm_amd.%s: the right-hand sides have %d columns, U has %d" % (what, m, F.U.m))
    if prime != F.U.prime:
        raise ValueError("spasm_amd.%s: the right-hand sides are mod %d, the factorization mod %d" % (what, prime, F.U.prime))


def _gesv_call(fn, B):
    b = view_csr(B)
    ok = np.zeros(max(B.n, 1), np.bool_)
    x = fn(C.byref(b), ok.ctypes.data_as(C.POINTER(C.c_bool)))
    X = copy_csr(x)
    lib().spasm_hip_csr_free(x)
    return X, ok[:B.n].copy()


class Solver:
    """spasm_hip_solver: the plan of the three sweeps for one factorization (with L), reused by every gesv() call.
    levels: dict(forward, back, forward_launches, back_launches)."""

    def __init__(self, F):
        _check_solvable(F, F.U.m, F.U.prime, "Solver")
        require_gpu("Solver")
        L = lib()
        lu, up, qinv = _lu_for(F, 0, 0)
        self._S = L.spasm_hip_solver_create(C.byref(lu))
        L.spasm_hip_csr_free(up)
        self.m, self.n, self.prime = F.U.m, F.L.n, F.U.prime
        out = (C.c_int * 4)()
        L.spasm_hip_solver_levels(self._S, out)
        self.levels = {"forward": out[0], "back": out[1], "forward_launches": out[2], "back_launches": out[3]}

    def gesv(self, B):
        """(X, ok) as spasm_gesv (spasm_solve.c:52) returns them: X is B.n x (rows of A), ok[i] iff row i of B lies in the row
        space of U; rows without a solution hold what the reference computes for them."""
        if self._S is None:
            raise ValueError("Solver is closed")
        if B.m != self.m or B.prime != self.prime:
            raise ValueError("spasm_amd.Solver.gesv: B is %d columns mod %d, the factorization %d columns mod %d"
                             % (B.m, B.prime, self.m, self.prime))
        S = self._S
        return _gesv_call(lambda b, ok: lib().spasm_hip_solver_gesv(S, b, ok), B)

    def stats(self):
        """spasm_hip_solver_stats: the plan's seconds and the last gesv's device ms per sweep, launches, bytes, batches; of the
        plan, per batch: the launches of each sweep that split every dependency list over a workgroup, and those that step
        through a run of levels."""
        out = (C.c_double * 16)()
        lib().spasm_hip_solver_stats(self._S, out, 16)
        keys = ("plan_s", "scatter_ms", "forward_ms", "check_ms", "back_ms", "emit_ms", "forward_launches", "back_launches",
                "launches", "sweep_bytes", "batches", "rhs_per_batch", "forward_split_launches", "back_split_launches",
                "forward_run_launches", "back_run_launches")
        return {k: out[t] for t, k in enumerate(keys)}

    def close(self):
        if self._S is not None:
            lib().spasm_hip_solver_destroy(self._S)
            self._S = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def gesv(F, B):
    """spasm_gesv (spasm_solve.c:52): solves X.A = B over F (from echelonize with opts.L).  Returns (X: Csr, ok: bool array)."""
    _check_solvable(F, B.m, B.prime, "gesv")
    require_gpu("gesv")
    L = lib()
    lu, up, qinv = _lu_for(F, 0, 0)
    try:
        return _gesv_call(lambda b, ok: L.spasm_hip_gesv(C.byref(lu), b, ok), B)
    finally:
        L.spasm_hip_csr_free(up)


def solve(F, b):
    """spasm_solve (spasm_solve.c:13): x.A = b for one dense b (U.m values).  Returns (x: int32 array of A's rows, ok)."""
    b = np.ascontiguousarray(b, np.int32)
    if b.ndim != 1:
        raise ValueError("spasm_amd.solve: b must be one vector")
    _check_solvable(F, len(b), F.U.prime, "solve")
    require_gpu("solve")
    L = lib()
    lu, up, qinv = _lu_for(F, 0, 0)
    x = np.zeros(max(F.L.n, 1), np.int32)
    try:
        ok = L.spasm_hip_solve(C.byref(lu), b.ctypes.data_as(C.POINTER(C.c_int32)), x.ctypes.data_as(C.POINTER(C.c_int32)))
    finally:
        L.spasm_hip_csr_free(up)
    return x[:F.L.n], bool(ok)


# ---- x.A and rank certificates (spasm_spmv.c, spasm_certificate.c; spasm_amd/csrc/spmv.hip, host_cert.cpp) ----

def _i32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


def xApy(X, A, Y=None):
    """spasm_xApy (spasm_spmv.c:9) on the GPU: Y + X.A mod p, balanced.  X is one vector (A.n values) or a k x A.n batch (one
    pass over A for all k); Y (same shape as the result, default zeros) is not modified."""
    X = np.asarray(X)
    one = X.ndim == 1
    X = np.ascontiguousarray(X.reshape(1, -1) if one else X, np.int64)
    if X.ndim != 2 or X.shape[1] != A.n:
        raise ValueError("spasm_amd.xApy: X has shape %s, A has %d rows" % (X.shape, A.n))
    k = X.shape[0]
    if k > 64:
        raise ValueError("spasm_amd.xApy: at most 64 vectors per call (%d)" % k)
    Yout = np.zeros((k, A.m), np.int64) if Y is None else np.array(Y, np.int64).reshape(k, A.m)
    require_gpu("xApy")
    p = A.prime
    Xc = np.ascontiguousarray(_balanced(X, p))
    Yc = np.ascontiguousarray(_balanced(Yout, p))
    a = view_csr(A)
    lib().spasm_hip_xApy_batch(C.byref(a), k, _i32p(Xc) if Xc.size else None, _i32p(Yc) if Yc.size else None)
    return Yc[0] if one else Yc


def xApy_stats():
    """spasm_hip_xApy_stats: the last x.A call's device ms (upload of A, its column-major image, the product), algorithmic bytes."""
    out = (C.c_double * 8)()
    lib().spasm_hip_xApy_stats(out, 8)
    keys = ("upload_ms", "image_ms", "product_ms", "product_bytes", "k", "short_columns", "long_columns", "nnz")
    return {k: out[t] for t, k in enumerate(keys)}


def _balanced(v, p):
    v = np.asarray(v, np.int64) % p
    return np.where(v > p // 2, v - p, v).astype(np.int32)


class Certificate:
    """struct spasm_rank_certificate (spasm.h:110-118): rank r, modulus, the 32-byte hash of the input, pivot rows i, pivot
    columns j, and the solutions x and y on the pivot rows (balanced)."""

    def __init__(self, r, prime, hash, i, j, x, y):
        self.r, self.prime, self.hash = int(r), int(prime), bytes(hash)
        self.i, self.j = (np.ascontiguousarray(v, np.int32) for v in (i, j))
        self.x, self.y = (np.ascontiguousarray(v, np.int32) for v in (x, y))
        if len(self.hash) != 32:
            raise ValueError("a certificate hash has 32 bytes")

    def copy(self):
        return Certificate(self.r, self.prime, self.hash, self.i.copy(), self.j.copy(), self.x.copy(), self.y.copy())

    def __eq__(self, other):
        return (isinstance(other, Certificate) and (self.r, self.prime, self.hash) == (other.r, other.prime, other.hash)
                and all(np.array_equal(a, b) for a, b in zip((self.i, self.j, self.x, self.y), (other.i, other.j, other.x, other.y))))

    def _c(self):
        """a struct spasm_rank_certificate viewing this object's arrays (kept alive by the struct)"""
        c = CCertificate()
        c.r = self.r
        c.prime = self.prime
        C.memmove(c.hash, self.hash, 32)
        arrays = tuple(np.ascontiguousarray(v if len(v) else np.zeros(1, np.int32), np.int32) for v in (self.i, self.j, self.x, self.y))
        c._keep = arrays
        c.i, c.j, c.x, c.y = (_i32p(v) for v in arrays)
        return c

    @staticmethod
    def _of(c):
        r = max(int(c.r), 0)
        arr = lambda ptr: np.ctypeslib.as_array(ptr, shape=(r,)).copy() if r else np.zeros(0, np.int32)     # noqa: E731
        return Certificate(c.r, c.prime, bytes(c.hash), arr(c.i), arr(c.j), arr(c.x), arr(c.y))

    def save(self, path):
        """spasm_rank_certificate_save (spasm_certificate.c:221): the reference's text format"""
        c = self._c()
        f = _libc.fopen(path.encode(), b"w")
        if not f:
            raise OSError("cannot open %s" % path)
        try:
            lib().spasm_hip_rank_certificate_save(C.byref(c), f)
        finally:
            _libc.fclose(f)

    @staticmethod
    def load(path):
        """spasm_rank_certificate_load (spasm_certificate.c:242), the fifth line read into j; ValueError on a short file"""
        L = lib()
        f = _libc.fopen(path.encode(), b"r")
        if not f:
            raise OSError("cannot open %s" % path)
        c = CCertificate()
        try:
            ok = L.spasm_hip_rank_certificate_load(f, C.byref(c))
        finally:
            _libc.fclose(f)
        out = Certificate._of(c) if ok else None
        for ptr in (c.i, c.j, c.x, c.y):
            _libc.free(C.cast(ptr, C.c_void_p))
        if out is None:
            raise ValueError("%s is not a complete rank certificate" % path)
        return out


def _hash_arg(hash):
    h = bytes(hash)
    if len(h) != 32:
        raise ValueError("the hash has 32 bytes (a SHA-256 digest), not %d" % len(h))
    return (C.c_uint8 * 32).from_buffer_copy(h)


def certificate_rank_create(A, hash, F):
    """spasm_certificate_rank_create (spasm_certificate.c:21) on the GPU: F from echelonize with opts.L on A (the same matrix,
    the same modulus), hash the 32-byte digest of the input (load(..., with_hash=True)).  Returns a Certificate."""
    _check_solvable(F, A.m, A.prime, "certificate_rank_create")
    if F.L.n != A.n:
        raise ValueError("spasm_amd.certificate_rank_create: L has %d rows, A %d" % (F.L.n, A.n))
    h = _hash_arg(hash)
    require_gpu("certificate_rank_create")
    L = lib()
    a = view_csr(A)
    lu, up, qinv = _lu_for(F, 0, 0)
    try:
        c = L.spasm_hip_certificate_rank_create(C.byref(a), h, C.byref(lu))
    finally:
        L.spasm_hip_csr_free(up)
    out = Certificate._of(c.contents)
    L.spasm_hip_rank_certificate_free(c)
    return out


def certificate_rank_verify(A, hash, cert):
    """spasm_certificate_rank_verify (spasm_certificate.c:101) on the GPU: True iff cert proves the rank of A."""
    h = _hash_arg(hash)
    require_gpu("certificate_rank_verify")
    a = view_csr(A)
    c = cert._c()
    return bool(lib().spasm_hip_certificate_rank_verify(C.byref(a), h, C.byref(c)))


def factorization_verify(A, F, seeds=(42, 1337, 21011984)):
    """spasm_factorization_verify (spasm_certificate.c:165) for every seed at once: x.A == (x.L).U for a random x on the pivotal
    rows.  One seed: a bool; a sequence: a list of bools."""
    one = np.ndim(seeds) == 0
    s = np.atleast_1d(np.asarray(seeds, np.uint64))
    _check_solvable(F, A.m, A.prime, "factorization_verify")
    if F.L.n != A.n:
        raise ValueError("spasm_amd.factorization_verify: L has %d rows, A %d" % (F.L.n, A.n))
    require_gpu("factorization_verify")
    L = lib()
    a = view_csr(A)
    lu, up, qinv = _lu_for(F, 0, 0)
    ok = np.zeros(max(len(s), 1), np.bool_)
    try:
        L.spasm_hip_factorization_verify_batch(C.byref(a), C.byref(lu), len(s), s.ctypes.data_as(C.POINTER(C.c_uint64)),
                                               ok.ctypes.data_as(C.POINTER(C.c_bool)))
    finally:
        L.spasm_hip_csr_free(up)
    res = [bool(v) for v in ok[:len(s)]]
    return res[0] if one else res


# ---- maximum matching, Dulmage-Mendelsohn, strongly connected components (spasm_matching.c, spasm_dm.c, spasm_scc.c;
# spasm_amd/csrc/matching.hip, host_dm.cpp) ----

def _check_pattern(A, what):
    """the checks the C side would die on, as a ValueError first"""
    if not isinstance(A, Csr):
        raise ValueError("spasm_amd.%s: A must be a spasm_amd.Csr" % what)
    if A.n < 0 or A.m < 0:
        raise ValueError("spasm_amd.%s: A is %d x %d" % (what, A.n, A.m))
    if A.p[0] != 0 or np.any(np.diff(A.p) < 0) or len(A.j) < A.nnz:
        raise ValueError("spasm_amd.%s: the row pointers of A are malformed" % what)
    j = A.j[:A.nnz]
    if j.size and (j.min() < 0 or j.max() >= A.m):
        raise ValueError("spasm_amd.%s: a column index of A lies outside [0, %d)" % (what, A.m))


class DM:
    """struct spasm_dm (spasm.h:74-82) as numpy arrays: row / column permutations p and q, fine block boundaries r and c (nb + 1
    each), coarse boundaries rr and cc (5 each)."""

    def __init__(self, p, q, r, c, nb, rr, cc):
        self.p, self.q = (np.ascontiguousarray(v, np.int32) for v in (p, q))
        self.r, self.c = (np.ascontiguousarray(v, np.int32) for v in (r, c))
        self.nb = int(nb)
        self.rr, self.cc = (np.ascontiguousarray(v, np.int32) for v in (rr, cc))

    @staticmethod
    def _of(ptr, n, m, L):
        s = ptr.contents
        nb = int(s.nb)
        arr = lambda a, k: np.ctypeslib.as_array(a, shape=(k,)).copy() if k else np.zeros(0, np.int32)     # noqa: E731
        out = DM(arr(s.p, n), arr(s.q, m), arr(s.r, nb + 1), arr(s.c, nb + 1), nb, list(s.rr), list(s.cc))
        L.spasm_hip_dm_free(ptr)
        return out

    def blocks(self):
        """the fine blocks: a list of (rows, columns) of A, in the order of r and c"""
        return [(self.p[self.r[k]:self.r[k + 1]], self.q[self.c[k]:self.c[k + 1]]) for k in range(self.nb)]


def maximum_matching(A):
    """spasm_maximum_matching (spasm_matching.c:103) on the GPU: (jmatch, imatch, size); jmatch[i] is the column matched to row i,
    imatch[j] the row matched to column j, -1 when unmatched.  Any maximum matching (not necessarily the reference's)."""
    _check_pattern(A, "maximum_matching")
    require_gpu("maximum_matching")
    jmatch = np.zeros(max(A.n, 1), np.int32)
    imatch = np.zeros(max(A.m, 1), np.int32)
    a = view_csr(A)
    k = lib().spasm_hip_maximum_matching(C.byref(a), _ip(jmatch), _ip(imatch))
    return jmatch[:A.n], imatch[:A.m], int(k)


def structural_rank(A):
    """the size of a maximum matching of A's pattern (spasm.h:242 declares it; the reference never defines it)"""
    _check_pattern(A, "structural_rank")
    require_gpu("structural_rank")
    a = view_csr(A)
    return int(lib().spasm_hip_structural_rank(C.byref(a)))


def dulmage_mendelsohn(A):
    """spasm_dulmage_mendelsohn (spasm_dm.c:90) on the GPU: a DM in the reference's layout (q = C0|C1|C2|C3, p = R1|R2|R3|R0;
    fine blocks H, the strongly connected components of S, V).  When S is empty nb = 2 (the reference: 0)."""
    _check_pattern(A, "dulmage_mendelsohn")
    require_gpu("dulmage_mendelsohn")
    L = lib()
    a = view_csr(A)
    return DM._of(L.spasm_hip_dulmage_mendelsohn(C.byref(a)), A.n, A.m, L)


def strongly_connected_components(A):
    """spasm_strongly_connected_components (spasm_scc.c:14) of a square A, on the host: p == q, r == c, A(p, p) block upper
    triangular with strongly connected blocks"""
    _check_pattern(A, "strongly_connected_components")
    if A.n != A.m:
        raise ValueError("spasm_amd.strongly_connected_components: A is %d x %d, not square" % (A.n, A.m))
    L = lib()
    a = view_csr(A)
    return DM._of(L.spasm_hip_strongly_connected_components(C.byref(a)), A.n, A.n, L)


def permute(A, p, qinv, with_values=True):
    """spasm_permute (spasm_permutation.c:68): row i of the result is row p[i] of A, column j of A is column qinv[j]; p or qinv
    None: the identity"""
    _check_pattern(A, "permute")
    vecs = []
    for v, k, name in ((p, A.n, "p"), (qinv, A.m, "qinv")):
        if v is None:
            vecs.append(None)
            continue
        v = np.ascontiguousarray(v, np.int32)
        if v.shape != (k,) or not np.array_equal(np.sort(v), np.arange(k)):
            raise ValueError("spasm_amd.permute: %s is not a permutation of 0 .. %d" % (name, k - 1))
        vecs.append(v if k else np.zeros(1, np.int32))
    L = lib()
    a = view_csr(A)
    out = L.spasm_hip_permute(C.byref(a), *(None if v is None else _ip(v) for v in vecs), 1 if with_values else 0)
    B = copy_csr(out)
    L.spasm_hip_csr_free(out)
    return B


def dm_stats():
    """spasm_hip_dm_stats: the last matching / decomposition call, stage by stage (ms) and its counts"""
    out = (C.c_double * 13)()
    lib().spasm_hip_dm_stats(out, 13)
    keys = ("upload_ms", "greedy_ms", "phases_ms", "reach_ms", "coarse_ms", "scc_ms", "total_ms", "greedy_size", "phases",
            "levels", "small_levels", "size", "nb")
    return {k: out[t] for t, k in enumerate(keys)}
