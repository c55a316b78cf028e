"""Timing of X.A = B on the GPU (spasm_amd.Solver / spasm_gesv) against the compiled reference's spasm_gesv on the host.

    python tools/bench_solve.py [--workloads mk12.b3,mk13.b5] [--ks 1,64,1024,8192] [--reps 5] [--ref-sample 64]

For every generated workload: echelonize with opts.L on the GPU, then right-hand sides of which half are random combinations
of 3 rows of A (solvable) and half random sparse rows (4 entries).  Per k: the plan (spasm_hip_solver_create) in ms, the median
solve in ms over --reps runs after one warm-up, RHS/s, levels and launches of F and B, the algorithmic bytes of the sweep
kernels and the fraction of the HBM peak (8 TB/s) they would take at the measured device time of the sweeps.  The reference's
spasm_gesv (oracle/_ref, OpenMP on the CPUs this process may use) runs on the same factorization for --ref-sample rows and
its time for k rows is PROJECTED linearly from that sample (labelled as such).  One JSON line on stdout."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import spasm_amd                      # noqa: E402
import workloads                      # noqa: E402

HBM_PEAK = 8.0e12


def make_rhs(A, k, seed):
    """k rows: even rows random combinations of 3 rows of A, odd rows 4 random entries (balanced values)"""
    p = A.prime
    rng = np.random.default_rng(seed)
    ti, tj, tx = [], [], []
    for t in range(0, k, 2):
        for i in rng.choice(A.n, size=3, replace=False):
            lo, hi = int(A.p[i]), int(A.p[i + 1])
            c = int(rng.integers(1, p))
            ti.append(np.full(hi - lo, t, np.int64))
            tj.append(A.j[lo:hi].astype(np.int64))
            tx.append(A.x[lo:hi].astype(np.int64) * c % p)
    for t in range(1, k, 2):
        ti.append(np.full(4, t, np.int64))
        tj.append(rng.choice(A.m, size=4, replace=False).astype(np.int64))
        tx.append(rng.integers(1, p, size=4, dtype=np.int64))
    ti, tj, tx = np.concatenate(ti), np.concatenate(tj), np.concatenate(tx)
    key = ti * A.m + tj
    uk, inv = np.unique(key, return_inverse=True)
    val = np.zeros(len(uk), np.int64)
    np.add.at(val, inv, tx % p)
    val %= p
    keep = val != 0
    uk, val = uk[keep], val[keep]
    rows = uk // A.m
    ptr = np.zeros(k + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=k), out=ptr[1:])
    val = np.where(val > p // 2, val - p, val).astype(np.int32)
    return spasm_amd.Csr(k, A.m, ptr, (uk % A.m).astype(np.int32), val, p)


def rows_of(B, k):
    return spasm_amd.Csr(k, B.m, B.p[:k + 1].copy(), B.j[:B.p[k]].copy(), B.x[:B.p[k]].copy(), B.prime)


def ref_seconds(F, B, threads):
    from oracle import oracle as orc
    if not orc.ref_available():
        return None, "oracle/_ref not built"
    C = lambda M: orc.CSR(M.n, M.m, M.p, M.j, M.x, M.prime)      # noqa: E731
    orc.ref_set_threads(threads)
    import ctypes
    R = orc.ref()
    R.spasm_gesv.restype = ctypes.POINTER(orc._RefCsr)
    lu, up, q = orc._ref_lu(orc.Fact(C(F.U), F.qinv), 0)
    lp = orc._ref_to(C(F.L))
    pp = np.ascontiguousarray(F.Lp, np.int32).copy()
    lu.L = lp
    lu.p = pp.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    b = orc._ref_to(C(B))
    ok = np.zeros(max(B.n, 1), np.bool_)
    R.spasm_gesv.argtypes = [ctypes.POINTER(orc._RefLu), ctypes.POINTER(orc._RefCsr), ctypes.POINTER(ctypes.c_bool)]
    saved = orc._silence()
    t0 = time.perf_counter()
    try:
        x = R.spasm_gesv(ctypes.byref(lu), b, ok.ctypes.data_as(ctypes.POINTER(ctypes.c_bool)))
    finally:
        orc._unsilence(saved)
    dt = time.perf_counter() - t0
    for ptr in (x, b, lp, up):
        R.spasm_csr_free(ptr)
    return dt, "measured on %d rows with %d OpenMP threads" % (B.n, threads)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="mk12.b3,mk13.b5")
    ap.add_argument("--ks", default="1,64,1024,8192")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ref-sample", type=int, default=64)
    args = ap.parse_args()
    spasm_amd.lib()
    if spasm_amd.device_count() < 1:
        raise SystemExit("bench_solve.py needs an MI355X")
    ks = [int(v) for v in args.ks.split(",")]
    threads = spasm_amd.usable_cpus()
    out = {"metric": "gesv", "hbm_peak_bytes_per_s": HBM_PEAK, "ref_threads": threads, "workloads": []}
    for name in args.workloads.split(","):
        A, source = workloads.load_matrix(name)
        o = spasm_amd.default_opts()
        o.L = True
        t0 = time.perf_counter()
        F = spasm_amd.echelonize(A, o)
        t_fact = time.perf_counter() - t0
        Ball = make_rhs(A, max(ks), seed=7)
        w = {"name": name, "source": source, "n": A.n, "m": A.m, "nnz": A.nnz, "rank": F.U.n, "nnz_L": F.L.nnz,
             "echelonize_with_L_s": round(t_fact, 3), "runs": []}
        t0 = time.perf_counter()
        S = spasm_amd.Solver(F)
        w["plan_ms"] = round(1e3 * (time.perf_counter() - t0), 2)
        w["levels"] = S.levels
        ref_dt, ref_how = ref_seconds(F, rows_of(Ball, min(args.ref_sample, max(ks))), threads)
        for k in ks:
            B = rows_of(Ball, k)
            X, ok = S.gesv(B)                      # warm-up
            times, stats = [], []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                X, ok = S.gesv(B)
                times.append(time.perf_counter() - t0)
                stats.append(S.stats())
            med = float(np.median(times))
            st = stats[int(np.argsort(times)[len(times) // 2])]
            sweep_ms = st["forward_ms"] + st["check_ms"] + st["back_ms"]
            run = {"k": k, "solve_ms_median": round(1e3 * med, 3), "rhs_per_s": round(k / med, 1), "ok": int(ok.sum()),
                   "nnz_X": X.nnz, "device_ms": {key: round(st[key], 3) for key in ("scatter_ms", "forward_ms", "check_ms", "back_ms", "emit_ms")},
                   "launches": {"forward": int(st["forward_launches"]), "back": int(st["back_launches"]), "all": int(st["launches"])},
                   "sweep_bytes": int(st["sweep_bytes"]), "batches": int(st["batches"]),
                   "sweep_hbm_fraction": round(st["sweep_bytes"] / (sweep_ms * 1e-3) / HBM_PEAK, 4) if sweep_ms > 0 else None}
            if ref_dt is not None:
                per = ref_dt / min(args.ref_sample, max(ks))
                run["ref_gesv_s"] = round(per * k, 4)
                run["ref_gesv_s_kind"] = ("measured on %d rows" % k) if k == min(args.ref_sample, max(ks)) else \
                    ("projected from %d measured rows" % min(args.ref_sample, max(ks)))
            w["runs"].append(run)
        w["ref_gesv"] = ref_how
        S.close()
        out["workloads"].append(w)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
