"""Timing of the Dulmage-Mendelsohn decomposition on the GPU (spasm_amd.dulmage_mendelsohn) against the compiled reference's
spasm_dulmage_mendelsohn on the host and scipy's Hopcroft-Karp (maximum_bipartite_matching).

    python tools/bench_dm.py [--workloads mk13.b5,mk13.b5^T,mk14.b4,mk15.b4,gen2M,chain200k] [--reps 5] [--no-ref] [--no-scipy]

GPU: the median of --reps calls after one warm-up, split by stage with spasm_hip_dm_stats (A up and its column-major pattern,
greedy, augmenting phases, the two coarse searches, the coarse sets on the host, the SCCs of S on the host), with the greedy
size, the phases and the BFS levels.  The reference runs once where oracle/_ref exists, single-threaded as it is written; its
stderr goes to /dev/null but its fprintf per row stays inside its time.  scipy runs once where it imports.
Writes profiles/dm_bench_dm.json and prints it as one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import spasm_amd                      # noqa: E402
import workloads                      # noqa: E402
import dm_cases                       # noqa: E402

PRIME = 42013


def matrix(name):
    """(A, description) of a workload; '<name>^T' is the transpose (the wide orientation of an mk matrix)"""
    if name == "gen2M":
        rng = np.random.default_rng(3)
        sizes = [int(s) for s in rng.choice([1, 1, 2, 3, 5, 8, 40, 200], 6000)]
        K = dm_cases.generate(spasm_amd.Csr, PRIME, 600000, sizes, 450000, extra=3, seed=3)
        return K.A, "generated: H 600k rows, S 6000 blocks, V 450k columns"
    if name.startswith("chain"):
        n = int(name[len("chain"):].replace("k", "000"))
        return dm_cases.chain(spasm_amd.Csr, PRIME, n).A, "upper-bidiagonal chain, columns reversed"
    tall = not name.endswith("^T")
    A, src = workloads.load_matrix(name if tall else name[:-2], tall=tall)
    return A, src


def gpu_times(A, reps):
    spasm_amd.dulmage_mendelsohn(A)
    stats, walls = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        spasm_amd.dulmage_mendelsohn(A)
        walls.append(time.perf_counter() - t0)
        stats.append(spasm_amd.dm_stats())
    out = {k: round(float(np.median([s[k] for s in stats])), 3) for k in stats[0]}
    out["wall_s"] = round(float(np.median(walls)), 4)
    out["scc_share"] = round(out["scc_ms"] / max(out["total_ms"], 1e-9), 3)
    return out


def ref_time(A):
    from oracle import oracle as orc
    if not orc.ref_available():
        return {"ref": "oracle/_ref not built"}
    from test_dm_host import _ref_bind
    R = _ref_bind(orc)
    a = orc._ref_to(orc.CSR(A.n, A.m, A.p, A.j, A.x, PRIME))
    saved = orc._silence()
    t0 = time.perf_counter()
    try:
        ptr = R.spasm_dulmage_mendelsohn(a)
    finally:
        el = time.perf_counter() - t0
        orc._unsilence(saved)
    R.spasm_dm_free(ptr)
    R.spasm_csr_free(a)
    return {"ref_s": round(el, 3), "ref": "measured, 1 run, single-threaded, per-row fprintf (to /dev/null) inside"}


def scipy_time(A):
    try:
        import scipy.sparse as sp
        from scipy.sparse.csgraph import maximum_bipartite_matching
    except ImportError:
        return {"scipy": "not importable"}
    M = sp.csr_matrix((np.ones(A.nnz, np.int8), A.j, A.p), shape=(A.n, A.m))
    t0 = time.perf_counter()
    side = "column" if A.n >= A.m else "row"
    size = int(np.count_nonzero(maximum_bipartite_matching(M, perm_type=side) >= 0))
    return {"scipy_hk_s": round(time.perf_counter() - t0, 3), "scipy_size": size}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="mk13.b5,mk13.b5^T,mk14.b4,mk15.b4,gen2M,chain200k")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-ref", action="store_true")
    ap.add_argument("--no-scipy", action="store_true", help="skip scipy's Hopcroft-Karp (minutes on the generated 2 M-row matrix)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dm_bench_dm.json"))
    args = ap.parse_args()
    if spasm_amd.device_count() < 1:
        raise SystemExit("bench_dm.py needs a GPU")
    rows = []
    for name in args.workloads.split(","):
        A, src = matrix(name)
        row = {"workload": name, "source": src, "n": A.n, "m": A.m, "nnz": A.nnz}
        row.update(gpu_times(A, args.reps))
        if not args.no_ref:
            row.update(ref_time(A))
        if not args.no_scipy:
            row.update(scipy_time(A))
        print(json.dumps(row), file=sys.stderr, flush=True)
        rows.append(row)
    out = {"bench": "dm", "reps": args.reps, "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
