"""Timing of the kernel basis: spasm_hip_kernel (reduced rows downloaded, transposed and assembled on the host) against
spasm_hip_kernel_basis (all of it on the device), the compiled reference's spasm_kernel, and the host transposition against the
device one.

    python tools/bench_kernel.py [--workloads mk12.b3,mk13.b5] [--reps 5] [--no-ref] [--ref-timeout 600] [--out profiles/kernel_bench_kernel.json]

For every generated workload the factor comes from spasm_hip_echelonize in the timing process itself.  ONE timed object per
process: the tool starts a fresh child (this script with --one) for each of
    kernel            (a) spasm_amd.kernel(F)
    kernel_basis      (b) spasm_amd.kernel_basis(F), with the stage split of kernel_stats() of the median run
    transpose_A / transpose_device_A, transpose_R / transpose_device_R      spasm_hip_transpose against spasm_hip_transpose_device
                      on the input matrix and on R = spasm_amd.rref(F)
    ref_kernel        (c) spasm_kernel of oracle/_ref on the same factor (one run, no warm-up; OpenMP on the CPUs of the process)
Every child first asserts (a) == (b) array for array (kernel and kernel_basis only), then one warm-up call and --reps timed calls
with a host clock around calls that end in a download; the median and the spread are reported.  Block cache: the library keeps
freed device blocks between calls, so the timed calls find their blocks cached (the warm-up paid for them); the warm-up call is
reported as first_call_ms.  Times include the Python wrapper's copy of the result.  One JSON document, also written to --out."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

OBJECTS = ["kernel", "kernel_basis", "transpose_A", "transpose_device_A", "transpose_R", "transpose_device_R", "ref_kernel"]


def same(K, want):
    return (K.n, K.m) == (want.n, want.m) and np.array_equal(K.p, want.p) and np.array_equal(K.j, want.j) and np.array_equal(K.x, want.x)


def timed(fn, reps, stats=None):
    t0 = time.perf_counter()
    fn()
    first = time.perf_counter() - t0
    times, extra = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
        extra.append(stats() if stats else None)
    order = np.argsort(times)
    mid = int(order[len(times) // 2])
    out = {"first_call_ms": round(1e3 * first, 3), "median_ms": round(1e3 * times[mid], 3), "min_ms": round(1e3 * min(times), 3),
           "max_ms": round(1e3 * max(times), 3), "reps": reps}
    if stats:
        out["stats_of_the_median_run"] = {k: round(v, 3) for k, v in extra[mid].items()}
    return out


def one(name, what, reps):
    import spasm_amd
    import workloads
    spasm_amd.lib()
    if spasm_amd.device_count() < 1:
        raise SystemExit("bench_kernel.py needs an MI355X")
    A, source = workloads.load_matrix(name)
    F = spasm_amd.echelonize(A)
    out = {"workload": name, "object": what, "source": source, "n": A.n, "m": A.m, "nnz": A.nnz, "rank": F.U.n, "nnz_U": F.U.nnz}
    if what in ("kernel", "kernel_basis"):
        want, K = spasm_amd.kernel(F), spasm_amd.kernel_basis(F)
        assert same(K, want), "spasm_hip_kernel_basis differs from spasm_hip_kernel on %s" % name
        out.update(rows_K=K.n, nnz_K=K.nnz, equal_to_spasm_hip_kernel=True)
        del want, K
        if what == "kernel":
            out.update(timed(lambda: spasm_amd.kernel(F), reps))
        else:
            out.update(timed(lambda: spasm_amd.kernel_basis(F), reps, spasm_amd.kernel_stats))
    elif what.startswith("transpose"):
        M = A if what.endswith("_A") else spasm_amd.rref(F)[0]
        out.update(rows=M.n, columns=M.m, entries=M.nnz)
        if "device" in what:
            T, host = spasm_amd.transpose_device(M), spasm_amd.transpose(M)
            assert same(T, host), "spasm_hip_transpose_device differs from spasm_hip_transpose on %s" % name
            del T, host
            out.update(timed(lambda: spasm_amd.transpose_device(M), reps, spasm_amd.transpose_stats))
        else:
            out.update(timed(lambda: spasm_amd.transpose(M), reps))
    elif what == "ref_kernel":
        import ctypes
        from oracle import oracle as orc
        if not orc.ref_available():
            out["not_measured"] = "oracle/_ref was not built"
        else:
            R = orc.ref()
            threads = spasm_amd.usable_cpus()
            orc.ref_set_threads(threads)
            R.spasm_kernel.restype = ctypes.POINTER(orc._RefCsr)
            R.spasm_kernel.argtypes = [ctypes.POINTER(orc._RefLu)]
            lu, up, q = orc._ref_lu(orc.Fact(orc.CSR(F.U.n, F.U.m, F.U.p, F.U.j, F.U.x, F.U.prime), F.qinv), 0)
            saved = orc._silence()
            t0 = time.perf_counter()
            try:
                k = R.spasm_kernel(ctypes.byref(lu))
            finally:
                orc._unsilence(saved)
            dt = time.perf_counter() - t0
            out.update(one_run_ms=round(1e3 * dt, 3), threads=threads, rows_K=int(k.contents.n), nnz_K=int(k.contents.p[k.contents.n]))
            R.spasm_csr_free(k)
            R.spasm_csr_free(up)
    else:
        raise SystemExit("unknown object %s" % what)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="mk12.b3,mk13.b5")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--objects", default=",".join(OBJECTS))
    ap.add_argument("--no-ref", action="store_true")
    ap.add_argument("--ref-timeout", type=float, default=600.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kernel_bench_kernel.json"))
    ap.add_argument("--one", default=None, help="workload:object -- time this one object in this process (what the children run)")
    args = ap.parse_args()
    if args.reps < 5:
        raise SystemExit("at least 5 timed runs per object")
    if args.one:
        name, what = args.one.split(":")
        return one(name, what, args.reps)
    doc = {"metric": "kernel_basis", "method": "host clock around calls that end in a download; one warm-up, then the median of "
           "%d runs; one timed object per process; block cache warm (first_call_ms is the call that filled it)" % args.reps, "runs": []}
    objects = [o for o in args.objects.split(",") if not (args.no_ref and o == "ref_kernel")]
    env = dict(os.environ, SPASM_HIP_VERBOSE="0")
    for name in args.workloads.split(","):
        for what in objects:
            cmd = [sys.executable, os.path.abspath(__file__), "--one", "%s:%s" % (name, what), "--reps", str(args.reps)]
            try:
                child = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=args.ref_timeout if what == "ref_kernel" else None)
            except subprocess.TimeoutExpired:
                doc["runs"].append({"workload": name, "object": what, "not_measured": "no result within %.0f s" % args.ref_timeout})
                continue
            if child.returncode != 0:
                sys.stderr.write(child.stderr[-3000:])
                raise SystemExit("%s:%s failed with status %d" % (name, what, child.returncode))
            doc["runs"].append(json.loads(child.stdout.strip().splitlines()[-1]))
            sys.stderr.write("%s:%s done\n" % (name, what))
    text = json.dumps(doc, indent=1)
    with open(args.out, "w") as f:
        f.write(text + "\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
