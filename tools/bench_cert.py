"""Timing of rank certificates on the GPU (spasm_amd.certificate_rank_create / _verify, factorization_verify, x.A) against the
compiled reference's spasm_certificate_rank_create / _verify on the host.

    python tools/bench_cert.py [--workloads mk13.b5,mk15.b4] [--reps 3] [--no-ref]

For every generated workload: echelonize with opts.L on the GPU, then --reps runs (after one warm-up) of: the three
factorization checks of tools/rank (one batched call), create, verify, and x.A alone for k = 1, 2, 3 (device ms of the product
kernel and of building the column-major image, algorithmic bytes and GB/s).  The reference's create and verify run once on the
same factorization where oracle/_ref exists (single-threaded: its spasm_solve and spasm_xApy loops have no parallel region).
One JSON line on stdout."""
import argparse
import ctypes as C
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

SEEDS = (42, 1337, 21011984)


def med(f, reps):
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def ref_times(A, hash, F):
    from oracle import oracle as orc
    if not orc.ref_available():
        return {"ref": "oracle/_ref not built"}
    from test_cert_host import ref_create, ref_verify
    Cv = lambda M: orc.CSR(M.n, M.m, M.p, M.j, M.x, M.prime)      # noqa: E731
    t0 = time.perf_counter()
    cert = ref_create(orc, Cv(A), hash, Cv(F.U), F.qinv, Cv(F.L), F.Lp)
    t1 = time.perf_counter()
    ok = ref_verify(orc, Cv(A), hash, cert)
    t2 = time.perf_counter()
    return {"ref_create_s": round(t1 - t0, 3), "ref_verify_s": round(t2 - t1, 3), "ref_verify_ok": ok, "ref": "measured, 1 run"}, cert


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="mk13.b5,mk15.b4")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-ref", action="store_true")
    args = ap.parse_args()
    spasm_amd.lib()
    if spasm_amd.device_count() < 1:
        raise SystemExit("bench_cert.py needs an MI355X")
    out = {"metric": "rank_certificate", "workloads": []}
    for name in args.workloads.split(","):
        A, source = workloads.load_matrix(name)
        o = spasm_amd.default_opts()
        o.L = True
        t0 = time.perf_counter()
        F = spasm_amd.echelonize(A, o)
        w = {"name": name, "source": source, "n": A.n, "m": A.m, "nnz": A.nnz, "rank": F.U.n, "nnz_L": F.L.nnz, "nnz_U": F.U.nnz,
             "echelonize_with_L_s": round(time.perf_counter() - t0, 3)}
        hash = bytes(range(32))
        checks = spasm_amd.factorization_verify(A, F, SEEDS)
        w["factorization_checks"] = checks
        w["factorization_checks_s"] = round(med(lambda: spasm_amd.factorization_verify(A, F, SEEDS), args.reps), 4)
        box = {}
        w["create_s"] = round(med(lambda: box.__setitem__("c", spasm_amd.certificate_rank_create(A, hash, F)), args.reps), 4)
        cert = box["c"]
        w["verify_ok"] = spasm_amd.certificate_rank_verify(A, hash, cert)
        w["verify_s"] = round(med(lambda: spasm_amd.certificate_rank_verify(A, hash, cert), args.reps), 4)
        w["xA"] = []
        rng = np.random.default_rng(1)
        for k in (1, 2, 3):
            X = rng.integers(0, A.prime, (k, A.n), dtype=np.int64)
            runs = []
            for _ in range(args.reps + 1):
                t0 = time.perf_counter()
                spasm_amd.xApy(X, A)
                runs.append((time.perf_counter() - t0, spasm_amd.xApy_stats()))
            runs = sorted(runs[1:], key=lambda r: r[1]["product_ms"])
            wall, st = runs[len(runs) // 2]
            w["xA"].append({"k": k, "wall_s": round(wall, 4), "product_ms": round(st["product_ms"], 4), "image_ms": round(st["image_ms"], 4),
                            "upload_ms": round(st["upload_ms"], 4), "product_bytes": int(st["product_bytes"]),
                            "product_GB_per_s": round(st["product_bytes"] / (st["product_ms"] * 1e-3) / 1e9, 1) if st["product_ms"] > 0 else None,
                            "long_columns": int(st["long_columns"]), "short_columns": int(st["short_columns"])})
        if not args.no_ref:
            r = ref_times(A, hash, F)
            if isinstance(r, tuple):
                info, ref_cert = r
                info["ref_certificate_equal"] = bool(ref_cert == cert)
                w.update(info)
            else:
                w.update(r)
        out["workloads"].append(w)
        print(json.dumps(w), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
