"""Maximum matching and the Dulmage-Mendelsohn decomposition on the GPU (spasm_amd/csrc/matching.hip, host_dm.cpp): every
result passes tests/dm_cases.check_dm (which proves the matching maximum and the decomposition finest), and its canonical form
equals the reference's, stored in tests/golden/reference/dm.npz (tests/test_dm_host.py), on the suite's matrices, their
transposes and random permutations; generated matrices with a known answer up to about 2 M rows; the greedy-defeating chain;
mk13.b5 in both orientations; tools/dm."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import dm_cases
from conftest import ROOT, matrix_path
from test_dm_host import PRIME, dm_case_names, load_case, scc_canonical, square_matrices, stored_dm, stored_scc

import spasm_amd

pytestmark = pytest.mark.gpu

TOOL = os.path.join(ROOT, "tools", "dm")


def as_csr(A):
    return spasm_amd.Csr(A.n, A.m, A.p, A.j, A.x, PRIME)


def run_dm(A):
    """dulmage_mendelsohn and maximum_matching of A (a spasm_amd.Csr), both checked; returns (dm, size)"""
    dm = spasm_amd.dulmage_mendelsohn(A)
    jm, im, size = spasm_amd.maximum_matching(A)
    assert np.count_nonzero(jm >= 0) == np.count_nonzero(im >= 0) == size
    rows = np.flatnonzero(jm >= 0)
    assert np.array_equal(im[jm[rows]], rows), "jmatch and imatch disagree"
    for i in rows.tolist():
        assert jm[i] in A.j[A.p[i]:A.p[i + 1]], "a matched pair is not an entry of A"
    assert spasm_amd.structural_rank(A) == size
    dm_cases.check_dm(A, dm, size)
    return dm, size


@pytest.mark.parametrize("case", dm_case_names())
def test_dm_matches_the_reference(oracle, case):
    """A and its transpose (as cases), plus three random row and column permutations of each: check_dm, the stored size and the
    stored canonical form (the permutations mapped back)"""
    want = stored_dm(oracle, case)
    A = load_case(oracle, case, spasm_amd.Csr)
    dm, size = run_dm(A)
    assert size == int(want["size"][0])
    assert dm_cases.same_canonical(dm_cases.canonical(dm, A.n, A.m), want)
    rng = np.random.default_rng(len(case))
    for _ in range(3):
        p, q = rng.permutation(A.n), rng.permutation(A.m)
        B = dm_cases.permuted_pattern(A, p, q, spasm_amd.Csr, PRIME)
        dmb, sizeb = run_dm(B)
        assert sizeb == size
        back = dm_cases._Fake.__new__(dm_cases._Fake)
        back.p, back.q, back.r, back.c, back.nb, back.rr, back.cc = p[dmb.p], q[dmb.q], dmb.r, dmb.c, dmb.nb, dmb.rr, dmb.cc
        assert dm_cases.same_canonical(dm_cases.canonical(back, A.n, A.m), want)


def test_scc_matches_the_reference(oracle):
    for name in square_matrices(oracle):
        A = as_csr(oracle.load_sms(matrix_path(name), PRIME))
        ours = spasm_amd.strongly_connected_components(A)
        got, want = scc_canonical(ours), stored_scc(oracle, name)
        assert np.array_equal(got["verts"], want["verts"]) and np.array_equal(got["ptr"], want["ptr"]), name


def test_two_calls_are_identical(oracle):
    K = dm_cases.generate(spasm_amd.Csr, PRIME, 3000, list(np.random.default_rng(5).integers(1, 40, 800)), 2000, extra=3, seed=5)
    a, b = spasm_amd.dulmage_mendelsohn(K.A), spasm_amd.dulmage_mendelsohn(K.A)
    for f in ("p", "q", "r", "c", "rr", "cc"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f
    j1, i1, _ = spasm_amd.maximum_matching(K.A)
    j2, i2, _ = spasm_amd.maximum_matching(K.A)
    assert np.array_equal(j1, j2) and np.array_equal(i1, i2)


@pytest.mark.parametrize("shape", [(0, 0), (0, 5), (5, 0), (4, 6), (1, 7), (7, 1)])
def test_edge_cases(shape):
    n, m = shape
    empty = spasm_amd.Csr(n, m, np.zeros(n + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32), PRIME)
    dm, size = run_dm(empty)
    assert size == 0 and dm.nb == 2 and list(dm.r) == [0, 0, n] and list(dm.c) == [0, m, m]     # all of A is R0 x C0
    if n and m:
        full = dm_cases.csr_of(spasm_amd.Csr, n, m, np.repeat(np.arange(n), m), np.tile(np.arange(m), n), PRIME)
        dm, size = run_dm(full)
        assert size == min(n, m)


@pytest.mark.parametrize("name", ["empty.sms", "void.sms"])
def test_empty_and_void_matrices(oracle, name):
    A = as_csr(oracle.load_sms(matrix_path(name), PRIME))
    run_dm(A)


@pytest.mark.parametrize("h_rows,n_blocks,v_cols,seed", [(20000, 3000, 15000, 1), (0, 5000, 0, 2), (600000, 6000, 450000, 3)])
def test_generated_with_known_answer(h_rows, n_blocks, v_cols, seed):
    rng = np.random.default_rng(seed)
    sizes = [int(s) for s in rng.choice([1, 1, 2, 3, 5, 8, 40, 200], n_blocks)]
    K = dm_cases.generate(spasm_amd.Csr, PRIME, h_rows, sizes, v_cols, extra=3, seed=seed)
    t = time.time()
    dm = spasm_amd.dulmage_mendelsohn(K.A)
    el = time.time() - t
    st = spasm_amd.dm_stats()
    dm_cases.check_dm(K.A, dm, K.size)
    assert dm.nb == n_blocks + 2
    assert dm_cases.same_canonical(dm_cases.canonical(dm, K.A.n, K.A.m), K.canonical())
    print("generated %d x %d (%d entries, %d blocks): %.3f s; stats %s" % (K.A.n, K.A.m, K.A.nnz, n_blocks, el, st))


def test_chain_defeats_greedy_and_finishes():
    n = 50000
    K = dm_cases.chain(spasm_amd.Csr, PRIME, n)
    t = time.time()
    dm = spasm_amd.dulmage_mendelsohn(K.A)
    el = time.time() - t
    st = spasm_amd.dm_stats()
    dm_cases.check_dm(K.A, dm, n)
    assert dm.nb == n + 2 and st["greedy_size"] == n - 1 and st["size"] == n
    print("chain %d: %.3f s, %d phases, %d levels (%d inside one workgroup); stats %s" % (n, el, st["phases"], st["levels"],
                                                                                         st["small_levels"], st))


# mk13.b5 (tools/workloads.py regenerates it): the compiled reference's spasm_dulmage_mendelsohn and spasm_maximum_matching on
# the CPU, checked with check_dm, canonical() and digest() of tests/dm_cases.py (the reference itself is not on the GPU machines):
#   tall (270270 x 135135) and wide (135135 x 270270)
MK13_B5 = {      # (the reference returns nb = 0 here, S being empty: nb = 2 is ours)
    True: {"size": 135135, "rr": [0, 0, 0, 135135, 270270], "cc": [0, 0, 0, 0, 135135], "nb": 2,
           "digest": "d9c6153fb7568332f4e0f5b56493bac88ba92a2c583d05cb83ce78287549a86f"},
    False: {"size": 135135, "rr": [0, 135135, 135135, 135135, 135135], "cc": [0, 135135, 270270, 270270, 270270], "nb": 2,
            "digest": "8b2d54941a3f4083be50ab785cce886000268c3b27416d62444b55bae3780d70"},
}


@pytest.mark.parametrize("tall", [True, False])
def test_mk13_b5(tall):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import workloads
    A, _ = workloads.load_matrix("mk13.b5", tall=tall)
    t = time.time()
    dm = spasm_amd.dulmage_mendelsohn(A)
    el = time.time() - t
    st = spasm_amd.dm_stats()
    size = int(st["size"])
    dm_cases.check_dm(A, dm, size)
    want = MK13_B5[tall]
    assert size == want["size"] and list(dm.rr) == want["rr"] and list(dm.cc) == want["cc"] and dm.nb == want["nb"]
    assert dm_cases.digest(dm_cases.canonical(dm, A.n, A.m)) == want["digest"]
    try:
        import scipy.sparse as sp
        from scipy.sparse.csgraph import maximum_bipartite_matching
    except ImportError:
        sp = None
    if sp is not None:
        M = sp.csr_matrix((np.ones(A.nnz, np.int8), A.j, A.p), shape=(A.n, A.m))
        assert np.count_nonzero(maximum_bipartite_matching(M, perm_type="column") >= 0) == size
    print("mk13.b5 %s: %.3f s; stats %s" % ("tall" if tall else "wide", el, st))


def _verbose_lines(d, n, m):
    """what tools/dm --verbose prints for a stored reference result (the SCC lines as a multiset)"""
    rr, cc = [int(v) for v in d["rr"]], [int(v) for v in d["cc"]]
    out = ["structural rank = %d" % (rr[2] + cc[4] - cc[3])]
    if rr[1] > 0 and cc[2] > 0:
        out.append("*) H (%d x %d)" % (rr[1], cc[2]))
    s_n, s_m = rr[2] - rr[1], cc[3] - cc[2]
    if s_n > 0 and s_m > 0:
        out.append("*) S (%d x %d) : " % (s_n, s_m))
        R2 = set(d["R2"].tolist())
        rp = d["fine_rows_ptr"]
        sizes = [int(rp[k + 1] - rp[k]) for k in range(len(rp) - 1) if rp[k + 1] > rp[k] and int(d["fine_rows"][rp[k]]) in R2]
        out += ["    *) SCC of size %d" % s for s in sizes if s > 1]
        if sizes.count(1):
            out.append("    -> plus %d SCC of size 1" % sizes.count(1))
    if n - rr[2] > 0 and cc[4] - cc[3] > 0:
        out.append("*) V (%d x %d)" % (n - rr[2], cc[4] - cc[3]))
    return out


@pytest.mark.parametrize("name", ["dm.sms", "dm2.sms", "scc.sms", "scc3.sms", "mat364.sms", "BIOMD0000000424.int.mpl.sms",
                                  "rectangular_h.sms"])
def test_tool_dm(oracle, name):
    A = as_csr(oracle.load_sms(matrix_path(name), PRIME))
    with open(matrix_path(name)) as f:
        v = subprocess.run([TOOL, "--verbose"], stdin=f, capture_output=True, text=True, timeout=120)
    assert v.returncode == 0, v.stderr
    got, want = v.stdout.splitlines(), _verbose_lines(stored_dm(oracle, name), A.n, A.m)
    assert sorted(got) == sorted(want)
    with open(matrix_path(name)) as f:
        p = subprocess.run([TOOL, "--permuted"], stdin=f, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    dm = spasm_amd.dulmage_mendelsohn(A)
    lines = p.stdout.splitlines()
    n, m, _ = lines[0].split()
    assert (int(n), int(m)) == (A.n, A.m)
    got = sorted(tuple(int(t) for t in ln.split()[:2]) for ln in lines[1:] if ln.split() != ["0", "0", "0"])
    B = spasm_amd.permute(A, dm.p, np.argsort(dm.q).astype(np.int32))
    want = sorted((i + 1, int(B.j[e]) + 1) for i in range(B.n) for e in range(B.p[i], B.p[i + 1]))
    assert got == want
    with open(matrix_path(name)) as f:
        t = subprocess.run([TOOL, "--tabulated"], stdin=f, capture_output=True, text=True, timeout=120)
    assert t.returncode == 0 and t.stdout == ""
    with open(matrix_path(name)) as f:
        i = subprocess.run([TOOL, "--image", "1"], stdin=f, capture_output=True, text=True, timeout=120)
    assert i.returncode == 2 and "PNM output is not supported" in i.stderr
