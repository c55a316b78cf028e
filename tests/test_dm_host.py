"""Maximum matching, Dulmage-Mendelsohn and strongly connected components on the host side: what the compiled reference returns
on the suite's 32 matrices and their transposes (tests/golden/reference/dm.npz: the matching size, rr, cc, nb and the canonical
partition of tests/dm_cases.py), the checker pinned against those results, the generators against the reference, the exported
symbols, the struct layout, the reference's tools/dm.c linked through the facade, and the Python entry points' refusals.  The
GPU side is tests/test_gpu_dm.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dm_cases
from conftest import ALL_TEST_MATRICES, ROOT, matrix_path, reference_vectors

import spasm_amd
from spasm_amd.matrix import CDm

PRIME = 42013
REF_TREE = "/root/reference"


# ---- the compiled reference (oracle/_ref) ----
def _ref_bind(oracle):
    R = oracle.ref()
    pc = C.POINTER(oracle._RefCsr)
    R.spasm_dulmage_mendelsohn.restype = C.POINTER(CDm)
    R.spasm_dulmage_mendelsohn.argtypes = [pc]
    R.spasm_strongly_connected_components.restype = C.POINTER(CDm)
    R.spasm_strongly_connected_components.argtypes = [pc]
    R.spasm_maximum_matching.restype = C.c_int
    R.spasm_maximum_matching.argtypes = [pc, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    R.spasm_dm_free.argtypes = [C.POINTER(CDm)]
    return R


class _Dm:
    def __init__(self, ptr, n, m):
        s = ptr.contents
        self.nb = int(s.nb)
        self.p = np.ctypeslib.as_array(s.p, shape=(n,)).copy() if n else np.zeros(0, np.int32)
        self.q = np.ctypeslib.as_array(s.q, shape=(m,)).copy() if m else np.zeros(0, np.int32)
        k = self.nb + 1 if self.nb > 0 else 0
        self.r = np.ctypeslib.as_array(s.r, shape=(k,)).copy() if k else np.zeros(0, np.int32)
        self.c = np.ctypeslib.as_array(s.c, shape=(k,)).copy() if k else np.zeros(0, np.int32)
        self.rr, self.cc = np.array(list(s.rr), np.int32), np.array(list(s.cc), np.int32)


def ref_dm(oracle, A):
    """the reference's spasm_dulmage_mendelsohn and spasm_maximum_matching on A: (dm, size)"""
    R = _ref_bind(oracle)
    a = oracle._ref_to(A)
    saved = oracle._silence()
    try:
        ptr = R.spasm_dulmage_mendelsohn(a)
        jm = np.zeros(max(A.n, 1), np.int32)
        im = np.zeros(max(A.m, 1), np.int32)
        if A.n <= A.m:
            size = R.spasm_maximum_matching(a, jm.ctypes.data_as(C.POINTER(C.c_int)), im.ctypes.data_as(C.POINTER(C.c_int)))
        else:
            t = oracle._ref_to(dm_cases.transpose_of(A, oracle.CSR))
            size = R.spasm_maximum_matching(t, im.ctypes.data_as(C.POINTER(C.c_int)), jm.ctypes.data_as(C.POINTER(C.c_int)))
            R.spasm_csr_free(t)
    finally:
        oracle._unsilence(saved)
    dm = _Dm(ptr, A.n, A.m)
    R.spasm_dm_free(ptr)
    R.spasm_csr_free(a)
    return dm, int(size)


def ref_scc(oracle, A):
    R = _ref_bind(oracle)
    a = oracle._ref_to(A)
    ptr = R.spasm_strongly_connected_components(a)
    dm = _Dm(ptr, A.n, A.n)
    R.spasm_dm_free(ptr)
    R.spasm_csr_free(a)
    return dm


def scc_canonical(dm):
    """the set of blocks of a strongly connected decomposition (each sorted, blocks sorted by their first vertex)"""
    blocks = sorted((np.sort(dm.p[dm.r[k]:dm.r[k + 1]]) for k in range(dm.nb)), key=lambda b: int(b[0]))
    return {"verts": np.concatenate(blocks + [np.zeros(0, np.int32)]).astype(np.int32),
            "ptr": np.cumsum([0] + [len(b) for b in blocks]).astype(np.int32)}


def dm_case_names():
    return [name + t for name in ALL_TEST_MATRICES for t in ("", "^T")]


def load_case(oracle, case, cls=None):
    """a case of the dm family as cls (oracle.CSR by default): '<matrix>' or '<matrix>^T'"""
    name, tr = (case[:-2], True) if case.endswith("^T") else (case, False)
    A = oracle.load_sms(matrix_path(name), PRIME)
    if tr:
        A = dm_cases.transpose_of(A, oracle.CSR)
    if cls is not None:
        A = cls(A.n, A.m, A.p, A.j, A.x, PRIME)
    return A


def stored_dm(oracle, case):
    """the reference's result for a case of the dm family (recomputed and compared where oracle/_ref exists)"""
    def live():
        A = load_case(oracle, case)
        dm, size = ref_dm(oracle, A)
        out = {"size": np.array([size], np.int32), "rr": dm.rr, "cc": dm.cc, "nb": np.array([dm.nb], np.int32)}
        out.update(dm_cases.canonical(dm, A.n, A.m))
        return out
    return reference_vectors(oracle, "dm", case, live)


def stored_scc(oracle, name):
    def live():
        A = oracle.load_sms(matrix_path(name), PRIME)
        dm = ref_scc(oracle, A)
        out = {"nb": np.array([dm.nb], np.int32)}
        out.update(scc_canonical(dm))
        return out
    return reference_vectors(oracle, "dm", "scc:" + name, live)


def square_matrices(oracle):
    out = []
    for name in ALL_TEST_MATRICES:
        A = oracle.load_sms(matrix_path(name), PRIME)
        if A.n == A.m:
            out.append(name)
    return out


# ---- stored reference vectors ----
@pytest.mark.parametrize("case", dm_case_names())
def test_reference_dm_vectors_are_consistent(oracle, case):
    """the stored (or recomputed) reference result: the canonical sets partition the rows and columns with the sizes rr / cc say,
    the structural rank is rr[2] + cc[4] - cc[3], and the fine blocks cover H, S and V"""
    A = load_case(oracle, case)
    d = stored_dm(oracle, case)
    rr, cc, size = [int(v) for v in d["rr"]], [int(v) for v in d["cc"]], int(d["size"][0])
    assert size == rr[2] + cc[4] - cc[3] == rr[3]
    assert [len(d[k]) for k in ("R1", "R2", "R03")] == [rr[1], rr[2] - rr[1], A.n - rr[2]]
    assert [len(d[k]) for k in ("C01", "C2", "C3")] == [cc[2], cc[3] - cc[2], A.m - cc[3]]
    assert np.array_equal(np.sort(np.concatenate([d["R1"], d["R2"], d["R03"]])), np.arange(A.n))
    assert np.array_equal(np.sort(np.concatenate([d["C01"], d["C2"], d["C3"]])), np.arange(A.m))
    assert np.array_equal(np.sort(d["fine_rows"]), np.arange(A.n)) and np.array_equal(np.sort(d["fine_cols"]), np.arange(A.m))


@pytest.mark.parametrize("case", dm_case_names())
def test_checker_accepts_the_reference(oracle, case):
    """check_dm on the reference's own decomposition: the checker is pinned against the reference (needs oracle/_ref; where it is
    absent the stored canonical form is checked against the checker's König bound instead)"""
    A = load_case(oracle, case)
    d = stored_dm(oracle, case)
    if oracle.ref_available():
        dm, size = ref_dm(oracle, A)
        if dm.nb == 0:                                  # S empty: the reference leaves its workspace in r and c
            dm.nb, dm.r, dm.c = 2, np.array([0, dm.rr[1], A.n]), np.array([0, dm.cc[2], A.m])
        dm_cases.check_dm(A, dm, size)
        assert dm_cases.same_canonical(dm_cases.canonical(dm, A.n, A.m), d)
    # the stored sets alone: R1 u R2 u C3 covers every entry of A and has the size of the matching
    rows, cols = dm_cases._coo(A)
    in_cover = np.zeros(A.n, bool)
    in_cover[np.concatenate([d["R1"], d["R2"]])] = True
    c3 = np.zeros(A.m, bool)
    c3[d["C3"]] = True
    assert np.all(in_cover[rows] | c3[cols])
    assert len(d["R1"]) + len(d["R2"]) + len(d["C3"]) == int(d["size"][0])


def test_checker_refuses_broken_decompositions(oracle):
    A = load_case(oracle, "dm.sms")
    dm, size = ref_dm(oracle, A) if oracle.ref_available() else (None, None)
    if dm is None:
        pytest.skip("oracle/_ref not built")
    dm_cases.check_dm(A, dm, size)
    with pytest.raises(AssertionError):
        dm_cases.check_dm(A, dm, size + 1)
    bad = _Dm.__new__(_Dm)
    bad.__dict__.update({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in dm.__dict__.items()})
    bad.p[[0, -1]] = bad.p[[-1, 0]]
    with pytest.raises(AssertionError):
        dm_cases.check_dm(A, bad, size)


def test_scc_reference_vectors(oracle):
    names = square_matrices(oracle)
    assert "scc.sms" in names and "mat364.sms" in names
    for name in names:
        A = oracle.load_sms(matrix_path(name), PRIME)
        d = stored_scc(oracle, name)
        assert np.array_equal(np.sort(d["verts"]), np.arange(A.n))
        assert len(d["ptr"]) == int(d["nb"][0]) + 1


@pytest.mark.parametrize("name", ["scc.sms", "scc2.sms", "scc3.sms", "mat364.sms", "t1.sms", "dm2.sms", "trefethen_500.sms"])
def test_host_scc_matches_the_reference(oracle, name):
    """spasm_hip_strongly_connected_components is host code: the same blocks as the reference, in a block upper triangular order"""
    A = oracle.load_sms(matrix_path(name), PRIME)
    if A.n != A.m:
        pytest.skip("not square")
    ours = spasm_amd.strongly_connected_components(spasm_amd.Csr(A.n, A.m, A.p, A.j, A.x, PRIME))
    assert np.array_equal(ours.p, ours.q) and np.array_equal(ours.r, ours.c) and ours.nb == len(ours.r) - 1
    got = scc_canonical(ours)
    want = stored_scc(oracle, name)
    assert np.array_equal(got["verts"], want["verts"]) and np.array_equal(got["ptr"], want["ptr"])
    rows, cols = dm_cases._coo(A)
    pinv = np.empty(A.n, np.int64)
    pinv[ours.p] = np.arange(A.n)
    blk = np.searchsorted(ours.r, pinv[rows], side="right") - 1
    assert np.all(pinv[cols] >= ours.r[blk])


def test_permute_and_pinv(oracle):
    A = oracle.load_sms(matrix_path("mat364.sms"), PRIME)
    B = spasm_amd.Csr(A.n, A.m, A.p, A.j, A.x, PRIME)
    rng = np.random.default_rng(3)
    p, q = rng.permutation(A.n).astype(np.int32), rng.permutation(A.m).astype(np.int32)
    qinv = np.argsort(q).astype(np.int32)
    C_ = spasm_amd.permute(B, p, qinv)
    dense = np.zeros((A.n, A.m), np.int64)
    rows, cols = dm_cases._coo(A)
    dense[rows, cols] = A.x
    got = np.zeros_like(dense)
    r2, c2 = dm_cases._coo(C_)
    got[r2, c2] = C_.x
    assert np.array_equal(got, dense[p][:, q])
    with pytest.raises(ValueError):
        spasm_amd.permute(B, p[:-1], qinv)
    with pytest.raises(ValueError):
        spasm_amd.permute(B, np.zeros(A.n, np.int32), qinv)


# ---- the generators against the reference ----
@pytest.mark.parametrize("seed", range(4))
def test_generators_match_the_reference(oracle, seed):
    if not oracle.ref_available():
        pytest.skip("oracle/_ref not built")
    rng = np.random.default_rng(100 + seed)
    sizes = [int(s) for s in rng.integers(1, 9, 12)]
    for h, v in ((5, 4), (0, 3), (6, 0), (0, 0)):
        K = dm_cases.generate(oracle.CSR, PRIME, h, sizes, v, seed=seed)
        dm, size = ref_dm(oracle, K.A)
        assert size == K.size
        if dm.nb == 0:
            dm.nb, dm.r, dm.c = 2, np.array([0, dm.rr[1], K.A.n]), np.array([0, dm.cc[2], K.A.m])
        dm_cases.check_dm(K.A, dm, size)
        assert dm_cases.same_canonical(dm_cases.canonical(dm, K.A.n, K.A.m), K.canonical())
    K = dm_cases.chain(oracle.CSR, PRIME, 300)
    dm, size = ref_dm(oracle, K.A)
    assert size == 300
    assert dm_cases.same_canonical(dm_cases.canonical(dm, 300, 300), K.canonical())


# ---- ABI ----
def test_dm_symbols_are_exported():
    out = subprocess.run(["nm", "-D", "--defined-only", spasm_amd.LIB_PATH], check=True, capture_output=True, text=True).stdout
    names = {line.split()[-1] for line in out.splitlines()}
    for s in ("spasm_hip_dm_alloc", "spasm_hip_dm_free", "spasm_hip_maximum_matching", "spasm_hip_structural_rank",
              "spasm_hip_dulmage_mendelsohn", "spasm_hip_strongly_connected_components", "spasm_hip_pinv", "spasm_hip_permute",
              "spasm_hip_dm_stats"):
        assert s in names, s
    facade = os.path.join(os.path.dirname(spasm_amd.LIB_PATH), "libspasm_hip_facade.so")
    out = subprocess.run(["nm", "-D", "--defined-only", facade], check=True, capture_output=True, text=True).stdout
    names = {line.split()[-1] for line in out.splitlines()}
    assert {"spasm_maximum_matching", "spasm_dulmage_mendelsohn", "spasm_strongly_connected_components",
            "spasm_structural_rank"} <= names
    shim = open(os.path.join(ROOT, "include", "spasm_hip_shim.h")).read()
    for s in ("spasm_maximum_matching", "spasm_structural_rank", "spasm_dulmage_mendelsohn", "spasm_strongly_connected_components",
              "spasm_dm_alloc", "spasm_dm_free", "spasm_pinv", "spasm_permute"):
        assert "#define %-29s spasm_hip_%s" % (s, s[len("spasm_"):]) in shim or "#define %s spasm_hip_%s" % (s, s[len("spasm_"):]) in shim, s


def test_dm_struct_layout(tmp_path):
    """struct spasm_dm of include/spasm_hip.h: offsets and size as ctypes sees them"""
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "spasm_hip.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", offsetof(struct spasm_dm, p), offsetof(struct spasm_dm, q),'
                   ' offsetof(struct spasm_dm, r), offsetof(struct spasm_dm, c), offsetof(struct spasm_dm, nb),'
                   ' offsetof(struct spasm_dm, rr), offsetof(struct spasm_dm, cc), sizeof(struct spasm_dm));\nreturn 0; }\n')
    exe = str(tmp_path / "layout")
    subprocess.run(["gcc", "-std=gnu99", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe], check=True, capture_output=True)
    got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    want = [getattr(CDm, f).offset for f in ("p", "q", "r", "c", "nb", "rr", "cc")] + [C.sizeof(CDm)]
    assert got == want


def test_dm_alloc_and_free_sizes():
    L = spasm_amd.lib()
    P = L.spasm_hip_dm_alloc(5, 7)
    s = P.contents
    assert s.nb == 0 and list(s.rr) == [0] * 5 and list(s.cc) == [0] * 5
    for k in range(5 + 6):
        s.r[k] = k
    for k in range(7 + 6):
        s.c[k] = k
    L.spasm_hip_dm_free(P)


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF_TREE, "tools")), reason="the reference tree is not on this machine")
def test_reference_dm_c_links_against_the_facade(tmp_path):
    """the reference's own tools/dm.c, unmodified, against the facade (spasm_dulmage_mendelsohn from the GPU library) and the
    reference's library (the rest): every spasm_* symbol resolves"""
    ref_lib_dir = os.path.join(ROOT, "oracle", "_ref")
    if not os.path.exists(os.path.join(ref_lib_dir, "libspasm_ref.so")):
        pytest.skip("oracle/_ref/libspasm_ref.so not built")
    hip_dir = os.path.dirname(spasm_amd.LIB_PATH)
    exe = str(tmp_path / "ref_dm_facade")
    subprocess.run(["gcc", "-O2", "-std=gnu99", "-I" + os.path.join(REF_TREE, "src"), os.path.join(REF_TREE, "tools", "dm.c"),
                    "-o", exe, "-L" + hip_dir, "-lspasm_hip_facade", "-L" + ref_lib_dir, "-lspasm_ref", "-lm", "-fopenmp",
                    "-Wl,-rpath," + hip_dir, "-Wl,-rpath," + ref_lib_dir, "-Wl,--no-undefined"], check=True, capture_output=True)
    need = {line.split()[-1] for line in subprocess.run(["nm", "-D", "--undefined-only", exe], check=True, capture_output=True,
                                                         text=True).stdout.splitlines() if "spasm" in line}
    facade = os.path.join(hip_dir, "libspasm_hip_facade.so")
    have_facade = {line.split()[-1] for line in subprocess.run(["nm", "-D", "--defined-only", facade], check=True, capture_output=True,
                                                               text=True).stdout.splitlines()}
    have_ref = {line.split()[-1] for line in subprocess.run(["nm", "-D", "--defined-only", os.path.join(ref_lib_dir, "libspasm_ref.so")],
                                                            check=True, capture_output=True, text=True).stdout.splitlines()}
    assert "spasm_dulmage_mendelsohn" in need and "spasm_dulmage_mendelsohn" in have_facade
    assert need <= have_facade | have_ref, need - have_facade - have_ref
    assert "not found" not in subprocess.run(["ldd", exe], check=True, capture_output=True, text=True).stdout


# ---- Python entry points ----
def test_python_entry_points_refuse_before_c(oracle):
    A = oracle.load_sms(matrix_path("dm.sms"), PRIME)
    B = spasm_amd.Csr(A.n, A.m, A.p, A.j, A.x, PRIME)
    bad_col = spasm_amd.Csr(A.n, A.m, A.p, np.where(np.arange(len(A.j)) == 0, A.m, A.j), A.x, PRIME)
    bad_ptr = spasm_amd.Csr(A.n, A.m, np.concatenate([[1], A.p[1:]]), A.j, A.x, PRIME)
    for fn in (spasm_amd.maximum_matching, spasm_amd.structural_rank, spasm_amd.dulmage_mendelsohn,
               spasm_amd.strongly_connected_components):
        for bad in (bad_col, bad_ptr, "not a matrix"):
            with pytest.raises(ValueError):
                fn(bad)
    with pytest.raises(ValueError):
        spasm_amd.strongly_connected_components(spasm_amd.Csr(2, 3, [0, 1, 2], [0, 2], [1, 1], PRIME))
    if spasm_amd.device_count() == 0:
        for fn in (spasm_amd.maximum_matching, spasm_amd.structural_rank, spasm_amd.dulmage_mendelsohn):
            with pytest.raises(RuntimeError):
                fn(B)


def test_no_oracle_word_in_the_package():
    for d, _, files in os.walk(os.path.join(ROOT, "spasm_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".cpp", ".h", ".c")):
                assert "oracle" not in open(os.path.join(d, f)).read().lower(), f
