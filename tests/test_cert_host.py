"""Rank certificates (spasm_certificate.c) on the host: what the compiled reference creates on the suite's matrices, stored in
tests/golden/reference/certificate.npz with the reference's own verdicts (the certificate, and six single mutations of it);
the hash-seeded generator and the file hash against the reference's; the text format of save and load.  The GPU side
(create, verify, factorization checks, x.A, the tools) is tests/test_gpu_cert.py."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ALL_TEST_MATRICES, matrix_path, reference_vectors
from test_solve_host import SOLVE_MODULI, oracle_fact

import spasm_amd
from spasm_amd.matrix import CCertificate

_libc = C.CDLL(None)
_libc.fopen.restype = C.c_void_p
_libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
_libc.fclose.argtypes = [C.c_void_p]
_libc.free.argtypes = [C.c_void_p]

MUTATIONS = ("hash byte", "prime", "i out of range", "j out of range", "one x", "one y", "two pivot rows swapped")


def mutate(cert, which, n):
    """the certificate after one mutation (None where it does not apply: too few pivots)"""
    c = cert.copy()
    k = c.r // 2
    p = c.prime
    if which == "hash byte":
        h = bytearray(c.hash)
        h[7] ^= 0x10
        c.hash = bytes(h)
    elif which == "prime":
        c.prime = p + 2
    elif c.r == 0:
        return None
    elif which == "i out of range":
        c.i[k] = n
    elif which == "j out of range":
        c.j[k] = -1
    elif which in ("one x", "one y"):
        v = c.x if which == "one x" else c.y
        w = (int(v[k]) + 1) % p
        v[k] = w - p if w > p // 2 else w
    elif which == "two pivot rows swapped":
        if c.r < 2:
            return None
        c.i[0], c.i[c.r - 1] = c.i[c.r - 1], c.i[0]
    return c


# ---- the compiled reference (oracle/_ref) ----
def _ref_bind(oracle):
    R = oracle.ref()
    pc, pl = C.POINTER(oracle._RefCsr), C.POINTER(oracle._RefLu)
    R.spasm_certificate_rank_create.restype = C.POINTER(CCertificate)
    R.spasm_certificate_rank_create.argtypes = [pc, C.POINTER(C.c_uint8), pl]
    R.spasm_certificate_rank_verify.restype = C.c_bool
    R.spasm_certificate_rank_verify.argtypes = [pc, C.POINTER(C.c_uint8), C.POINTER(CCertificate)]
    R.spasm_rank_certificate_save.argtypes = [C.POINTER(CCertificate), C.c_void_p]
    R.spasm_triplet_load.restype = C.POINTER(oracle._RefTriplet)
    R.spasm_triplet_load.argtypes = [C.c_void_p, C.c_int64, C.c_void_p]
    R.spasm_prng_seed.argtypes = [C.POINTER(C.c_uint8), C.c_int64, C.c_uint32, C.c_void_p]
    return R


def _h(hash):
    return (C.c_uint8 * 32).from_buffer_copy(bytes(hash))


def ref_file_hash(oracle, path, prime):
    R = _ref_bind(oracle)
    f = _libc.fopen(path.encode(), b"r")
    digest = (C.c_uint8 * 32)()
    saved = oracle._silence()
    try:
        T = R.spasm_triplet_load(f, prime, digest)
        R.spasm_triplet_free(T)
    finally:
        oracle._unsilence(saved)
        _libc.fclose(f)
    return bytes(digest)


def ref_create(oracle, A, hash, U, qinv, L, Lp):
    R = _ref_bind(oracle)
    lu, up, q = oracle._ref_lu(oracle.Fact(U, qinv), 0)
    lp = oracle._ref_to(L)
    pp = np.ascontiguousarray(Lp, np.int32).copy() if len(Lp) else np.zeros(1, np.int32)
    lu.L = lp
    lu.p = pp.ctypes.data_as(C.POINTER(C.c_int))
    a = oracle._ref_to(A)
    saved = oracle._silence()
    try:
        c = R.spasm_certificate_rank_create(a, _h(hash), C.byref(lu))
    finally:
        oracle._unsilence(saved)
    cert = spasm_amd.Certificate._of(c.contents)
    for ptr in (c.contents.i, c.contents.j, c.contents.x, c.contents.y):
        _libc.free(C.cast(ptr, C.c_void_p))
    _libc.free(C.cast(c, C.c_void_p))
    for ptr in (a, lp, up):
        R.spasm_csr_free(ptr)
    return cert


def ref_verify(oracle, A, hash, cert):
    R = _ref_bind(oracle)
    a = oracle._ref_to(A)
    c = cert._c()
    try:
        return bool(R.spasm_certificate_rank_verify(a, _h(hash), C.byref(c)))
    finally:
        R.spasm_csr_free(a)


def ref_save_bytes(oracle, cert, path):
    R = _ref_bind(oracle)
    c = cert._c()
    f = _libc.fopen(str(path).encode(), b"w")
    R.spasm_rank_certificate_save(C.byref(c), f)
    _libc.fclose(f)
    with open(path, "rb") as fh:
        return fh.read()


def ref_prng(oracle, seed32, prime, seq, count):
    R = _ref_bind(oracle)
    ctx = C.create_string_buffer(4096)
    R.spasm_prng_seed(_h(seed32), prime, seq, ctx)
    return np.array([R.spasm_prng_ZZp(ctx) for _ in range(count)], np.int32)


# ---- stored vectors ----
def stored_hash(oracle, name):
    want = reference_vectors(oracle, "certificate", "hash|%s" % name,
                             lambda: {"hash": np.frombuffer(ref_file_hash(oracle, matrix_path(name), 42013), np.uint8)})
    return bytes(want["hash"].astype(np.uint8))


def cert_of(d):
    return spasm_amd.Certificate(int(d["r"]), int(d["prime"]), bytes(d["hash"].astype(np.uint8)), d["i"], d["j"], d["x"], d["y"])


def stored_cert_case(oracle, name, p, tmp_dir):
    """(A, hash, (U, qinv, L, Lp), the reference's certificate, {verdicts, saved bytes}) of one stored case"""
    A = oracle.load_sms(matrix_path(name), p)
    hash = stored_hash(oracle, name)
    U, qinv, L, Lp = oracle_fact(oracle, A, False)

    def live():
        cert = ref_create(oracle, A, hash, U, qinv, L, Lp)
        verdicts = [ref_verify(oracle, A, hash, cert)]
        for which in MUTATIONS:
            c = mutate(cert, which, A.n)
            verdicts.append(2 if c is None else int(ref_verify(oracle, A, hash, c)))
        saved = ref_save_bytes(oracle, cert, os.path.join(tmp_dir, "ref.cert"))
        return {"r": np.int64(cert.r), "prime": np.int64(cert.prime), "hash": np.frombuffer(cert.hash, np.uint8), "i": cert.i,
                "j": cert.j, "x": cert.x, "y": cert.y, "verdicts": np.array(verdicts, np.uint8),
                "saved": np.frombuffer(saved, np.uint8)}

    want = reference_vectors(oracle, "certificate", "%s|%d" % (name, p), live)
    return A, hash, (U, qinv, L, Lp), cert_of(want), want


CERT_CASES = [(name, p) for name in ALL_TEST_MATRICES for p in SOLVE_MODULI]


@pytest.mark.parametrize("name,p", CERT_CASES)
def test_stored_certificate_is_the_references(oracle, name, p, tmp_path):
    """the stored certificate has the shape of the factorization, the reference accepts it and refuses every mutation"""
    A, hash, (U, qinv, L, Lp), cert, want = stored_cert_case(oracle, name, p, str(tmp_path))
    assert cert.r == U.n and cert.prime == p and cert.hash == hash
    assert np.array_equal(cert.i, Lp[:U.n])
    assert np.array_equal(cert.j, np.flatnonzero(np.asarray(qinv) >= 0))
    v = want["verdicts"]
    assert v[0] == 1, "the reference refuses its own certificate"
    for t, which in enumerate(MUTATIONS):
        if mutate(cert, which, A.n) is None:
            assert v[1 + t] == 2, which
        elif which in ("hash byte", "prime", "i out of range", "j out of range"):
            assert v[1 + t] == 0, which                       # refused before any product
        else:
            assert v[1 + t] in (0, 1), which                  # (over a tiny field a swap can survive: only the GPU must agree)
    if oracle.ref_available():
        assert ref_verify(oracle, A, hash, cert)


@pytest.mark.parametrize("name,p", CERT_CASES[::7])
def test_save_is_byte_identical_and_load_round_trips(oracle, name, p, tmp_path):
    A, hash, fact, cert, want = stored_cert_case(oracle, name, p, str(tmp_path))
    path = str(tmp_path / "ours.cert")
    cert.save(path)
    with open(path, "rb") as fh:
        ours = fh.read()
    assert ours == bytes(want["saved"].astype(np.uint8))
    back = spasm_amd.Certificate.load(path)
    assert back == cert                                       # the j line goes to j (the reference reads it into i again)
    path2 = str(tmp_path / "again.cert")
    back.save(path2)
    with open(path2, "rb") as fh:
        assert fh.read() == ours


def test_load_refuses_a_short_file(tmp_path):
    path = str(tmp_path / "short.cert")
    with open(path, "w") as fh:
        fh.write("3\n257\n" + "ab" * 32 + "\n0 1 2 \n0 1 2 \n5 6 \n")
    with pytest.raises(ValueError):
        spasm_amd.Certificate.load(path)


@pytest.mark.parametrize("name", ALL_TEST_MATRICES)
def test_file_hash_is_the_references(oracle, name):
    A, h = spasm_amd.load(matrix_path(name), 42013, with_hash=True)
    assert h == stored_hash(oracle, name)
    B = spasm_amd.load(matrix_path(name), 42013)
    assert (B.n, B.m) == (A.n, A.m) and np.array_equal(B.p, A.p) and np.array_equal(B.j, A.j) and np.array_equal(B.x, A.x)


@pytest.mark.parametrize("p", SOLVE_MODULI)
@pytest.mark.parametrize("seq", [0, 3])
def test_hash_seeded_prng_is_the_references(oracle, p, seq):
    seed = bytes(range(7, 7 + 32 * 5, 5))
    count = 300
    want = reference_vectors(oracle, "certificate", "prng|%d|%d" % (p, seq), lambda: {"values": ref_prng(oracle, seed, p, seq, count)})
    L = spasm_amd.lib()
    out = np.zeros(count, np.int32)
    L.spasm_hip_debug_prng_hash(_h(seed), p, seq, count, out.ctypes.data_as(C.POINTER(C.c_int32)))
    assert np.array_equal(out, want["values"])


def test_library_exports_the_certificate_entry_points():
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", spasm_amd.LIB_PATH], check=True, capture_output=True, text=True).stdout
    names = {line.split()[-1] for line in out.splitlines()}
    for sym in ("spasm_hip_xApy", "spasm_hip_xApy_batch", "spasm_hip_xApy_stats", "spasm_hip_certificate_rank_create",
                "spasm_hip_certificate_rank_verify", "spasm_hip_factorization_verify", "spasm_hip_factorization_verify_batch",
                "spasm_hip_rank_certificate_save", "spasm_hip_rank_certificate_load", "spasm_hip_rank_certificate_free"):
        assert sym in names, sym


def test_python_entry_points_refuse_before_c(oracle):
    p = 42013
    A = oracle.load_sms(matrix_path("mat364.sms"), p)
    U, qinv, L, Lp = oracle_fact(oracle, A, False)
    P = lambda M: spasm_amd.Csr(M.n, M.m, M.p, M.j, M.x, M.prime)      # noqa: E731
    Ap = P(A)
    h = bytes(32)
    with pytest.raises(ValueError):
        spasm_amd.certificate_rank_create(Ap, h, spasm_amd.Fact(P(U), qinv))
    with pytest.raises(ValueError):
        spasm_amd.certificate_rank_create(Ap, b"short", spasm_amd.Fact(P(U), qinv, L=P(L), Lp=Lp))
    with pytest.raises(ValueError):
        spasm_amd.xApy(np.zeros(A.n + 1, np.int64), Ap)
    with pytest.raises(ValueError):
        spasm_amd.xApy(np.zeros((65, A.n), np.int64), Ap)
    if spasm_amd.device_count() == 0:
        with pytest.raises(RuntimeError):
            spasm_amd.xApy(np.zeros(A.n, np.int64), Ap)
        with pytest.raises(RuntimeError):
            spasm_amd.factorization_verify(Ap, spasm_amd.Fact(P(U), qinv, L=P(L), Lp=Lp))
