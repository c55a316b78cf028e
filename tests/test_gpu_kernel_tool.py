"""tools/kernel: the drop-in for the reference's tools/kernel.c, with --left, --output and --check."""
import os
import subprocess

import numpy as np
import pytest

import spasm_amd
from conftest import ROOT, matrix_path
import kernel_cases as kc

pytestmark = pytest.mark.gpu

KERNEL = os.path.join(ROOT, "tools", "kernel")
RANK = os.path.join(ROOT, "tools", "rank")
P = 42013


def _need_tools():
    if not (os.path.exists(KERNEL) and os.path.exists(RANK)):
        subprocess.run(["make", "-C", os.path.join(ROOT, "tools")], check=True)


def _read_sms(path, p):
    with open(path) as f:
        lines = f.read().strip().split("\n")
    n, m, kind = lines[0].split()
    assert kind == "M" and lines[-1].split() == ["0", "0", "0"]
    M = np.zeros((int(n), int(m)), np.int64)
    for line in lines[1:-1]:
        i, j, x = line.split()
        M[int(i) - 1, int(j) - 1] = int(x) % p
    return M


@pytest.mark.parametrize("left", [False, True], ids=["right", "left"])
@pytest.mark.parametrize("name", ["singular.sms", "rectangular_l.sms"])
def test_kernel_tool(name, left, tmp_path):
    _need_tools()
    env = dict(os.environ, SPASM_HIP_VERBOSE="0")
    out_path = str(tmp_path / "K.sms")
    args = [KERNEL, "--matrix", matrix_path(name), "--modulus", str(P), "--output", out_path, "--check"] + (["--left"] if left else [])
    out = subprocess.run(args, capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "CORRECT kernel basis" in out.stderr and "INCORRECT" not in out.stderr
    A = kc.dense(spasm_amd.load(matrix_path(name), P), P)
    if left:
        A = A.T.copy()
    # the rank tools/rank reports (a matrix and its transpose have the same)
    r = subprocess.run([RANK, "--matrix", matrix_path(name), "--modulus", str(P)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rank = int(r.stdout.strip().split()[-1])
    K = _read_sms(out_path, P)
    assert K.shape == (A.shape[1] - rank, A.shape[1])
    assert ("Kernel basis matrix is %d x %d with %d nz" % (K.shape[0], K.shape[1], np.count_nonzero(K))) in out.stderr
    assert not np.any(kc.matmul_mod(A, K.T.copy(), P))
    assert len(kc.rref(K, P)[1]) == K.shape[0]


def test_the_check_finds_a_tampered_row():
    """what --check computes, through Python: the rows of K times A^T (from the device transposition) are zero, and no longer
    once one value of K is altered"""
    A = spasm_amd.load(matrix_path("singular.sms"), P)
    F = spasm_amd.echelonize(A)
    K = spasm_amd.kernel_basis(F)
    At = spasm_amd.transpose_device(A)
    rows = kc.balanced(kc.dense(K, P), P)[:64]
    assert K.n > 0 and F.U.n > 0 and not np.any(spasm_amd.xApy(rows, At))
    # one value altered on a pivotal column c: the product changes by column c of A, which is not zero
    c = int(np.flatnonzero(F.qinv >= 0)[0])
    rows[0, c] += 1
    assert np.any(spasm_amd.xApy(rows, At)[0]) and not np.any(spasm_amd.xApy(rows[1:], At))
