"""spasm_hip_transpose_device / spasm_hip_dtranspose (spasm_amd/csrc/transpose.hip) against the numpy model of the stable order
(tests/kernel_cases.py): every route at tiny sizes through the two experiment switches, the routes asserted from the stats."""
import os
import subprocess
import sys

import numpy as np
import pytest

import spasm_amd
from conftest import ROOT, matrix_path
import kernel_cases as kc

pytestmark = pytest.mark.gpu

CASES = kc.transpose_cases()
SWITCHES = ("SPASM_HIP_TRANSPOSE_SHORT", "SPASM_HIP_TRANSPOSE_CHUNK")


def _set(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _check(A, T, keep_values=True):
    p, j, x = kc.model_transpose(A, keep_values)
    assert (T.n, T.m, T.prime) == (A.m, A.n, A.prime)
    assert np.array_equal(T.p, p) and np.array_equal(T.j, j)
    if x is None:
        assert T.x is None
    else:
        assert T.x is not None and T.x.dtype == np.int32 and np.array_equal(T.x, x)


def _pattern(A):
    B = spasm_amd.Csr(A.n, A.m, A.p, A.j, A.x, A.prime)
    B.x = None
    return B


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_stable_transpose_on_every_route(case, monkeypatch):
    name, A, env, routes = case
    _set(monkeypatch, env)
    T = spasm_amd.transpose_device(A)
    st = spasm_amd.transpose_stats()
    _check(A, T)
    assert (st["short_columns"], st["long_columns"], st["row_chunks"]) == routes
    assert st["longest_column"] == (np.diff(T.p).max() if T.n else 0)
    # without values, and from a pattern: x is absent
    _check(A, spasm_amd.transpose_device(A, keep_values=False), keep_values=False)
    _check(_pattern(A), spasm_amd.transpose_device(_pattern(A)))
    # twice is A with its rows sorted by column, which the model gives as well; two calls return the same arrays
    TT = spasm_amd.transpose_device(T)
    _check(T, TT)
    back = spasm_amd.transpose_device(spasm_amd.transpose_device(TT))
    assert np.array_equal(back.p, TT.p) and np.array_equal(back.j, TT.j) and np.array_equal(back.x, TT.x)
    again = spasm_amd.transpose_device(A)
    assert np.array_equal(again.p, T.p) and np.array_equal(again.j, T.j) and np.array_equal(again.x, T.x)


@pytest.mark.parametrize("env", [{}, {"SPASM_HIP_TRANSPOSE_SHORT": "4", "SPASM_HIP_TRANSPOSE_CHUNK": "128"}], ids=["default", "small"])
@pytest.mark.parametrize("name", kc.GOLDEN_FOR_TRANSPOSE)
def test_golden_matrices_both_ways(name, env, monkeypatch):
    _set(monkeypatch, env)
    A = spasm_amd.load(matrix_path(name), 42013)
    T = spasm_amd.transpose_device(A)
    _check(A, T)
    st = spasm_amd.transpose_stats()
    lens, short_max, chunk = np.diff(T.p), (4 if env else kc.TR_SHORT), (128 if env else kc.TR_CHUNK)
    nlong = int(np.sum(lens > short_max))
    assert st["short_columns"] == np.sum((lens > 0) & (lens <= short_max)) and st["long_columns"] == nlong
    assert st["row_chunks"] == (-(-A.n // chunk) if nlong else 0)
    host = spasm_amd.transpose(A)
    assert np.array_equal(T.p, host.p) and np.array_equal(T.j, host.j) and np.array_equal(T.x, host.x)
    # sorted rows: transposing twice returns A itself
    back = spasm_amd.transpose_device(T)
    assert np.array_equal(back.p, A.p) and np.array_equal(back.j, A.j) and np.array_equal(back.x, A.x)


def test_device_pointer_entry_point(monkeypatch):
    """spasm_hip_dtranspose on tensors resident in HBM, on a stream of the caller's"""
    import ctypes as C
    import torch
    _set(monkeypatch, {"SPASM_HIP_TRANSPOSE_SHORT": "4"})
    A = dict((c[0], c[1]) for c in CASES)["random_sparse"]
    dA = spasm_amd.DeviceCsr.from_host(A)
    Tp = torch.empty(A.m + 1, dtype=torch.int64, device="cuda")
    Tj = torch.empty(A.nnz, dtype=torch.int32, device="cuda")
    Tx = torch.empty(A.nnz, dtype=torch.int32, device="cuda")
    stream = torch.cuda.Stream()
    a = dA.cstruct(nnz=-1)
    with torch.cuda.stream(stream):
        rc = spasm_amd.lib().spasm_hip_dtranspose(C.byref(a), 1, Tp.data_ptr(), Tj.data_ptr(), Tx.data_ptr(), stream.cuda_stream)
    assert rc == 0
    p, j, x = kc.model_transpose(A)
    assert np.array_equal(Tp.cpu().numpy(), p) and np.array_equal(Tj.cpu().numpy(), j) and np.array_equal(Tx.cpu().numpy(), x)
    st = spasm_amd.transpose_stats()
    assert st["upload_ms"] == 0 and st["download_ms"] == 0 and st["long_columns"] > 0


CHILD = """
import numpy as np, spasm_amd
A = spasm_amd.Csr(3, 2, np.array([0, 2, 3, 4]), np.array([1, 1, 0, 1]), np.array([5, 6, 7, 8]), 42013)
spasm_amd.transpose_device(A)
print("returned")
"""


@pytest.mark.parametrize("env", [{}, {"SPASM_HIP_TRANSPOSE_SHORT": "1"}], ids=["short", "long"])
def test_repeated_entry_dies_cleanly(env):
    """a 3 x 2 CSR with (0, 1) twice: outside the contract, refused by either route -- an exit with a message, not a fault"""
    full = dict(os.environ, PYTHONPATH=ROOT, SPASM_HIP_EXPERIMENT="1", **env)
    out = subprocess.run([sys.executable, "-c", CHILD], capture_output=True, text=True, env=full, timeout=120)
    assert out.returncode > 0, (out.returncode, out.stderr[-2000:])          # an exit status, not a signal
    assert "[spasm-hip]" in out.stderr and "twice" in out.stderr and "returned" not in out.stdout
