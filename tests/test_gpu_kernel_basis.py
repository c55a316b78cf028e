"""spasm_hip_kernel_basis (spasm_amd/csrc/kernel_basis.hip) against spasm_hip_kernel, array for array, on echelonized golden
matrices and on the constructed factors of tests/kernel_cases.py, and against the exact model of the kernel basis."""
import numpy as np
import pytest

import spasm_amd
from conftest import matrix_path
import kernel_cases as kc
from test_gpu_echelonize import SMALL_SET

pytestmark = pytest.mark.gpu

FACTOR_CASES = kc.factor_cases()


def _same(K, want):
    assert (K.n, K.m, K.prime) == (want.n, want.m, want.prime)
    assert np.array_equal(K.p, want.p) and np.array_equal(K.j, want.j) and np.array_equal(K.x, want.x)


@pytest.mark.parametrize("p", [257, 42013, 4294967291])
@pytest.mark.parametrize("name", SMALL_SET + ["mat364.sms"])
def test_kernel_basis_equals_kernel_on_echelonized_matrices(name, p):
    A = spasm_amd.load(matrix_path(name), p)
    F = spasm_amd.echelonize(A)
    want = spasm_amd.kernel(F)
    K = spasm_amd.kernel_basis(F)
    _same(K, want)
    st = spasm_amd.kernel_stats()
    assert (st["rows"], st["nnz"]) == (K.n, K.nnz) and K.n == A.m - F.U.n


@pytest.mark.parametrize("case", FACTOR_CASES, ids=[c[0] for c in FACTOR_CASES])
def test_kernel_basis_on_constructed_factors(case, monkeypatch):
    name, F, env, retry = case
    monkeypatch.delenv("SPASM_HIP_KERNEL_POOL", raising=False)
    want = spasm_amd.kernel(F)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    K = spasm_amd.kernel_basis(F)
    st = spasm_amd.kernel_stats()
    _same(K, want)
    U, p = F.U, F.U.prime
    assert (K.n, K.m) == (U.m - U.n, U.m) and K.p[0] == 0
    assert (st["pool_retries"] >= 1) if retry else (st["pool_retries"] == 0)
    # the exact model: the same matrix, so U . K^T == 0 and rank K == m - r; -1 stored as the balanced value
    model = kc.model_kernel(F)
    assert np.array_equal(kc.balanced(kc.dense(K, p), p), model)
    assert not np.any(kc.matmul_mod(kc.dense(U, p), kc.dense(K, p).T.copy(), p))
    assert len(kc.rref(kc.dense(K, p), p)[1]) == U.m - U.n
    nonpiv = np.flatnonzero(F.qinv < 0)
    assert np.array_equal(K.j[K.p[:-1]], nonpiv) and np.all(K.x[K.p[:-1]] == -1)
    if K.nnz:
        assert K.x.min() >= p // 2 - p + 1 and K.x.max() <= p // 2
