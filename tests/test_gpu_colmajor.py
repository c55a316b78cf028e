"""The column-major image of spasm_amd/csrc/colmajor.hip through its users other than the transpose: x.A (spmv.hip) and the
matching's pattern of A^T (matching.hip), on the matrices of kernel_cases.transpose_cases() -- the shapes a count / scan / fill
goes wrong on (no rows, no columns, empty rows, columns around a wave, a column of 4,097 rows, a row of 4,097 columns: the scan
carries across its blocks of 1,024; edge values) -- with their switches ignored, mod 42013 and mod 4294967291.
tests/test_gpu_transpose.py runs the transpose on the same matrices; tests/test_kernel_cases_host.py holds the model of x.A
against the dense helpers without a GPU."""
import numpy as np
import pytest

import dm_cases
import kernel_cases as kc

import spasm_amd

pytestmark = pytest.mark.gpu

CASES = [(name, A) for name, A, _, _ in kc.transpose_cases()]
IDS = [c[0] for c in CASES]


@pytest.mark.parametrize("p", kc.COLMAJOR_MODULI)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_xApy_is_the_exact_product(case, p):
    """k = 1 and k = 3: equal to the integer model mod p, balanced; the two lists of x.A hold every column, the empty ones
    included (a product with no columns returns before it records its statistics: nothing to read there)"""
    A = kc.with_prime(case[1], p)
    lens = np.diff(kc.model_transpose(A)[0])
    X, Y0 = kc.xa_inputs(A, 3, 7)
    want = kc.model_xApy(X, A, Y0)
    for k in (1, 3):
        got = np.asarray(spasm_amd.xApy(X[:k], A, Y0[:k]), np.int64)
        assert got.shape == (k, A.m)
        assert np.array_equal(got % p, want[:k])
        assert np.all(got >= p // 2 - p + 1) and np.all(got <= p // 2)
        if A.m > 0:
            st = spasm_amd.xApy_stats()
            assert st["k"] == k and st["nnz"] == A.nnz
            assert st["long_columns"] == np.sum(lens > kc.XA_LONG)
            assert st["short_columns"] + st["long_columns"] == A.m


@pytest.mark.parametrize("p", kc.COLMAJOR_MODULI)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_matching_and_dm_on_the_pattern(case, p):
    A = kc.with_prime(case[1], p)
    jm, im, size = spasm_amd.maximum_matching(A)
    rows = np.flatnonzero(jm >= 0)
    cols = np.flatnonzero(im >= 0)
    assert len(rows) == len(cols) == size
    assert np.array_equal(im[jm[rows]], rows) and np.array_equal(jm[im[cols]], cols), "jmatch and imatch are not inverse to each other"
    for i in rows.tolist():
        assert jm[i] in A.j[A.p[i]:A.p[i + 1]], "a matched pair is not an entry of A"
    dm_cases.check_dm(A, spasm_amd.dulmage_mendelsohn(A), size)
    assert spasm_amd.maximum_matching(dm_cases.transpose_of(A, spasm_amd.Csr))[2] == size
