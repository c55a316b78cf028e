"""tests/kernel_cases.py checked without a GPU: the numpy model of the stable order against the host spasm_amd.transpose, the
routes each transposition case claims, and the exact model of the kernel basis on every constructed factor."""
import os

import numpy as np
import pytest

import spasm_amd
from conftest import ROOT, matrix_path
import kernel_cases as kc

TRANSPOSE_CASES = kc.transpose_cases()
FACTOR_CASES = kc.factor_cases()


def _same_as_host_transpose(A):
    p, j, x = kc.model_transpose(A)
    T = spasm_amd.transpose(A)
    assert (T.n, T.m) == (A.m, A.n)
    assert np.array_equal(T.p, p) and np.array_equal(T.j, j) and np.array_equal(T.x, x)


@pytest.mark.parametrize("case", TRANSPOSE_CASES, ids=[c[0] for c in TRANSPOSE_CASES])
def test_model_of_the_stable_order_is_the_host_transpose(case):
    _same_as_host_transpose(case[1])


@pytest.mark.parametrize("name", kc.GOLDEN_FOR_TRANSPOSE)
def test_model_of_the_stable_order_on_the_golden_matrices(name):
    A = spasm_amd.load(matrix_path(name), 42013)
    _same_as_host_transpose(A)
    _same_as_host_transpose(spasm_amd.transpose(A))


def test_transposition_cases_reach_every_route():
    routes = {c[0]: c[3] for c in TRANSPOSE_CASES}
    assert routes["threshold_default"] == (2, 1, 1) and routes["threshold_4"] == (2, 1, 1)
    assert [routes["chunks_%d" % k][2] for k in (1, 2, 3)] == [1, 2, 3]
    assert routes["one_column_4097_rows"] == (0, 1, 1) and routes["one_column_65_rows"] == (1, 0, 0)
    assert routes["one_row_4097_columns"] == (4097, 0, 0)
    assert routes["full_alternating_last"] == (1, 2, 1) and routes["full_alternating_last_chunked"] == (1, 2, 8)
    assert routes["0x0"] == routes["5x0"] == routes["0x5"] == routes["empty_rows"] == (0, 0, 0)
    # entries on both sides of the chunk boundaries, first and last entry of a column on one
    A = dict((c[0], c[1]) for c in TRANSPOSE_CASES)["chunks_3"]
    p, j, _ = kc.model_transpose(A)
    assert j[p[2]:p[3]].tolist() == [127, 128, 255, 256]
    values = dict((c[0], c[1]) for c in TRANSPOSE_CASES)["edge_values_long"].x
    assert {kc.INT32_MIN, kc.INT32_MAX, 0, -1} <= set(values.tolist())


def test_the_two_default_thresholds_the_cases_are_built_around():
    text = open(os.path.join(ROOT, "spasm_amd", "csrc", "transpose.hip")).read()
    for expr in kc.SOURCE_EXPRESSIONS:
        assert expr in text, expr


@pytest.mark.parametrize("p", kc.COLMAJOR_MODULI)
@pytest.mark.parametrize("case", TRANSPOSE_CASES, ids=[c[0] for c in TRANSPOSE_CASES])
def test_model_xApy_is_the_dense_product(case, p):
    """the entry-by-entry model tests/test_gpu_colmajor.py holds x.A against, checked against the dense helpers"""
    A = kc.with_prime(case[1], p)
    X, Y0 = kc.xa_inputs(A, 3, 7)
    want = (kc.matmul_mod(X, kc.dense(A, p), p) + Y0) % p
    assert np.array_equal(kc.model_xApy(X, A, Y0), want)
    assert np.array_equal(kc.model_xApy(X[:1], A, Y0[:1]), want[:1])


def test_colmajor_cases_reach_both_lists_of_xA_and_a_scan_carry():
    lens = {c[0]: np.diff(kc.model_transpose(c[1])[0]) for c in TRANSPOSE_CASES}
    assert "XA_LONG = %d;" % kc.XA_LONG in open(os.path.join(ROOT, "spasm_amd", "csrc", "spmv.hip")).read()
    assert lens["one_column_4097_rows"].tolist() == [4097] and lens["one_row_4097_columns"].tolist() == [1] * 4097
    assert np.sum(lens["random_sparse"] == 0) > 0 and np.sum(lens["full_alternating_last"] > kc.XA_LONG) == 2
    assert [int(lens["one_column_%d_rows" % n][0] > kc.XA_LONG) for n in (1, 63, 64, 65)] == [0, 1, 1, 1]


@pytest.mark.parametrize("case", FACTOR_CASES, ids=[c[0] for c in FACTOR_CASES])
def test_model_kernel_of_the_constructed_factors(case):
    """U . K^T == 0 and rank K == m - r for the exact model, and the factor is what the library expects: unit pivots first,
    on distinct columns, recorded in qinv"""
    F = case[1]
    U, p = F.U, F.U.prime
    for i in range(U.n):
        jj, xx = U.row(i)
        assert xx[0] == 1 and F.qinv[jj[0]] == i and len(set(jj.tolist())) == len(jj)
    assert int(np.sum(F.qinv >= 0)) == U.n
    K = kc.model_kernel(F)
    assert K.shape == (U.m - U.n, U.m)
    assert not np.any(kc.matmul_mod(kc.dense(U, p), (K % p).T.copy(), p))
    assert len(kc.rref(K % p, p)[1]) == U.m - U.n
    assert K.size == 0 or (K.min() >= p // 2 - p + 1 and K.max() <= p // 2)


def test_factor_cases_cover_the_moduli_and_the_orders():
    cases = {c[0]: c for c in FACTOR_CASES}
    assert {c[1].U.prime for c in FACTOR_CASES} >= {3, 4294967291}
    assert [cases["corank_1_r%s" % s][1].U.n for s in ("1", "64", "65_big", "300")] == [1, 64, 65, 300]
    piv = [int(cases["shuffled_rows"][1].U.row(i)[0][0]) for i in range(40)]
    assert piv != sorted(piv)
    F = cases["one_dense_column"][1]
    nonpiv = np.flatnonzero(F.qinv < 0)
    counts = np.bincount(F.U.j, minlength=F.U.m)[nonpiv]
    assert counts.tolist() == [0, 0, F.U.n, 0, 0]
    assert any(c[3] for c in FACTOR_CASES)
