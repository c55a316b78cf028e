"""GPU parity of the dense image's build through the tables of backsolve_plan (spasm_amd/csrc/backsolve.hip): rows handed to
the kernel as pre-scaled offsets, heads read once, rows that start at zero in registers with the entries of U_n added to
the LDS ring afterwards.  S = A_n - A_p R from spasm_hip_schur (the C ABI) is compared with spasm_schur's, entry for entry,

  * on a factor whose rows have more than two dependencies outside their chunk AND more than two inside it (the `far` and
    `near` lists, beside the two inline ones of the head and of the pass table);
  * with non-pivotal entries of U in adjacent columns, which share a packed 32-bit word of the ring, on a column count
    that is no multiple of any slab width and whose last slab of 12 words reaches beyond the padded row (505..512);
  * on a factor with more than four non-pivotal entries per row of U, which takes the pre-filled path (sparse_init == 0);

for one modulus of each arithmetic (signed 16-bit, unsigned 16-bit, 32-bit Montgomery) and every SPASM_HIP_BS_SHAPE."""
import numpy as np
import pytest

import spasm_amd

pytestmark = pytest.mark.gpu

PRIMES = [42013, 65521, 4294967291]
SHAPES = ["0", "1", "2", "3", "4", "5"]


def _as_product(A):
    return spasm_amd.Csr(A.n, A.m, A.p, A.j, A.x, A.prime)


def _system(rng, p, npiv, nnon, nred, near, far, np_cols, red_entries):
    """pivot row k: 1 on column k, `near` pivotal entries among the next 40 columns, `far` of them at least 1500 columns
    away, and non-pivotal entries on the columns np_cols(k) of the nnon trailing ones; then nred rows to reduce."""
    m = npiv + nnon
    ti, tj, tx = [], [], []
    for k in range(npiv):
        cols = [k]
        room = min(40, npiv - k - 1)
        if room > 0:
            cols += list(k + 1 + rng.choice(room, size=min(near, room), replace=False))
        room = npiv - (k + 1500)
        if room > 0:
            cols += list(k + 1500 + rng.choice(room, size=min(far, room), replace=False))
        cols += [npiv + int(c) for c in np_cols(k)]
        ti += [k] * len(cols)
        tj += [int(c) for c in cols]
        tx += [1] + [int(v) for v in rng.integers(1, p, size=len(cols) - 1)]
    for k in range(nred):
        cols = rng.choice(m, size=min(red_entries, m), replace=False)
        ti += [npiv + k] * len(cols)
        tj += [int(c) for c in cols]
        tx += [int(v) for v in rng.integers(1, p, size=len(cols))]
    return npiv + nred, m, np.array(ti, np.int32), np.array(tj, np.int32), np.array(tx, np.int64)


def _check(oracle, monkeypatch, p, shape, sysm, min_pivots, np_per_row_above_four):
    monkeypatch.setenv("SPASM_HIP_BACKSOLVE", "1")
    monkeypatch.setenv("SPASM_HIP_BS_SHAPE", shape)
    spasm_amd.lib().spasm_hip_forget_cached_images()
    n, m, ti, tj, tx = sysm
    A = oracle.compress(p, n, m, ti, tj, tx)
    npiv, perm, F = oracle.pivots_extract_structural(A, oracle.empty_fact(A.n, A.m, p))
    assert npiv >= min_pivots
    # which start of the rows the build takes (backsolve_build: the kernel adds U_n itself up to four entries per row)
    nnp = int(np.count_nonzero(np.asarray(F.qinv)[np.asarray(F.U.j[:F.U.p[F.U.n]])] < 0))
    assert (nnp > 4 * F.U.n) == np_per_row_above_four
    rows = perm[npiv:]
    want, p_out_want, _ = oracle.schur(A, rows, F)
    S, p_out = spasm_amd.schur(_as_product(A), rows, spasm_amd.Fact(_as_product(F.U), F.qinv))
    assert np.array_equal(p_out, p_out_want)
    assert oracle.same_matrix(oracle.CSR(S.n, S.m, S.p, S.j, S.x, p), want)
    for i in range(S.n):
        jj, _ = S.row(i)
        assert np.all(np.diff(jj) > 0)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("p", PRIMES)
def test_plan_far_and_near_lists(oracle, monkeypatch, p, shape):
    """four dependencies within 40 rows (inside the chunk: one in the pass table, three in the near list) and four at least
    1,500 rows away (outside any chunk of <= 1,260 rows: two in the head, two in the far list)."""
    rng = np.random.default_rng(101)
    nnon = 100
    sysm = _system(rng, p, npiv=3600, nnon=nnon, nred=300, near=4, far=4, np_cols=lambda k: rng.choice(nnon, size=3, replace=False), red_entries=6)
    _check(oracle, monkeypatch, p, shape, sysm, min_pivots=3000, np_per_row_above_four=False)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("p", PRIMES)
def test_plan_adjacent_entries_and_last_slab(oracle, monkeypatch, p, shape):
    """every other row of U has four of its entries on five consecutive non-pivotal columns (three packed words: two of the
    four share one, wherever the words begin), the others three anywhere; 509 non-pivotal columns: 21 slabs of 24 columns
    and 5 more, and the 22nd slab of 12 words ends beyond the 256 words of the padded row."""
    rng = np.random.default_rng(202)
    nnon = 509

    def np_cols(k):
        if k % 2 == 0:
            base = int(rng.integers(0, nnon - 5))
            return base + rng.choice(5, size=4, replace=False)
        return rng.choice(nnon, size=3, replace=False)
    sysm = _system(rng, p, npiv=2600, nnon=nnon, nred=300, near=2, far=1, np_cols=np_cols, red_entries=6)
    _check(oracle, monkeypatch, p, shape, sysm, min_pivots=2000, np_per_row_above_four=False)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("p", PRIMES)
def test_plan_prefilled_rows(oracle, monkeypatch, p, shape):
    """seven non-pivotal entries per row of U: R is pre-filled by bs_init_kernel and the rows start from it."""
    rng = np.random.default_rng(303)
    nnon = 333
    sysm = _system(rng, p, npiv=2600, nnon=nnon, nred=300, near=3, far=3, np_cols=lambda k: rng.choice(nnon, size=7, replace=False), red_entries=6)
    _check(oracle, monkeypatch, p, shape, sysm, min_pivots=2000, np_per_row_above_four=True)
