"""Every launch shape of the X.A = B solver (spasm_amd/csrc/solve.hip) on factorizations built for it (tests/solve_cases.py):
X and ok must equal the exact model's, array for array, and Solver.levels / Solver.stats() must say that the launches the
shape was built for are the ones that ran (the counts of solve_cases.planned, which tests/test_solve_cases_host.py holds
against each shape's claim)."""
import numpy as np
import pytest

import solve_cases as sc
from test_solve_host import balanced, dense

import spasm_amd

pytestmark = pytest.mark.gpu


def _fact(fact):
    U, qinv, L, Lp = fact
    return spasm_amd.Fact(U, qinv, L=L, Lp=Lp)


def _assert_same(X, ok, want, okw):
    assert (X.n, X.m) == (want.n, want.m)
    assert np.array_equal(X.p, want.p)
    assert np.array_equal(X.j, want.j)
    assert np.array_equal(X.x, want.x)
    assert ok.dtype == np.bool_ and np.array_equal(ok, okw)


def _assert_plan(S, plan, batches=1):
    """the launches of the plan are the solver's, kind by kind"""
    assert S.levels == {"forward": plan["F"]["levels"], "back": plan["B"]["levels"], "forward_launches": plan["F"]["launches"],
                        "back_launches": plan["B"]["launches"]}
    st = S.stats()
    got = {k: int(st[k]) for k in ("forward_split_launches", "back_split_launches", "forward_run_launches", "back_run_launches")}
    assert got == {"forward_split_launches": plan["F"]["split"], "back_split_launches": plan["B"]["split"],
                   "forward_run_launches": plan["F"]["run"], "back_run_launches": plan["B"]["run"]}
    assert (int(st["forward_launches"]), int(st["back_launches"])) == (batches * plan["F"]["launches"], batches * plan["B"]["launches"])
    assert int(st["launches"]) == batches * (7 + plan["F"]["launches"] + plan["B"]["launches"])
    assert int(st["batches"]) == batches


def _run(fact, B, p, plan=None):
    """Solver(F).gesv(B) against the model and the plan; returns (X, ok, the model's X, the plan)"""
    plan = sc.planned(*fact) if plan is None else plan
    want, okw = sc.model_gesv(*fact, B, p)
    with spasm_amd.Solver(_fact(fact)) as S:
        X, ok = S.gesv(B)
        _assert_plan(S, plan, batches=1 if B.n else 0)
    _assert_same(X, ok, want, okw)
    return X, ok, want, plan


@pytest.mark.parametrize("p", sc.SMALL_PRIMES)
@pytest.mark.parametrize("u,l", sc.PAIRS)
def test_launch_kinds(u, l, p):
    """one level per launch, runs of thin levels, split lists (one level and a run), each as U's structure and as L's; 70
    right-hand sides (two blocks) that fill every unknown"""
    fact, rng = sc.pair_case(u, l, p, ncheck=5)
    B = sc.right_hand_sides(rng, p, *fact[:3], 70)
    X, ok, want, plan = _run(fact, B, p)
    assert sc.summary(plan["F"]) == sc.CLAIMS[u] and sc.summary(plan["B"]) == sc.CLAIMS[l]
    assert ok[0:68:2].all() and not ok[1:68:2].any() and ok[68]
    assert (np.diff(X.p)[0:68:3] > fact[0].n // 2).all()                # (the dense combinations reach most unknowns)
    Y, oky = spasm_amd.gesv(_fact(fact), B)
    _assert_same(Y, oky, want, ok)
    if u.startswith("split_run"):
        b = dense(B)[0]
        x, okx = spasm_amd.solve(_fact(fact), balanced(b, p))
        assert okx == ok[0]
        assert np.array_equal(x.astype(np.int64) % p, dense(X)[0])


@pytest.fixture(scope="module")
def k_factor():
    p = 42013
    fact, rng = sc.flat_case(sc.K_RANK, p, ncheck=6)
    S = spasm_amd.Solver(_fact(fact))
    yield p, fact, rng, S, sc.planned(*fact)
    S.close()


@pytest.mark.parametrize("k", sc.K_VALUES)
def test_numbers_of_right_hand_sides(k_factor, k):
    """around the blocks of 64 and the scan's chunks of 1,024 (1,025 and 2,049: the carry from chunk to chunk), on two emit chunks"""
    p, fact, rng, S, plan = k_factor
    assert plan["emit_chunks"] == 2
    B = sc.right_hand_sides(np.random.default_rng(k), p, *fact[:3], k, dense_rows=False, combine=20)
    want, okw = sc.model_gesv(*fact, B, p)
    X, ok = S.gesv(B)
    _assert_same(X, ok, want, okw)
    _assert_plan(S, plan, batches=1 if k else 0)
    if k >= 4:
        assert X.p[k] > 20 * (k - 2)                # rows long enough to fill both chunks


def test_one_solver_through_shrinking_and_growing_calls(k_factor):
    p, fact, rng, S, plan = k_factor
    for k in (1, 2049, 3):
        B = sc.right_hand_sides(np.random.default_rng(100 + k), p, *fact[:3], k, dense_rows=False, combine=20)
        want, okw = sc.model_gesv(*fact, B, p)
        X, ok = S.gesv(B)
        _assert_same(X, ok, want, okw)
        _assert_plan(S, plan)
        assert int(S.stats()["rhs_per_batch"]) == (k + 63) // 64 * 64


@pytest.mark.parametrize("r,p", [(1023, 42013), (1024, 42013), (1535, 4294967291), (2563, 42013), (2563, 4294967291)])
def test_emit_chunks(r, p):
    """1, 2, 2 and 5 chunks of the emission (2,563 / 5: bounds that do not divide, more chunks than a workgroup has waves)"""
    fact, rng = sc.flat_case(r, p, ncheck=3)
    B = sc.right_hand_sides(rng, p, *fact[:3], 65, dense_rows=False, combine=60)
    X, ok, want, plan = _run(fact, B, p)
    assert plan["emit_chunks"] == sc.EMIT_RANKS[r]
    assert X.p[65] > 60 * 60


def test_emit_chunks_at_their_cap():
    """rank 131,772: 257 chunks asked for, 256 taken"""
    p = 42013
    fact, rng = sc.flat_case(sc.WIDE_RANK, p, ncheck=3)
    B = sc.right_hand_sides(rng, p, *fact[:3], 65, dense_rows=False, combine=40)
    X, ok, want, plan = _run(fact, B, p)
    assert plan["emit_chunks"] == 256 and sc.WIDE_RANK // 512 == 257
    assert X.p[65] > 60 * 40 and X.j.max() > sc.WIDE_RANK - 2000 and X.j.min() < 2000


@pytest.mark.parametrize("nc", list(sc.CHECK_COLUMNS))
def test_check_columns(nc):
    """0 columns to check (every right-hand side has a solution), 1, 8, 9 (one wave, then two), 4,100 (the cap of 512)"""
    p = 65537
    fact, rng = sc.check_case(nc, p)
    B = sc.right_hand_sides(rng, p, *fact[:3], 70)
    X, ok, want, plan = _run(fact, B, p)
    assert (plan["checked"], plan["check_waves"]) == (nc, sc.CHECK_COLUMNS[nc])
    if nc == 0:
        assert ok.all()
    else:
        assert ok[0:68:2].all() and not ok[1:68:2].any()


@pytest.mark.parametrize("p", [42013, 4294967291])
def test_check_columns_without_an_entry_in_u(p):
    """a non-zero b in a column that no row of U touches: no solution"""
    fact, rng = sc.check_case(8, p, check_used=0.5)
    U, qinv = fact[0], fact[1]
    empty = np.setdiff1d(np.flatnonzero(qinv < 0), np.unique(U.j))
    assert len(empty) == 4
    B = sc.right_hand_sides(rng, p, *fact[:3], 70, extra_cols=empty)
    X, ok, want, plan = _run(fact, B, p)
    assert ok[0:68:2].all() and not ok[1:68:2].any()


@pytest.mark.parametrize("p", [3, 65537, 4294967291])
@pytest.mark.parametrize("nc", [0, 9])
@pytest.mark.parametrize("row_order", ["reversed", "half"])
def test_late_pivot_columns(row_order, nc, p):
    """rows of U in reverse order (F has no dependency left, every touched pivot column is checked) and half of them; with
    every column a pivot column (nc = 0) the late ones are all there is to check, and they alone say that the reference's loop
    does not clear these right-hand sides"""
    fact, rng = sc.check_case(nc, p, row_order=row_order)
    B = sc.right_hand_sides(rng, p, *fact[:3], 70)
    X, ok, want, plan = _run(fact, B, p)
    assert plan["late"] > 0 and plan["checked"] == nc + plan["late"]
    assert plan["F"]["levels"] == 1 if row_order == "reversed" else plan["F"]["levels"] > 1
    assert not ok[0:68:2].all() and ok[68]              # combinations of rows of U, not cleared; the zero row is


@pytest.mark.parametrize("p", [2147483659, 4294967291])
def test_scatter_of_repeated_columns_that_wrap(p):
    """two entries -1 in one column: (p-1) + (p-1) passes 2^32"""
    fact, rng = sc.pair_case("sweep", "runs", p, ncheck=5)
    U, qinv, L, Lp = fact
    base = sc.right_hand_sides(rng, p, U, qinv, L, 8)
    piv, free = int(np.flatnonzero(qinv >= 0)[3]), int(np.flatnonzero(qinv < 0)[0])
    ptr, cols, vals = [0], [], []
    for t in range(8):
        j, x = base.row(t)
        j, x = j.tolist(), x.tolist()
        if t in (0, 1, 4):
            c = piv if t != 1 else free
            j, x = [c, c] + j, [-1, -1] + x             # (first in the row: the sum of the two is what wraps)
        if t == 4:
            j, x = [piv] + j, [-1] + x                  # three times
        cols += j
        vals += x
        ptr.append(len(cols))
    B = spasm_amd.Csr(8, U.m, np.asarray(ptr, np.int64), np.asarray(cols, np.int32), np.asarray(vals, np.int32), p)
    assert 2 * (p - 1) >= 2 ** 32
    _run(fact, B, p)


@pytest.mark.parametrize("p", [3, 65537, 2147483647])
def test_values_stored_in_0_p(p):
    fact, rng = sc.pair_case("runs", "sweep", p, seed=5, ncheck=5)
    state = rng.bit_generator.state
    B = sc.right_hand_sides(rng, p, *fact[:3], 70, unbalanced=True)
    assert B.x.min() >= 0 and (p == 3 or B.x.max() > p // 2)
    X, ok, want, plan = _run(fact, B, p)
    rng.bit_generator.state = state
    Bb = sc.right_hand_sides(rng, p, *fact[:3], 70)
    assert np.array_equal(Bb.j, B.j) and Bb.x.min() < 0
    with spasm_amd.Solver(_fact(fact)) as S:
        Y, oky = S.gesv(Bb)
    _assert_same(Y, oky, X, ok)


@pytest.mark.parametrize("p", [3, 4294967291])
@pytest.mark.parametrize("which", sc.ODDITIES)
def test_what_the_reference_tolerates_in_a_factor(which, p):
    """rows of L without a pivot, entries right of the diagonal, repeated entries, rows of U out of order: one at a time and together"""
    fact, rng = sc.oddity_case(which, p)
    B = sc.right_hand_sides(rng, p, *fact[:3], 40)
    X, ok, want, plan = _run(fact, B, p)
    Lp = fact[3]
    assert (np.diff(Lp) < 0).any()
    for t in range(40):
        assert np.all(np.diff(X.row(t)[0]) > 0) and set(X.row(t)[0].tolist()) <= set(Lp.tolist())


@pytest.fixture(scope="module")
def batch_case():
    p = 65537
    fact, rng = sc.pair_case("sweep", "runs", p, seed=9, ncheck=5)
    B = sc.right_hand_sides(rng, p, *fact[:3], 321)
    want, okw = sc.model_gesv(*fact, B, p)
    lengths = np.diff(B.p)
    assert lengths.max() > 10 * max(1, lengths[lengths > 0].min()) and len(set(lengths.tolist())) > 50      # very different lengths
    return p, fact, B, want, okw, sc.planned(*fact)


def _head(M, k):
    return spasm_amd.Csr(k, M.m, M.p[:k + 1], M.j[:M.p[k]], M.x[:M.p[k]], M.prime)


@pytest.mark.parametrize("k", [1, 64, 65, 200, 321])
@pytest.mark.parametrize("cap", [64, 128])
def test_batches(batch_case, monkeypatch, cap, k):
    """SPASM_HIP_SOLVE_BATCH: the rows of B rebased batch by batch, ok and the row pointers of X continued"""
    p, fact, B, want, okw, plan = batch_case
    Bk = _head(B, k)
    wk, okk = (want, okw) if k == 321 else sc.model_gesv(*fact, Bk, p)
    with spasm_amd.Solver(_fact(fact)) as S:
        monkeypatch.delenv("SPASM_HIP_SOLVE_BATCH", raising=False)
        X1, ok1 = S.gesv(Bk)
        _assert_plan(S, plan, batches=1)
        assert int(S.stats()["rhs_per_batch"]) == (k + 63) // 64 * 64
        monkeypatch.setenv("SPASM_HIP_SOLVE_BATCH", str(cap + 5))          # (rounded down to a multiple of 64)
        X, ok = S.gesv(Bk)
        per = min(cap, (k + 63) // 64 * 64)
        _assert_plan(S, plan, batches=(k + per - 1) // per)
        assert int(S.stats()["rhs_per_batch"]) == per
    _assert_same(X1, ok1, wk, okk)
    _assert_same(X, ok, wk, okk)
    assert np.array_equal(wk.p, want.p[:k + 1])
