"""CPU checks of tests/solve_cases.py: the model returns what the compiled reference stored for every case of
tests/golden/reference/gesv.npz, the constants and expressions the shapes are built around are still in solve.hip (the scan: colmajor.hip), and
every shape of tests/test_gpu_solve_shapes.py lands on the launches it claims."""
import os

import numpy as np
import pytest

import modulus_edges as me
import solve_cases as sc
from test_solve_host import CASES, stored_case

SOLVE_HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "spasm_amd", "csrc", "solve.hip")


@pytest.mark.parametrize("name,p,complete", CASES)
def test_model_returns_the_stored_reference(oracle, name, p, complete):
    A, U, qinv, L, Lp, B, want = stored_case(oracle, name, p, complete)
    X, ok = sc.model_gesv(U, qinv, L, Lp, B, p)
    assert (X.n, X.m) == (int(want["n"]), int(want["m"]))
    assert np.array_equal(X.p, want["p"])
    assert np.array_equal(X.j, want["j"])
    assert np.array_equal(X.x, want["x"])
    assert np.array_equal(ok.astype(np.uint8), want["ok"])


@pytest.mark.parametrize("expr", sc.SOURCE_EXPRESSIONS)
def test_source_expression_is_still_there(expr):
    """a moved or changed constant fails here first: update solve_cases.py (and the shapes built on it) with it"""
    with open(SOLVE_HIP) as f:
        assert expr in f.read(), "`%s` no longer in spasm_amd/csrc/solve.hip" % expr


@pytest.mark.parametrize("expr", sc.SCAN_EXPRESSIONS)
def test_scan_expression_is_still_there(expr):
    with open(os.path.join(os.path.dirname(SOLVE_HIP), "colmajor.hip")) as f:
        assert expr in f.read(), "`%s` no longer in spasm_amd/csrc/colmajor.hip" % expr


def test_python_constants_are_the_sources():
    with open(SOLVE_HIP) as f:
        text = f.read()
    for name in ("SV_WAVES", "SV_TAIL_WAVES", "SV_THIN", "SV_RUN", "SV_SPLIT"):
        assert "constexpr int %s = %d;" % (name, getattr(sc, name)) in text
    assert sc.SCAN_CHUNK == 1024
    assert [sc.emit_chunks(r) for r in (0, 511, 1023, 1024, 1535, 1536, 2563, 131071, 131072, sc.WIDE_RANK)] == [1, 1, 1, 2, 2, 3, 5, 255, 256, 256]
    assert [sc.check_waves(nc) for nc in (0, 1, 8, 9, 4088, 4089, 4100)] == [1, 1, 1, 2, 511, 512, 512]
    assert all(me.is_prime(q) for q in sc.SMALL_PRIMES + [2147483659])


def test_mul_is_exact():
    rng = np.random.default_rng(0)
    for p in (3, 65537, 2147483659, 3037000507, 4294967291):
        c = np.concatenate([rng.integers(0, p, size=50, dtype=np.int64), [p - 1, p - 1, 0]])
        v = np.concatenate([rng.integers(0, p, size=50, dtype=np.int64), [p - 1, 1, p - 1]])
        assert sc._mul(c, v, p).tolist() == [int(a) * int(b) % p for a, b in zip(c, v)]
        assert sc._mul(p - 1, v, p).tolist() == [(p - 1) * int(b) % p for b in v]


def test_structure_has_the_levels_it_was_asked_for():
    rng = np.random.default_rng(1)
    widths, deps = sc.STRUCTURES["split"]
    r, t, i = sc._structure(rng, widths, deps)
    assert r == sum(widths) and (i < t).all()
    level, ndeps = sc._levels(r, t, i, range(r))
    assert np.bincount(level).tolist() == widths
    want = sorted(np.concatenate([np.broadcast_to(np.asarray(d), (w,)) for w, d in zip(widths, deps)]).tolist())
    assert sorted(ndeps.tolist()) == want
    assert len(set(zip(t.tolist(), i.tolist()))) == len(t)          # no dependency twice


@pytest.mark.parametrize("p", sc.SMALL_PRIMES)
@pytest.mark.parametrize("u,l", sc.PAIRS)
def test_pairs_land_on_their_launches(u, l, p):
    (U, qinv, L, Lp), _ = sc.pair_case(u, l, p, ncheck=5)
    plan = sc.planned(U, qinv, L, Lp)
    assert sc.summary(plan["F"]) == sc.CLAIMS[u]
    assert sc.summary(plan["B"]) == sc.CLAIMS[l]
    assert plan["checked"] == 5 and plan["late"] == 0
    assert sum(sc.STRUCTURES[u][0]) == sum(sc.STRUCTURES[l][0]) == U.n


def test_split_kinds_of_the_claims():
    """the step kinds behind the counts: where the lone levels split, and that the thin runs are what the claims say"""
    (U, qinv, L, Lp), _ = sc.pair_case("split", "chain", 42013)
    plan = sc.planned(U, qinv, L, Lp)
    assert plan["F"]["steps"] == [(0, 1, False), (1, 2, False), (2, 3, True), (3, 4, True), (4, 5, True), (5, 6, True), (6, 7, False)]
    assert plan["B"]["steps"] == [(0, 1, False), (1, 201, False)]
    (U, qinv, L, Lp), _ = sc.pair_case("split_run", "split_run2", 3)
    plan = sc.planned(U, qinv, L, Lp)
    assert plan["F"]["steps"] == plan["B"]["steps"] == [(0, 1, False), (1, 4, True)]
    (U, qinv, L, Lp), _ = sc.pair_case("runs", "sweep", 65537)
    assert sc.planned(U, qinv, L, Lp)["F"]["steps"] == [(0, 1, False), (1, 3, False), (3, 4, False), (4, 7, False), (7, 8, False), (8, 10, False)]


@pytest.mark.parametrize("r", list(sc.EMIT_RANKS) + [sc.K_RANK, sc.WIDE_RANK])
def test_flat_cases_have_their_emit_chunks(r):
    (U, qinv, L, Lp), _ = sc.flat_case(r, 42013, ncheck=3)
    plan = sc.planned(U, qinv, L, Lp)
    assert U.n == r and plan["emit_chunks"] == {**sc.EMIT_RANKS, sc.K_RANK: 2, sc.WIDE_RANK: 256}[r]
    assert sc.summary(plan["F"]) == sc.summary(plan["B"]) == {"levels": 3, "launches": 3, "split": 0, "run": 0}


@pytest.mark.parametrize("nc", list(sc.CHECK_COLUMNS))
def test_check_cases_have_their_waves(nc):
    (U, qinv, L, Lp), _ = sc.check_case(nc, 65537)
    plan = sc.planned(U, qinv, L, Lp)
    assert (plan["checked"], plan["late"], plan["check_waves"]) == (nc, 0, sc.CHECK_COLUMNS[nc])
    assert U.m == U.n + nc


def test_check_cases_with_late_columns():
    (U, qinv, L, Lp), _ = sc.check_case(9, 65537, row_order="reversed")
    plan = sc.planned(U, qinv, L, Lp)
    assert sc.summary(plan["F"]) == {"levels": 1, "launches": 1, "split": 0, "run": 0}       # every dependency became a late entry
    straight = sc.planned(*sc.check_case(9, 65537)[0])
    assert plan["late"] > 40 and plan["checked"] == 9 + plan["late"] and straight["F"]["levels"] == 3
    (U, qinv, L, Lp), _ = sc.check_case(9, 65537, row_order="half")
    plan = sc.planned(U, qinv, L, Lp)
    assert plan["late"] >= 10 and plan["F"]["levels"] >= 2 and plan["checked"] == 9 + plan["late"]
    for order in ("reversed", "half"):                             # every column a pivot column: the late ones are all that is checked
        plan = sc.planned(*sc.check_case(0, 65537, row_order=order)[0])
        assert plan["checked"] == plan["late"] > 0
    (U, qinv, L, Lp), _ = sc.check_case(8, 65537, check_used=0.5)
    assert len(np.unique(U.j)) == U.n + 4                          # four of the eight columns without a pivot hold no entry


@pytest.mark.parametrize("which", sc.ODDITIES)
def test_oddities_are_in_the_factor(which):
    (U, qinv, L, Lp), _ = sc.oddity_case(which, 42013)
    every = which == "all"
    r = U.n
    assert L.n == r + 9 and L.m == r and len(set(Lp.tolist())) == r and (np.diff(Lp) < 0).any()
    jof = np.full(L.n, -1)
    jof[Lp] = np.arange(r)
    rows = np.repeat(np.arange(L.n), np.diff(L.p))
    assert bool((jof[rows] < 0).any()) == (every or which == "nonpivot")
    assert bool(((jof[rows] >= 0) & (L.j > jof[rows])).any()) == (every or which == "above")
    pairs = list(zip(rows.tolist(), L.j.tolist()))
    assert (len(set(pairs)) < len(pairs)) == (every or which == "repeat")
    plan = sc.planned(U, qinv, L, Lp)
    assert (plan["late"] > 0) == (every or which == "row_order")
    if which in ("nonpivot", "above"):
        assert sc.summary(plan["F"]) == sc.CLAIMS["runs"] and sc.summary(plan["B"]) == sc.CLAIMS["sweep"]


def test_model_solves_what_it_is_given():
    """on a generated factor: X.(L.U) == B on the rows with ok, the rows with an entry in a column without a pivot have none"""
    from test_solve_host import dense, mulmod
    p = 4294967291
    rng = np.random.default_rng(4)
    # (U's rows in order: out of order the reference's forward loop no longer clears every combination of them; no entries of
    #  L that the reference ignores: with them X solves another system than X.(L.U) = B)
    U, qinv, L, Lp = sc.layered(rng, p, *sc.STRUCTURES["runs"], *sc.STRUCTURES["sweep"], ncheck=7, extra_rows=9, nonpivot=True)
    B = sc.right_hand_sides(rng, p, U, qinv, L, 12)
    X, ok = sc.model_gesv(U, qinv, L, Lp, B, p)
    assert ok[0::2].all() and not ok[1:10:2].any()
    assert X.p[11] == X.p[10]                                       # the zero row
    assert len(set(B.row(11)[0].tolist())) == len(B.row(11)[0]) - 1  # the repeated column
    A = mulmod(dense(L), dense(U), p)
    XA = mulmod(dense(X), A, p)
    assert np.array_equal(XA[ok], dense(B)[ok])
    for t in range(12):
        assert np.all(np.diff(X.row(t)[0]) > 0) and set(X.row(t)[0].tolist()) <= set(Lp.tolist())
