"""CPU checks of tests/modulus_edges.py: the primes are prime and straddle their switches, the switches are still where the
table says, and the star factors' closed-form Schur complements are what the oracle computes."""
import os

import numpy as np
import pytest

import modulus_edges as me

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "spasm_amd", "csrc")


def test_is_prime():
    small = [q for q in range(200) if me.is_prime(q)]
    assert small == [q for q in range(2, 200) if all(q % d for d in range(2, q))]
    assert me.is_prime(4294967291) and not me.is_prime(4294967293) and not me.is_prime(65535)


@pytest.mark.parametrize("q", me.EDGE_PRIMES + [p for p, _ in me.MAXDEG_PAIRS] + [800011, 1100009])
def test_listed_moduli_are_prime(q):
    assert me.is_prime(q)


@pytest.mark.parametrize("regime", me.REGIMES, ids=[r[0] for r in me.REGIMES])
def test_pairs_straddle_their_switch_with_no_prime_between(regime):
    name, _, _, below_side, (lo, hi) = regime
    assert lo < hi
    assert below_side(lo) and not below_side(hi), name
    assert not any(me.is_prime(q) for q in range(lo + 1, hi))


@pytest.mark.parametrize("regime", me.REGIMES, ids=[r[0] for r in me.REGIMES])
def test_source_expression_is_still_there(regime):
    """a moved or changed threshold fails here first: update the table (and the GPU tests built on it) with it"""
    name, path, expr, _, _ = regime
    with open(os.path.join(CSRC, path)) as f:
        assert expr in f.read(), "%s: `%s` no longer in spasm_amd/csrc/%s" % (name, expr, path)


@pytest.mark.parametrize("path,expr", me.MAXDEG_SOURCES)
def test_maxdeg_expressions_are_still_there(path, expr):
    with open(os.path.join(CSRC, path)) as f:
        assert expr in f.read()


def test_extreme_primes():
    """3 is the smallest odd prime; 4294967291 = 0xfffffffb, the largest prime below 2^32 (the bound spmv.hip takes)"""
    assert 4294967291 == 0xfffffffb
    assert not any(me.is_prime(q) for q in range(4294967292, 1 << 32))


def test_lds_slot_bound():
    """the large LDS table (8,192 slots) allows CAPK keys before a batch of 64: at most 6,144 terms plus the row's own
    entry reach a slot -- the 6146 of wide_lds"""
    H = 8192
    capk = (H * 3) // 4 - 64
    assert capk + 64 + 1 < 6146


def test_maxdeg_pairs():
    by_p = {}
    for p, K in me.MAXDEG_PAIRS:
        by_p.setdefault(p, []).append(K)
    # at 195,225,781 the choice flips between K = 8 and K = 9
    assert me.narrow_dense(195225781, 8) and not me.narrow_dense(195225781, 9)
    # the wide cases beyond it hold data whose exact sum would wrap a 32-bit accumulator
    for p, K in me.MAXDEG_PAIRS[2:]:
        assert not me.narrow_dense(p, K) and K * (p - 1) >= me.TWO32


@pytest.mark.parametrize("p", me.EDGE_PRIMES)
@pytest.mark.parametrize("K,C,x,u", [(7, 1, 1, 1), (40, 3, -1, 1), (33, 2, "h", "h"), (33, 2, "-h", "h")])
def test_star_closed_form_equals_the_oracle(oracle, p, K, C, x, u):
    h = me.half(p)
    val = {"h": h, "-h": -h}
    x, u = val.get(x, x), val.get(u, u)
    n, m, ti, tj, tx, want = me.star(p, K, C=C, nred=5, x=x, u=u, a_seed=K + C)
    A, F, rows = me.star_factor(oracle, p, n, m, K, ti, tj, tx)
    S, p_out, _ = oracle.schur(A, rows, F)
    assert np.array_equal(p_out, rows)
    assert np.array_equal(me.dense_of_sparse_rows(S, K, C), want)
    D, q, _ = oracle.schur_dense(A, rows, F)
    assert np.array_equal(np.asarray(q, np.int64), np.arange(K, K + C))
    assert np.array_equal(np.mod(D, p), want)
