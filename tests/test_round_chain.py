"""
The sumcheck verifier's round chain and its interpolation (zkhip.verify.round_chain / round_poly_at), the one copy every protocol
module calls: against the models' independent interpolations, and on honest and tampered chains for every node count in use.
No GPU, no library: python integers only.
"""
import random

import numpy as np
import pytest

import plonk_model as pm
import wiring_model as wm
import zerocheck_model as zm
from zkhip import plonk, verify, wiring, zerocheck
from zkhip.field import R_MOD as R

N_ROUNDS = 3
NODE_COUNTS = (3, 4, 5, 6, 8)  # batch opening, wiring / lookup, gate, perm3, wide gate


# ---- interpolation ----
@pytest.mark.parametrize("K", range(3, 9))
def test_round_poly_at_is_the_models_interpolation(K):
    rng = random.Random(100 + K)
    ev, x = [rng.randrange(R) for _ in range(K)], rng.randrange(R)
    got = verify.round_poly_at(ev, x)
    assert got == pm.interpolate(ev, x)
    if K == 3:
        assert got == verify.product_round_target(*ev, x)
    if K == 4:
        assert got == wm.interpolate4(ev, x)
    if K == 5:
        assert got == zm.interpolate5(ev, x)
    for k in range(K):
        assert verify.round_poly_at(ev, k) == ev[k]


def test_round_poly_at_beyond_the_range_of_machine_integers():
    """the denominators are products of up to K - 1 node differences: past 21 nodes they leave 64 bits"""
    for K in (22, 30):
        rng = random.Random(200 + K)
        ev, x = [rng.randrange(R) for _ in range(K)], rng.randrange(R)
        assert verify.round_poly_at(ev, x) == pm.interpolate(ev, x)
        assert verify.round_poly_at(ev, K - 1) == ev[K - 1]


def test_one_interpolation_under_every_name():
    assert zerocheck.round_poly_at is verify.round_poly_at
    assert wiring.round_poly_at is verify.round_poly_at
    assert plonk.round_poly_at is verify.round_poly_at
    assert zerocheck._ints is verify._ints and zerocheck.eq_eval is verify.eq_eval


def test_round_poly_at_refuses_fewer_than_two_nodes():
    for ev in ([], [5]):
        with pytest.raises(ValueError):
            verify.round_poly_at(ev, 3)


# ---- the chain ----
def _poly_at(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


def _honest_chain(K, claimed, seed):
    """n rounds of random polynomials of degree K - 1 whose constant terms are fixed to meet each target -> (rounds as ints, chal, last)"""
    rng = random.Random(seed)
    inv2 = pow(2, -1, R)
    rounds, chal, target = [], [], claimed % R
    for _ in range(N_ROUNDS):
        hi = [rng.randrange(R) for _ in range(K - 1)]  # c_1 .. c_{K-1};  p(0) + p(1) = 2 c_0 + sum hi
        coeffs = [(target - sum(hi)) * inv2 % R] + hi
        rounds.append([_poly_at(coeffs, k) for k in range(K)])
        chal.append(rng.randrange(R))
        target = _poly_at(coeffs, chal[-1])
    return rounds, chal, target


def _limbs(rows):
    return np.stack([zm.mont(r) for r in rows])


@pytest.mark.parametrize("claimed", [0, 0x1234567 << 200])
@pytest.mark.parametrize("K", NODE_COUNTS)
def test_round_chain_accepts_an_honest_chain(K, claimed):
    rounds, chal, last = _honest_chain(K, claimed, 7 * K)
    assert (rounds[0][0] + rounds[0][1]) % R == claimed % R
    assert verify.round_chain(rounds, chal, claimed) == last
    # the same on Montgomery limbs, the form the records hold
    assert verify.round_chain(_limbs(rounds), zm.mont(chal), claimed) == last
    if claimed == 0:
        assert verify.round_chain(rounds, chal) == last


@pytest.mark.parametrize("K", NODE_COUNTS)
def test_round_chain_on_every_single_changed_evaluation(K):
    rounds, chal, last = _honest_chain(K, 0, 11 * K)
    for i in range(N_ROUNDS):
        for k in range(K):
            bad = [list(r) for r in rounds]
            bad[i][k] = (bad[i][k] + 1) % R
            got = verify.round_chain(bad, chal)
            if k < 2 or i < N_ROUNDS - 1:
                # p_i(0) + p_i(1) misses its target, or p_i(r_i) moves (the basis polynomial of node k >= 2 vanishes only at the
                # other nodes, and r_i is none of them) and round i + 1 misses
                assert got is None, (i, k)
            else:
                assert got is not None and got != last, (i, k)


@pytest.mark.parametrize("K", NODE_COUNTS)
def test_round_chain_refuses_a_wrong_claim_and_a_count_mismatch(K):
    rounds, chal, last = _honest_chain(K, 5, 13 * K)
    assert verify.round_chain(rounds, chal, 5) == last
    assert verify.round_chain(rounds, chal, 6) is None
    assert verify.round_chain(rounds, chal) is None
    with pytest.raises(ValueError):
        verify.round_chain(rounds, chal[:-1], 5)
    with pytest.raises(ValueError):
        verify.round_chain(_limbs(rounds)[:-1], zm.mont(chal), 5)
