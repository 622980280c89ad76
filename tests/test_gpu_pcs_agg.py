"""
zk_pcs_verify_agg (csrc/zk_pairing.hip) against zk_pcs_verify_batch: the aggregate's verdict is the AND of the per-opening verdicts of
the existing, unchanged verifier.  Real openings from the commit / open path at 3 and 4 variables over ONE 4-variable SRS (the
3-variate ones use its last three keys: skip = 1), commitments given as one term or as a sum of two.  Then the compensating forgery,
which equal weights let through and the derived weights do not, and the refusals.
"""
import numpy as np
import pytest

import pcs_agg_model as am
import pyoracle as po
import zkhip
from helpers import jac_norm_to_affine, pt_ints, rand_fr
from zkhip import dist_primitive as dp
from zkhip import pairing as pr
from zkhip._lib import ZK_ERR_INVALID

pytestmark = pytest.mark.gpu

R = po.R_MOD


def _mont(xs):
    return np.array([po.fr_to_mont_limbs(x) for x in xs], dtype=np.uint64).reshape(-1, 4)


def _jac(P):
    one = po.fq_to_mont_limbs(1)
    return np.array(one + one + [0] * 6 if P is None else po.fq_to_mont_limbs(P[0]) + po.fq_to_mont_limbs(P[1]) + one, dtype=np.uint64)


def _plus(rec, T):
    """the normalised record of (the record's point) + T"""
    return _jac(po.g1_add(pt_ints(jac_norm_to_affine(np.asarray(rec, dtype=np.uint64))), T))


@pytest.fixture(scope="module")
def setup(ctx):
    """(vk of the 4-variable SRS, vk of its last three keys, seven honest openings: four of 4 variables, three of 3 with skip = 1).
    An opening is (C [J, 18], e [J] integers, value [4], proofs [n, 18], point [n] integers, skip); openings 1 and 5 give their
    commitment as e C + (1 - e) C"""
    rng = po.SplitMix64(2718)
    s = rng.fr_vec(4)
    cubs = {4: dp.PolynomialCommitmentCub.new(ctx, _mont(s)), 3: dp.PolynomialCommitmentCub.new(ctx, _mont(s[1:]))}
    vks = {4: dp.pcs_vk(ctx, pr.powers_of_g2(s)), 3: dp.pcs_vk(ctx, pr.powers_of_g2(s[1:]))}
    ops = []
    for k, n in enumerate([4, 3, 4, 3, 4, 3, 4]):
        u = rng.fr_vec(n)
        d_poly = ctx.to_device(rand_fr(1 << n, 500 + k))
        C = np.asarray(dp.commit(ctx, cubs[n].mature(), d_poly, 1 << n), dtype=np.uint64).reshape(1, 18)
        value, proofs = dp.open_(ctx, cubs[n].mature(), d_poly, 1 << n, _mont(u))
        e = [1]
        if k in (1, 5):
            e0 = rng.fr()
            C, e = np.concatenate([C, C]), [e0, (1 - e0) % R]
        ops.append((C, e, np.asarray(value, dtype=np.uint64).reshape(4), np.asarray(proofs, dtype=np.uint64).reshape(n, 18), list(u), 4 - n))
    return vks, ops


def _agg(ctx, vks, ops, rho=None) -> bool:
    return dp.verify_agg(ctx, vks[4], [(C, _mont(e), v, pf, _mont(u), skip) for C, e, v, pf, u, skip in ops], rho=rho)


def _each(ctx, vks, ops) -> list:
    """the yardstick: zk_pcs_verify_batch on every opening, its commitment summed by zk_g1_lincomb"""
    out = []
    for C, e, v, pf, u, skip in ops:
        n = len(pf)
        cg = ctx.g1_lincomb(C, np.stack([am.canon_limbs(x) for x in e]))
        out.append(bool(dp.verify_batch(ctx, vks[n], cg.reshape(1, 18), v.reshape(1, 4), pf.reshape(1, n, 18), _mont(u).reshape(1, n, 4))[0]))
    return out


def _mutations(op):
    C, e, v, pf, u, skip = op
    T = po.g1_mul(po.G1_GEN, 12345)
    out = {"value": (C, e, _mont([(po.fr_from_mont_limbs(v) + 1) % R])[0], pf, u, skip)}
    C2 = C.copy()
    C2[-1] = _plus(C[-1], T)
    out["commitment term"] = (C2, e, v, pf, u, skip)
    out["commitment scalar"] = (C, e[:-1] + [(e[-1] + 1) % R], v, pf, u, skip)
    for i in range(len(pf)):
        p2 = pf.copy()
        p2[i] = _plus(pf[i], T)
        out[f"proof point {i}"] = (C, e, v, p2, u, skip)
        out[f"point coordinate {i}"] = (C, e, v, pf, u[:i] + [(u[i] + 1) % R] + u[i + 1:], skip)
    return out


@pytest.mark.parametrize("count", [1, 2, 7])
def test_honest_batches(ctx, setup, count):
    vks, ops = setup
    sel = ops[:count]
    assert _each(ctx, vks, sel) == [True] * count
    assert _agg(ctx, vks, sel) is True
    if count == 2:  # also the 3-variate opening alone, and with explicit weights
        assert _agg(ctx, vks, ops[1:2]) is True
        assert _agg(ctx, vks, sel, rho=np.array([[3, 0], [2**64 - 1, 2**64 - 1]], dtype=np.uint64)) is True


@pytest.mark.parametrize("which", [0, 1])
def test_one_change_at_a_time(ctx, setup, which):
    """openings 0 (4 variables, one commitment term) and 1 (3 variables, skip 1, two terms) mutated inside a batch of three"""
    vks, ops = setup
    for name, mut in _mutations(ops[which]).items():
        batch = ops[:which] + [mut] + ops[which + 1:3]
        each = _each(ctx, vks, batch)
        assert each == [k != which for k in range(3)], name
        assert _agg(ctx, vks, batch) is all(each), name


def test_compensating_forgery(ctx, setup):
    vks, ops = setup
    a, b = ops[0], ops[2]  # two honest openings of equal shape
    D = po.g1_mul(po.G1_GEN, po.SplitMix64(99).fr())
    fa = (np.stack([_plus(a[0][0], D)]),) + a[1:]
    fb = (np.stack([_plus(b[0][0], (D[0], (-D[1]) % po.Q_MOD))]),) + b[1:]
    assert _each(ctx, vks, [fa, fb]) == [False, False]
    assert _agg(ctx, vks, [fa, fb], rho=np.array([[1, 0], [1, 0]], dtype=np.uint64)) is True  # what unweighted aggregation lets through
    assert _agg(ctx, vks, [fa, fb]) is False
    assert _agg(ctx, vks, [fa, fb], rho=np.array([[1, 0], [2, 0]], dtype=np.uint64)) is False


def test_weights_are_the_models(ctx, setup):
    vks, ops = setup
    arrays = dp.agg_arrays([(C, _mont(e), v, pf, _mont(u), skip) for C, e, v, pf, u, skip in ops])
    rho = ctx.pcs_agg_weights(*arrays)
    assert [int(lo) | int(hi) << 64 for lo, hi in rho] == am.weights(*arrays)
    assert ctx.pcs_verify_agg(vks[4], *arrays, rho=rho) is True


def test_empty_call_and_refusals(ctx, setup):
    vks, ops = setup
    assert _agg(ctx, vks, []) is True
    C, e, v, pf, u, skip = ops[0]
    for bad in ((C, e, v, pf, u, 1), (ops[1][:5] + (2,))):  # nvars + skip beyond the key
        with pytest.raises(zkhip.ZkError) as err:
            _agg(ctx, vks, [ops[2], bad])
        assert err.value.code == ZK_ERR_INVALID and "opening 1" in str(err.value)
    off = pf.copy()
    off[2][6] ^= np.uint64(1)  # a proof point off the curve: named by opening and index
    with pytest.raises(zkhip.ZkError) as err:
        _agg(ctx, vks, [ops[1], (C, e, v, off, u, skip)])
    assert err.value.code == ZK_ERR_INVALID and "proof point 2 of opening 1" in str(err.value)
    assert _agg(ctx, vks, ops[:2]) is True  # the call after a refusal is a normal one
