"""
Aggregated PCS verification without a GPU:
  * zk_pcs_agg_weights through the ABI against the model's hashlib derivation (pcs_agg_model.weights), and its sensitivity to every
    input word;
  * the model's aggregate equation in the exponent, with the sampler's trapdoor: it holds for honest openings of mixed shapes and
    fails for one flipped value (and holds for the compensating forgery exactly when the weights are equal);
  * batch_open.opening_claim against what batch_open_verify hands to the device.
"""
import random

import numpy as np
import pytest

import batch_open_model as bm
import pcs_agg_model as am

R = am.R


def _arrays(shapes, seed):
    """random words in the shape of the ABI's arrays for openings of (nvars, skip, J): only the hash reads them"""
    rng = np.random.default_rng(seed)
    w = lambda *s: rng.integers(0, 2**64, size=s, dtype=np.uint64)
    nvars = np.array([s[0] for s in shapes], dtype=np.uint64)
    skip = np.array([s[1] for s in shapes], dtype=np.uint64)
    cstart = np.cumsum([0] + [s[2] for s in shapes]).astype(np.uint64)
    rows, terms = int(nvars.sum()), int(cstart[-1])
    return [nvars, skip, cstart, w(terms, 18), w(terms, 4), w(len(shapes), 4), w(rows, 18), w(rows, 4)]


SHAPES = {0: [], 1: [(3, 1, 1)], 3: [(4, 0, 1), (3, 1, 7), (0, 2, 0)]}


@pytest.mark.parametrize("count", [0, 1, 3])
def test_weights_through_the_abi_equal_the_hashlib_derivation(count):
    import zkhip

    args = _arrays(SHAPES[count], 10 + count)
    got = zkhip.Ctx.pcs_agg_weights(*args)
    assert got.shape == (count, 2)
    want = am.weights(*args)
    assert [int(lo) | int(hi) << 64 for lo, hi in got] == want
    assert (zkhip.Ctx.pcs_agg_weights(*args) == got).all()  # deterministic
    if count:
        assert len(set(want)) == count and all(r >> 64 for r in want)


def test_any_single_input_word_changes_every_weight():
    import zkhip

    args = _arrays(SHAPES[3], 99)
    base = zkhip.Ctx.pcs_agg_weights(*args)
    rng = random.Random(5)
    for which in range(3, 8):  # EVERY word of every data array, one random bit of it
        for pos in range(args[which].size):
            mod = [a.copy() for a in args]
            mod[which].reshape(-1)[pos] ^= np.uint64(1) << np.uint64(rng.randrange(64))
            got = zkhip.Ctx.pcs_agg_weights(*mod)
            assert (got != base).any(axis=1).all(), (which, pos)
            assert [int(lo) | int(hi) << 64 for lo, hi in got] == am.weights(*mod)
    # the shape words: nvars / skip / J moved between openings with every array's total length unchanged
    for mod_shapes in ([(3, 0, 1), (4, 1, 7), (0, 2, 0)], [(4, 1, 1), (3, 1, 7), (0, 2, 0)], [(4, 0, 2), (3, 1, 6), (0, 2, 0)]):
        mod = _arrays(mod_shapes, 99)
        mod[3:] = [a.copy() for a in args[3:]]
        got = zkhip.Ctx.pcs_agg_weights(*mod)
        assert (got != base).any(axis=1).all(), mod_shapes
    # offsets that do not start at 0 or decrease are refused
    for cs in ([1, 1, 8, 8], [0, 8, 1, 8]):
        mod = [a.copy() for a in args]
        mod[2] = np.array(cs, dtype=np.uint64)
        with pytest.raises(zkhip.ZkError):
            zkhip.Ctx.pcs_agg_weights(*mod)


# ---- the aggregate equation in the exponent ----
def _honest(rng, s_keys, nvars, skip, J):
    """one opening as discrete logarithms: random proof points, point and value; the commitment is what makes
    C - v = sum_i (s_{skip+i} - u_i) pi_i hold, split into J terms sum_j e_j C_j (J = 0 only fits a commitment of 0: not sampled)"""
    pis, us, v = [rng.randrange(R) for _ in range(nvars)], [rng.randrange(R) for _ in range(nvars)], rng.randrange(R)
    c = (v + sum((s_keys[skip + i] - u) * p for i, (u, p) in enumerate(zip(us, pis)))) % R
    terms = [(rng.randrange(R), rng.randrange(1, R)) for _ in range(J - 1)]
    e_last = rng.randrange(1, R)
    terms.append(((c - sum(C * e for C, e in terms)) * pow(e_last, -1, R) % R, e_last))
    return (nvars, skip, terms, v, pis, us)


def test_aggregate_equation_in_the_exponent():
    rng = random.Random(77)
    s_keys = [rng.randrange(1, R) for _ in range(5)]  # powers_g2 = [g2, s_0 g2, .., s_4 g2]
    ops = [_honest(rng, s_keys, 5, 0, 1), _honest(rng, s_keys, 4, 1, 10), _honest(rng, s_keys, 4, 1, 7), _honest(rng, s_keys, 3, 2, 2),
           _honest(rng, s_keys, 0, 0, 1), _honest(rng, s_keys, 1, 4, 3)]
    for count in (1, 2, len(ops)):
        rho = [rng.randrange(1, 2**128) for _ in range(count)]
        assert am.aggregate_holds_in_exponent(s_keys, ops[:count], rho)
        for k in range(count):  # one flipped value, one moved proof point, one changed commitment scalar
            nv, sk, terms, v, pis, us = ops[k]
            muts = [(nv, sk, terms, v ^ 1, pis, us), (nv, sk, [(terms[0][0], (terms[0][1] + 1) % R)] + terms[1:], v, pis, us)]
            if nv:
                muts.append((nv, sk, terms, v, [(pis[0] + 1) % R] + pis[1:], us))
                muts.append((nv, sk, terms, v, pis, us[:-1] + [(us[-1] + 1) % R]))
            for m in muts:
                assert not am.aggregate_holds_in_exponent(s_keys, ops[:k] + [m] + ops[k + 1:count], rho)
    # the term list: every input point once in L, every proof point once more in its M_j, g1 last in L
    starts, pts, ks = am.term_list(6, ops, [1] * len(ops), "g1")
    n_pts = sum(len(o[2]) + o[0] for o in ops)
    assert starts[0] == 0 and starts[1] == n_pts + 1 and pts[starts[1] - 1] == "g1" and starts[-1] == n_pts + 1 + sum(o[0] for o in ops)
    assert [starts[j + 1] - starts[j] for j in range(1, 6)] == [sum(1 for o in ops if o[1] < j <= o[1] + o[0]) for j in range(1, 6)]


def test_compensating_forgery_passes_equal_weights_only():
    rng = random.Random(78)
    s_keys = [rng.randrange(1, R) for _ in range(4)]
    a, b = _honest(rng, s_keys, 3, 1, 1), _honest(rng, s_keys, 3, 1, 1)
    d = rng.randrange(1, R)
    shift = lambda o, x: (o[0], o[1], [((o[2][0][0] * o[2][0][1] + x) * pow(o[2][0][1], -1, R) % R, o[2][0][1])], *o[3:])
    fa, fb = shift(a, d), shift(b, -d)
    assert not am.aggregate_holds_in_exponent(s_keys, [fa], [1]) and not am.aggregate_holds_in_exponent(s_keys, [fb], [1])
    assert am.aggregate_holds_in_exponent(s_keys, [fa, fb], [1, 1])
    assert am.aggregate_holds_in_exponent(s_keys, [fa, fb], [5, 5])
    assert not am.aggregate_holds_in_exponent(s_keys, [fa, fb], [1, 2])


# ---- opening_claim ----
class _Recorder:
    """a backend that records what batch_open_verify hands to the device"""

    def g1_lincomb(self, points, scalars_canon):
        self.comms, self.e_canon = np.array(points), np.array(scalars_canon)
        return np.arange(18, dtype=np.uint64)  # (a marker for C_g)

    def pcs_verify_batch(self, vk, commitments, values, proofs, points):
        self.cg, self.y, self.opening, self.rho = (np.array(x) for x in (commitments, values, proofs, points))
        return np.array([True])


@pytest.mark.parametrize("n,J,K", [(2, 1, 5), (4, 3, 7), (5, 4, 9)])
def test_opening_claim_is_what_batch_open_verify_computes(n, J, K):
    from zkhip import batch_open as bo

    tables, claims, alpha, rho = bm.instance(n, J, K, 400 + n)
    rec, _ = bm.prove(tables, claims, alpha, rho)
    rec["opening"] = np.random.default_rng(n).integers(0, 2**64, size=(n, 18), dtype=np.uint64)
    comms = np.random.default_rng(n + 1).integers(0, 2**64, size=(J, 18), dtype=np.uint64)
    cm, al, rm = bm.claims_mont(claims), bm.mont([alpha])[0], bm.mont(rho)
    be = _Recorder()
    assert bo.batch_open_verify(be, None, comms, cm, rec, al, rm) is True
    C, e, y, opening, r = bo.opening_claim(comms, cm, rec, al, rm)
    assert (C == be.comms).all() and (be.cg.reshape(-1) == np.arange(18)).all()
    assert am.fr_ints(e) == [sum(int(w) << (64 * i) for i, w in enumerate(row)) for row in be.e_canon] == bm.eq_coefficients(J, claims, alpha, rho)
    assert (y == be.y.reshape(4)).all() and (opening == be.opening.reshape(n, 18)).all() and (r == be.rho.reshape(n, 4)).all()
    # a broken chain: no claim, as batch_open_verify refuses before the device
    bad = {"rounds": rec["rounds"].copy(), "opening": rec["opening"]}
    bad["rounds"][0][2][1] ^= np.uint64(1)
    assert bo.opening_claim(comms, cm, bad, al, rm) is None and bo.batch_open_verify(_Recorder(), None, comms, cm, bad, al, rm) is False
