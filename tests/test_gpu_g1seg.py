"""
zk_g1_lincomb_seg (csrc/zk_g1seg.hip) against the integer model (pcs_agg_model.py: affine chord-and-tangent arithmetic), bit for bit on
the normalised output.  Segment lengths around the wavefront (63, 64, 65), the workgroup (256, 257) and the partials path (600), with
an empty first and last segment; the named scalars; the points that only a complete addition sums correctly; and the refusals, which
are a status of the call and never a fault.
"""
import random

import numpy as np
import pytest

import pcs_agg_model as am
import zkhip
from zkhip._lib import ZK_ERR_INVALID

pytestmark = pytest.mark.gpu

Q, R, G = am.Q, am.R, am.G
LENGTHS = [0, 1, 2, 63, 64, 65, 256, 257, 600, 0]
SCALARS = [0, 1, 2, 2**64, 2**128 - 1, 2**128, R - 1, 2**254]


def _pool(rng, n):
    """n points of G1 by a walk: P_0 = [k]G, P_i = P_{i-1} + [small]G"""
    steps = [am.mul(G, j) for j in range(1, 9)]
    pts = [am.mul(G, rng.randrange(1, R))]
    while len(pts) < n:
        pts.append(am.add(pts[-1], steps[rng.randrange(8)]))
    return pts


def _run(ctx, starts, terms):
    """terms: [(record [18], affine point or None, scalar)] -> (device output, the model's records)"""
    got = ctx.g1_lincomb_seg(starts, np.stack([t[0] for t in terms]), np.stack([am.canon_limbs(t[2]) for t in terms]))
    want = np.stack([am.words(P) for P in am.seg_sum(starts, [t[1] for t in terms], [t[2] for t in terms])])
    return got, want


def test_segment_lengths_against_the_model(ctx):
    rng = random.Random(2025)
    pool = _pool(rng, 48)
    starts = [0]
    for n in LENGTHS:
        starts.append(starts[-1] + n)
    terms = []
    for t in range(starts[-1]):
        P = pool[rng.randrange(len(pool))]
        k = rng.randrange(R) if t % 16 == 0 else rng.randrange(1 << 20)  # (one full-length scalar sets the trip count of every lane)
        rec = am.jac_words(P, rng.randrange(1, Q)) if t % 3 else am.words(P)
        terms.append((rec, P, k))
    got, want = _run(ctx, starts, terms)
    assert got.shape == (len(LENGTHS), 18)
    for s in range(len(LENGTHS)):
        assert (got[s] == want[s]).all(), (s, LENGTHS[s])
    assert (got[0] == am.words(None)).all() and (got[-1] == am.words(None)).all()  # the empty segments
    assert (ctx.g1_lincomb_seg(starts, np.stack([t[0] for t in terms]), np.stack([am.canon_limbs(t[2]) for t in terms])) == got).all()


def test_named_scalars(ctx):
    rng = random.Random(7)
    pool = _pool(rng, 4)
    # one segment per scalar, then all of them in one segment, then short calls whose largest scalar is each of them in turn
    terms = [(am.words(pool[i % 4]), pool[i % 4], k) for i, k in enumerate(SCALARS)]
    starts = list(range(len(SCALARS) + 1)) + [2 * len(SCALARS)]
    got, want = _run(ctx, starts, terms + terms)
    assert (got == want).all()
    assert (got[0] == am.words(None)).all() and (got[1] == am.words(pool[1])).all()
    for k in SCALARS:
        t = [(am.words(pool[0]), pool[0], k), (am.words(pool[1]), pool[1], k >> 1), (am.words(pool[2]), pool[2], 1)]
        got, want = _run(ctx, [0, 3], t)
        assert (got == want).all(), hex(k)


def test_points_that_need_the_complete_addition(ctx):
    rng = random.Random(11)
    P, S = _pool(rng, 2)
    k = rng.randrange(R)
    inf_rec = am.raw_words(rng.randrange(Q), rng.randrange(Q), 0)  # Z = 0 with arbitrary X, Y: infinity
    rep = lambda T: am.jac_words(T, rng.randrange(1, Q))
    cases = {
        "z=0": [(inf_rec, None, 5), (am.words(S), S, 3)],
        "only z=0": [(inf_rec, None, k)],
        "representatives": [(rep(P), P, k), (rep(P), P, 7), (rep(S), S, k)],
        "twice": [(am.words(P), P, 1), (am.words(P), P, 1)],
        "twice, other representative": [(am.words(P), P, k), (rep(P), P, k)],
        "P and -P": [(am.words(P), P, 1), (am.words(am.neg(P)), am.neg(P), 1)],
        "kP and -kP": [(rep(P), P, k), (am.words(am.neg(P)), am.neg(P), k)],
        "P, P, -2P": [(am.words(P), P, 1), (rep(P), P, 1), (am.words(am.neg(am.add(P, P))), am.neg(am.add(P, P)), 1)],
        "P, P, -P scaled": [(am.words(P), P, k), (am.words(P), P, k), (rep(am.neg(P)), am.neg(P), 2 * k % R)],
    }
    starts, terms = [0], []
    for c in cases.values():
        terms += c
        starts.append(len(terms))
    got, want = _run(ctx, starts, terms)
    for s, name in enumerate(cases):
        assert (got[s] == want[s]).all(), name
    for name in ("only z=0", "P and -P", "kP and -kP", "P, P, -2P", "P, P, -P scaled"):
        assert (got[list(cases).index(name)] == am.words(None)).all(), name
    assert (got[list(cases).index("twice")] == am.words(am.add(P, P))).all()


def test_bad_terms_are_refused_by_status(ctx):
    rng = random.Random(13)
    pool = _pool(rng, 5)
    good = [am.words(T) for T in pool]
    x, y = pool[0]
    over_q = am.raw_words(Q + 5, (y << 384) % Q, 1)  # a coordinate >= q
    off_curve = am.words((x, (y + 1) % Q))
    ks = np.stack([am.canon_limbs(rng.randrange(1 << 16)) for _ in range(5)])
    for bad, what in ((over_q, "canonical"), (off_curve, "curve")):
        for pos in (0, 4):
            recs = [r.copy() for r in good]
            recs[pos] = bad
            with pytest.raises(zkhip.ZkError) as e:
                ctx.g1_lincomb_seg([0, 2, 5], np.stack(recs), ks)
            assert e.value.code == ZK_ERR_INVALID and f"term {pos}:" in str(e.value) and what in str(e.value), str(e.value)
    recs = [good[0], off_curve, good[2], over_q, good[4]]  # two bad terms: the smallest is named
    with pytest.raises(zkhip.ZkError) as e:
        ctx.g1_lincomb_seg([0, 2, 5], np.stack(recs), ks)
    assert "term 1:" in str(e.value) and "curve" in str(e.value)
    bad_k = ks.copy()
    bad_k[3] = am.canon_limbs(R)  # a scalar that is not canonical, after a bad point and before one
    with pytest.raises(zkhip.ZkError) as e:
        ctx.g1_lincomb_seg([0, 2, 5], np.stack([good[0], good[1], good[2], good[3], off_curve]), bad_k)
    assert e.value.code == ZK_ERR_INVALID and "term 3:" in str(e.value) and "scalar" in str(e.value)
    with pytest.raises(zkhip.ZkError) as e:
        ctx.g1_lincomb_seg([0, 2, 5], np.stack(recs), bad_k)
    assert "term 1:" in str(e.value)
    with pytest.raises(zkhip.ZkError):
        ctx.g1_lincomb_seg([0, 3, 2], np.stack(good), ks)  # offsets that decrease
    # the call after a refusal is a normal one, and an empty call returns nothing
    assert (ctx.g1_lincomb_seg([0, 5], np.stack(good), ks)[0] == am.words(am.seg_sum([0, 5], pool, [int(k[0]) for k in ks])[0])).all()
    assert ctx.g1_lincomb_seg([], np.zeros((0, 18), np.uint64), np.zeros((0, 4), np.uint64)).shape == (0, 18)
    assert (ctx.g1_lincomb_seg([0, 0], np.zeros((0, 18), np.uint64), np.zeros((0, 4), np.uint64))[0] == am.words(None)).all()
