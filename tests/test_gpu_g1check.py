"""
zk_g1_decompress_check and zk_g1_check (csrc/zk_g1check.hip) against the integer model (g1check_model.py), bit for bit: the model
decides membership by the definition [r]P = O, the kernels by the endomorphism.  Every batch mixes the four statuses so the lanes of
one wave diverge; every status stands at lane 0 and at the last lane of some batch; the degenerate points (order 3 and 11, cofactor
parts, T + G, infinity) are in every batch above the smallest.
"""
import ctypes
import random

import numpy as np
import pytest

import g1check_model as gm

pytestmark = pytest.mark.gpu

COUNTS = [1, 2, 63, 64, 65, 300]


def _batch(count, first, last, seed):
    """count encodings: status `first` at lane 0, `last` at the last lane, the rest drawn from all cases, every case present when it fits"""
    pool = gm.by_status(1)
    rng = random.Random(seed)
    every = [e for _, e in gm.cases(1)]
    rng.shuffle(every)
    body = [every[i % len(every)] if i < len(every) else rng.choice(every) for i in range(count)]
    rng.shuffle(body)
    body[0] = rng.choice(pool[first])
    body[-1] = rng.choice(pool[last]) if count > 1 else body[0]
    return body


@pytest.mark.parametrize("count", COUNTS)
def test_decompress_check_matches_the_model(ctx, count):
    for status in range(4):
        encs = _batch(count, status, (status + 1) % 4 if count > 1 else status, 100 * count + status)
        want_pts, want_st = gm.expected(encs)
        if count >= 63:
            assert set(want_st.tolist()) == {0, 1, 2, 3}
        pts, st = ctx.g1_decompress_check(b"".join(encs))
        assert st.tolist() == want_st.tolist(), (count, status)
        assert (pts == want_pts).all(), (count, status)
        assert ctx.g1_decompress_check(np.frombuffer(b"".join(encs), dtype=np.uint8).reshape(count, 48))[1].tolist() == want_st.tolist()


def test_named_points_one_by_one(ctx):
    """each case alone in a call of its own lane 0 (a wave of one active lane), and all of them in one call"""
    encs = [e for _, e in gm.cases(1)]
    want_pts, want_st = gm.expected(encs)
    pts, st = ctx.g1_decompress_check(b"".join(encs))
    bad = [(n, int(a), int(b)) for (n, _), a, b in zip(gm.cases(1), st, want_st) if a != b]
    assert not bad, bad
    assert (pts == want_pts).all()
    for (name, e), w, s in zip(gm.cases(1), want_pts, want_st):
        if name.startswith(("order", "cofactor", "infinity", "inf+", "x=")):
            p1, s1 = ctx.g1_decompress_check(e)
            assert int(s1[0]) == int(s) and (p1[0] == w).all(), name


def _jac_cases():
    """(18 words, the model's status): every on-curve case as the normalised record and as another representative, infinity in several
    forms, a coordinate equal to q, a point off the curve"""
    rng = random.Random(77)
    out = []
    for name, e in gm.cases(1):
        s, P = gm.decompress_check(e)
        if s in (gm.OK, gm.NOT_IN_G1):
            out.append(gm.words(P))
            if P is not None:
                out.append(gm.jac_words(P, rng.randrange(2, gm.Q)))
    G2 = gm.mul(gm.G, 2)
    inf_any = gm.jac_words(G2, 5)
    inf_any[12:] = 0  # Z = 0 whatever X and Y are
    out.append(inf_any)
    qw = np.array([(gm.Q >> (64 * i)) & (2**64 - 1) for i in range(6)], dtype=np.uint64)
    for k in range(3):  # a coordinate equal to q: not canonical
        w = gm.words(G2)
        w[6 * k:6 * k + 6] = qw
        out.append(w)
    w = gm.words(G2)
    w[12:] = 2**64 - 1
    out.append(w)
    off = gm.words((G2[0], (G2[1] + 1) % gm.Q))  # not on the curve
    out += [off, gm.jac_words((G2[0], (G2[1] + 1) % gm.Q), 3)]
    return [(w, gm.check_words(w)) for w in out]


_JAC = []


@pytest.mark.parametrize("count", COUNTS)
def test_check_of_jacobian_records_matches_the_model(ctx, count):
    if not _JAC:
        _JAC.extend(_jac_cases())
    assert {s for _, s in _JAC} == {0, 1, 2, 3}
    by = {s: [w for w, t in _JAC if t == s] for s in range(4)}
    rng = random.Random(count)
    for status in range(4):
        order = list(range(len(_JAC)))
        rng.shuffle(order)
        rows = [_JAC[order[i % len(order)]] for i in range(count)]
        rows[0] = (rng.choice(by[status]), status)
        if count > 1:
            rows[-1] = (rng.choice(by[(status + 1) % 4]), (status + 1) % 4)
        got = ctx.g1_check(np.stack([w for w, _ in rows]))
        assert got.tolist() == [s for _, s in rows], (count, status)


def test_decompressed_points_pass_the_check_and_the_counts_of_zero(ctx):
    encs = [e for _, e in gm.cases(1)]
    pts, st = ctx.g1_decompress_check(b"".join(encs))
    keep = np.isin(st, (0, 3))
    assert ctx.g1_check(pts[keep]).tolist() == st[keep].tolist()
    # count = 0 is ZK_OK with or without pointers; null pointers with count > 0 are ZK_ERR_INVALID
    from zkhip._lib import ZK_ERR_INVALID

    p0, s0 = ctx.g1_decompress_check(b"")
    assert p0.shape == (0, 18) and s0.shape == (0,) and ctx.g1_check(np.zeros((0, 18), dtype=np.uint64)).shape == (0,)
    assert ctx.lib.zk_g1_decompress_check(ctx.h, 0, None, None, None) == 0 and ctx.lib.zk_g1_check(ctx.h, 0, None, None) == 0
    buf = (ctypes.c_uint8 * 144)()
    assert ctx.lib.zk_g1_decompress_check(ctx.h, 1, None, buf, buf) == ZK_ERR_INVALID
    assert ctx.lib.zk_g1_decompress_check(ctx.h, 1, buf, None, buf) == ZK_ERR_INVALID
    assert ctx.lib.zk_g1_check(ctx.h, 1, buf, None) == ZK_ERR_INVALID and ctx.lib.zk_g1_check(ctx.h, 1, None, buf) == ZK_ERR_INVALID
    with pytest.raises(ValueError):
        ctx.g1_decompress_check(b"\0" * 47)
