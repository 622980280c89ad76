"""
zk_g2_decompress_check and zk_g2_check (csrc/zk_g2check.hip) against the integer model (g2check_model.py), bit for bit, points and
status: the model decides membership by the definition [r]P = O, the kernels by psi(P) == [x]P.  Every batch mixes the four statuses so
the lanes of one wave diverge; the counts sit on both sides of the block edge; members, random twist points, cofactor parts T, T + kG,
points of order 13 and 23 (whose ladders meet equal operands, opposite operands and infinity), infinity and every malformed encoding
are in every batch that has room.
"""
import ctypes
import random

import numpy as np
import pytest

import g2check_model as gm

pytestmark = pytest.mark.gpu

COUNTS = [1, 63, 64, 65, 100]


def _arrange(items, count, first, last, seed):
    """count items: every one present when it fits, `first` at lane 0 and `last` at the last lane"""
    rng = random.Random(seed)
    every = list(items)
    rng.shuffle(every)
    body = [every[i % len(every)] for i in range(count)]
    rng.shuffle(body)
    body[0] = first
    if count > 1:
        body[-1] = last
    return body


@pytest.mark.parametrize("count", COUNTS)
def test_decompress_check_matches_the_model(ctx, count):
    pool = gm.by_status(1)
    every = [e for _, e in gm.cases(1)]
    for status in range(4):
        rng = random.Random(100 * count + status)
        encs = _arrange(every, count, rng.choice(pool[status]), rng.choice(pool[(status + 1) % 4]), 7 * count + status)
        want_pts, want_st = gm.expected(encs)
        if count >= 63:
            assert set(want_st.tolist()) == {0, 1, 2, 3}
        pts, st = ctx.g2_decompress_check(b"".join(encs))
        assert st.tolist() == want_st.tolist(), (count, status)
        assert (pts == want_pts).all(), (count, status)
    assert ctx.g2_decompress_check(np.frombuffer(b"".join(encs), dtype=np.uint8).reshape(count, 96))[1].tolist() == want_st.tolist()


def test_named_points_in_one_call_and_the_degenerate_ones_alone(ctx):
    cases = gm.cases(1)
    encs = [e for _, e in cases]
    want_pts, want_st = gm.expected(encs)
    pts, st = ctx.g2_decompress_check(b"".join(encs))
    bad = [(n, int(a), int(b)) for (n, _), a, b in zip(cases, st, want_st) if a != b]
    assert not bad, bad
    assert (pts == want_pts).all()
    for (name, e), w, s in zip(cases, want_pts, want_st):
        if name.startswith(("order", "infinity", "inf+")):
            p1, s1 = ctx.g2_decompress_check(e)
            assert int(s1[0]) == int(s) and (p1[0] == w).all(), name


def _records():
    """(24 words, the model's status): every point of the model, a coordinate equal to q or all ones in each position, records off the twist"""
    out = [gm.words(P) for _, P in gm.points(1)]
    P2 = gm.mul(gm.G2, 2)
    qw = np.array([(gm.Q >> (64 * i)) & (2**64 - 1) for i in range(6)], dtype=np.uint64)
    for k in range(4):  # a coordinate equal to q: not canonical
        w = gm.words(P2)
        w[6 * k:6 * k + 6] = qw
        out.append(w)
    w = gm.words(P2)
    w[18:] = 2**64 - 1
    out.append(w)
    out.append(gm.words((P2[0], ((P2[1][0] + 1) % gm.Q, P2[1][1]))))  # off the twist
    out.append(gm.words(((P2[0][0], (P2[0][1] + 1) % gm.Q), P2[1])))
    out.append(gm.words(((0, 0), (1, 0))))  # x = 0 but not the zero record
    return [(w, gm.check_words(w)) for w in out]


_REC = []


@pytest.mark.parametrize("stride", [192, 200])
@pytest.mark.parametrize("count", COUNTS)
def test_check_of_affine_records_matches_the_model(ctx, count, stride):
    if not _REC:
        _REC.extend(_records())
    assert {s for _, s in _REC} == {0, 1, 2, 3}
    by = {s: [r for r in _REC if r[1] == s] for s in range(4)}
    for status in range(4):
        rng = random.Random(count + 10 * status)
        rows = _arrange(_REC, count, rng.choice(by[status]), rng.choice(by[(status + 1) % 4]), 3 * count + status)
        want = [s for _, s in rows]
        raw = np.zeros((count, stride), dtype=np.uint8)
        raw[:, :192] = np.stack([w for w, _ in rows]).view(np.uint8).reshape(count, 192)
        if stride == 192:
            assert ctx.g2_check(np.stack([w for w, _ in rows])).tolist() == want, (count, status)
        else:
            raw[:, 193:] = 0xFF  # padding after the flag byte is not read
            if count > 2:  # the Rust struct's flag byte marks infinity whatever the coordinates hold
                raw[1, 192], want[1] = 1, 0
        assert ctx.g2_check(raw, g2_stride=stride).tolist() == want, (count, status, stride)


def test_decompressed_points_pass_the_check_and_the_counts_of_zero(ctx):
    encs = [e for _, e in gm.cases(1)]
    pts, st = ctx.g2_decompress_check(b"".join(encs))
    keep = np.isin(st, (0, 3))
    assert ctx.g2_check(pts[keep]).tolist() == st[keep].tolist()
    from zkhip._lib import ZK_ERR_INVALID

    p0, s0 = ctx.g2_decompress_check(b"")
    assert p0.shape == (0, 24) and s0.shape == (0,) and ctx.g2_check(np.zeros((0, 24), dtype=np.uint64)).shape == (0,)
    assert ctx.lib.zk_g2_decompress_check(ctx.h, 0, None, None, None) == 0 and ctx.lib.zk_g2_check(ctx.h, 0, None, 192, None) == 0
    buf = (ctypes.c_uint8 * 192)()
    assert ctx.lib.zk_g2_decompress_check(ctx.h, 1, None, buf, buf) == ZK_ERR_INVALID
    assert ctx.lib.zk_g2_decompress_check(ctx.h, 1, buf, None, buf) == ZK_ERR_INVALID
    assert ctx.lib.zk_g2_check(ctx.h, 1, buf, 192, None) == ZK_ERR_INVALID and ctx.lib.zk_g2_check(ctx.h, 1, None, 192, buf) == ZK_ERR_INVALID
    assert ctx.lib.zk_g2_check(ctx.h, 1, buf, 191, buf) == ZK_ERR_INVALID
    with pytest.raises(ValueError):
        ctx.g2_decompress_check(b"\0" * 95)
