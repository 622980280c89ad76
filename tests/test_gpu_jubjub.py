"""
Jubjub and Schnorr verification on the device (zk_jubjub_mul / _check, zk_schnorr_verify) bit for bit against the independent model
(jubjub_model.py) at counts around a wave and a workgroup (1, 63, 64, 65, 257): the multiplication with given points and with the fixed
base over the edge points and edge scalars of the CPU tests, the refusal of off-curve points with count and smallest index and an untouched
output, the membership statuses, and signatures with every corruption spread over the batch.
"""
import random

import numpy as np
import pytest

import jubjub_model as jm

pytestmark = pytest.mark.gpu
COUNTS = [1, 63, 64, 65, 257]


@pytest.fixture(scope="module")
def jub(ctx):
    from zkhip import jubjub as jj
    from zkhip import poseidon as ps

    p = ps.Poseidon(ctx)
    yield jj.Jubjub(ctx, p)
    p.free()


def cycled(n):
    """n (point, scalar) pairs: the 11 case points and the 9 edge scalars, cycled (99 distinct pairs)"""
    pts, ks = jm.case_points(), jm.SCALARS
    return [pts[i % len(pts)] for i in range(n)], [ks[i % len(ks)] for i in range(n)]


@pytest.mark.parametrize("n", COUNTS)
def test_mul_points(ctx, jub, n):
    from zkhip import jubjub as jj

    pts, ks = cycled(n)
    out = jub.mul(ctx.to_device(jj.points_limbs(pts)), ctx.to_device(jj.scalars_limbs(ks)), n)
    want = jj.points_limbs([jm.cached_mul(k, P) for P, k in zip(pts, ks)])
    assert (out.download((n, 2, 4)) == want).all()


@pytest.mark.parametrize("n", COUNTS)
def test_mul_fixed_base(ctx, jub, n):
    from zkhip import jubjub as jj

    rng = random.Random(n)
    ks = (jm.SCALARS + [rng.randrange(1 << 256) for _ in range(8)]) * (n // 17 + 1)
    ks = ks[:n]
    out = jub.mul(None, ctx.to_device(jj.scalars_limbs(ks)), n)
    want = jj.points_limbs([jm.cached_mul(k, jm.G) for k in ks])
    assert (out.download((n, 2, 4)) == want).all()


@pytest.mark.parametrize("n", [1, 65, 257])
def test_mul_refuses_off_curve(ctx, jub, n):
    from zkhip import jubjub as jj

    pts, ks = cycled(n)
    rng = random.Random(5)
    bad = sorted({0, n - 1} if n > 1 else {0})
    for where, count, first in ((bad, len(bad), 0), ([n - 1], 1, n - 1)):
        cur = list(pts)
        for i in where:
            cur[i] = jm.off_curve_point(rng)
        guard = np.full((n, 2, 4), 0x5A5A5A5A5A5A5A5A, dtype=np.uint64)
        out = ctx.to_device(guard)
        with pytest.raises(ValueError, match=rf"{count} of {n} points are not on the curve; the first is {first}$"):
            jub.mul(ctx.to_device(jj.points_limbs(cur)), ctx.to_device(jj.scalars_limbs(ks)), n, out=out)
        assert (out.download((n, 2, 4)) == guard).all()


def test_mul_refuses_non_canonical_coordinate(ctx, jub):
    """a coordinate that is not below r is no point: x = r (Montgomery limbs of the integer r itself) beside the identity's y"""
    from zkhip import jubjub as jj

    pts = jj.points_limbs([jm.G, jm.O, jm.G])
    pts[1, 0] = jj.scalars_limbs([jm.R])[0]
    with pytest.raises(ValueError, match=r"1 of 3 points are not on the curve; the first is 1$"):
        jub.mul(ctx.to_device(pts), ctx.to_device(jj.scalars_limbs([1, 1, 1])), 3)


@pytest.mark.parametrize("n", COUNTS)
def test_check(ctx, jub, n):
    from zkhip import jubjub as jj

    pts, _ = cycled(n)
    rng = random.Random(n + 1)
    pts = [jm.off_curve_point(rng) if i % 13 == 12 or i == n - 1 and n > 1 else P for i, P in enumerate(pts)]
    status = {P: (2 if not jm.on_curve(P) else 0 if jm.in_subgroup(P) else 3) for P in set(pts)}
    got = jub.check(ctx.to_device(jj.points_limbs(pts)), n)
    assert got.tolist() == [status[P] for P in pts]
    if n >= 63:
        assert {0, 2, 3} <= set(got.tolist())


def batch(n, kinds):
    """n signatures: valid ones cycled over the four signed cases; kinds = {lane: corruption}"""
    cases = jm.signed_cases()
    rows, want = [], []
    for i in range(n):
        _, PK, m, sig = cases[i % len(cases)]
        if i in kinds:
            (PK, m, sig), st = jm.corrupt(kinds[i], PK, m, sig)
            assert jm.cached_verify(PK, m, sig) == st
        else:
            st = jm.cached_verify(PK, m, sig)
            assert st == 0
        rows.append((PK, m, sig))
        want.append(st)
    return rows, want


def run(ctx, jub, rows):
    from zkhip import jubjub as jj
    from zkhip.field import fr_mont

    n = len(rows)
    pk = ctx.to_device(jj.points_limbs([r[0] for r in rows]))
    msg = ctx.to_device(np.stack([fr_mont(r[1]) for r in rows]))
    sig = ctx.to_device(jj.signatures_limbs([r[2] for r in rows]))
    return jub.schnorr_verify(pk, msg, sig, n).tolist()


@pytest.mark.parametrize("n", COUNTS)
def test_schnorr_mixed(ctx, jub, n):
    """every corruption somewhere: the first and the last lane, both sides of lane 63 / 64, the rest spread by a fixed stride"""
    lanes = [i for i in (0, n - 1, 62, 63, 64, 65, 7, 20, 33, 46, 100, 200, 255, 256) if i < n]
    kinds = {lane: jm.CORRUPTIONS[j % len(jm.CORRUPTIONS)] for j, lane in enumerate(dict.fromkeys(lanes))}
    rows, want = batch(n, kinds)
    assert run(ctx, jub, rows) == want
    if n >= 63:
        assert set(want) == {0, 1, 2, 3, 4}


def test_schnorr_all_valid(ctx, jub):
    rows, want = batch(130, {})
    assert want == [0] * 130 and run(ctx, jub, rows) == want


def test_schnorr_all_invalid(ctx, jub):
    rows, want = batch(130, {i: jm.CORRUPTIONS[i % len(jm.CORRUPTIONS)] for i in range(130)})
    assert 0 not in want and run(ctx, jub, rows) == want
