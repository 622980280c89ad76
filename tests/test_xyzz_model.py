"""
tests/xyzz_model.py checked on its own (no GPU): its group law against the oracle's on curve points, and its generated inputs against
what they claim -- the engineered intermediates really have their residues, the ordinary pairs really have different x, every operand
is inside the invariants of csrc/curve30.cuh, and tests/test_gpu_xyzz.py runs the whole generated list.
"""
import pytest

import pyoracle as po
import xyzz_model as xm
from xyzz_model import G1, G2, Q

BINARY = [m for m in xm.MODES if m not in xm.UNARY]


def _g1(P):
    return None if P is None else (P[0][0], P[1][0])


def test_law_equals_oracle_on_curve_points():
    p1, p2 = xm.curve_points("g1", 24), xm.curve_points("g2", 24)
    assert all(po.g1_is_on_curve(_g1(P)) for P in p1) and all(po.g2_is_on_curve(P) for P in p2)
    for i in range(23):
        for A, B in ((p1[i], p1[i + 1]), (p1[i], p1[i]), (p1[i], xm.law_neg(G1, p1[i])), (None, p1[i]), (p1[i], None), (None, None)):
            assert _g1(xm.law_add(G1, A, B)) == po.g1_add(_g1(A), _g1(B))
        assert _g1(xm.law_neg(G1, p1[i])) == po.g1_neg(_g1(p1[i]))
        for A, B in ((p2[i], p2[i + 1]), (p2[i], p2[i]), (p2[i], xm.law_neg(G2, p2[i])), (None, p2[i]), (p2[i], None), (None, None)):
            assert xm.law_add(G2, A, B) == po.g2_add(A, B)
        assert xm.law_neg(G2, p2[i]) == po.g2_neg(p2[i])


@pytest.mark.parametrize("name", ["g1", "g2"])
def test_scaling_and_decoding_round_trip(name):
    cv = xm.CURVES[name]
    rng = po.SplitMix64(5)
    for P in xm.curve_points(name, 24)[:6]:
        op = xm.scale(cv, P, cv.rand_nonzero(rng))
        assert xm.point(cv, op) == P and xm.consistent(cv, op)
        assert xm.affine_point(cv, xm.scale(cv, P, cv.one)) == P
    assert xm.point(cv, xm.inf_op(cv)) is None and xm.affine_point(cv, xm.inf_op(cv)) is None


@pytest.mark.parametrize("name", ["g1", "g2"])
def test_engineered_cases_have_the_residue_they_claim(name):
    cv = xm.CURVES[name]
    eng = xm.engineered(cv)
    seen = set()
    for tag, a, b, (what, residue) in eng:
        got = {"U2": xm.madd_u2, "S2": xm.madd_s2, "Q": xm.madd_q}[what](cv, a, b)
        assert got == residue, tag
        assert b[2] == cv.elem(xm.R390, 0) and b[3] == b[2], "b has z = 1: the full addition sees the same intermediates"
        seen.add(what)
    assert seen == {"U2", "S2", "Q"}
    # what the issue names: S2 small with a zero top limb and S2 = q - 1 against Y1 = q - 1 and q - 2^30 (+ 3q under the max lifts)
    s2 = [(a[1][0], r[0]) for _, a, _, (w, r) in eng if w == "S2"]
    for y in (Q - 1, Q - (1 << 30)):
        assert any(y1 == y and r < (1 << 360) for y1, r in s2) and any(y1 == y and r == Q - 1 for y1, r in s2)
    qs = [r[0] for _, _, _, (w, r) in eng if w == "Q"]
    assert Q - 1 in qs and any(r < (1 << 360) for r in qs)
    # every engineered pair is in the lists the GPU test runs, under the maximal lifts too
    tags = {c.tag for c in xm.cases(name, "madd")}
    assert all(f"{tag}/max" in tags for tag, *_ in eng)


@pytest.mark.parametrize("name", ["g1", "g2"])
@pytest.mark.parametrize("mode", xm.MODES)
def test_generated_operands(name, mode):
    cv = xm.CURVES[name]
    cs = xm.cases(name, mode)
    assert len(cs) >= 100
    kinds = {c.kind for c in cs}
    assert "same" in kinds and ("inf" in kinds or mode == "dbl_affine")
    for v in xm.VARIANTS:
        assert any(c.tag.endswith("/" + v) for c in cs)
    for c in cs:
        for op, lf in ((c.a, c.la), (c.b, c.lb)):
            if op is None:
                assert mode in xm.UNARY
                continue
            vals = xm.values(cv, op, lf)
            assert all(0 <= r < Q for co in op for r in co)
            assert all(0 <= v < xm.BOUND[k // cv.deg] * Q for k, v in enumerate(vals)), c.tag
            if xm.is_inf(cv, op):
                assert not any(vals), "infinity is sent as all-zero coordinates with lift 0"
            elif mode != "dbl_affine":
                assert xm.consistent(cv, op), c.tag
        if mode in ("madd", "madd_neg"):
            assert c.lb == xm.ZERO_LIFT[cv.deg], "the affine operand is canonical"
        if mode in xm.UNARY:
            assert xm.is_inf(cv, c.a) or c.a[1] != cv.zero
        elif c.kind == "ord":  # an ordinary pair takes the chord: different x, both finite
            A = xm.point(cv, c.a)
            B = xm.affine_point(cv, c.b) if mode in ("madd", "madd_neg") else xm.point(cv, c.b)
            assert A is not None and B is not None and A[0] != B[0], c.tag
        elif c.kind == "same":
            A = xm.point(cv, c.a)
            B = xm.affine_point(cv, c.b) if mode in ("madd", "madd_neg") else xm.point(cv, c.b)
            assert A[0] == B[0], c.tag
        else:
            assert xm.is_inf(cv, c.a) or xm.is_inf(cv, c.b)
        assert 1 <= c.rep <= 3


@pytest.mark.parametrize("name", ["g1", "g2"])
def test_lifts_reach_both_ends_of_every_band(name):
    cv = xm.CURVES[name]
    cs = xm.cases(name, "add")
    for k in range(4):
        ks = {l for c in cs for lf in (c.la, c.lb) for l in lf[k]}
        assert ks == set(range(xm.LIFT_MAX[k] + 1))


@pytest.mark.parametrize("name", ["g1", "g2"])
@pytest.mark.parametrize("mode", ["add_quad", "acc_quad"])
def test_quad_lists_interleave_the_branches(name, mode):
    cs = xm.cases(name, mode)
    assert len(cs) > 128 and len(cs) % 64 != 0, "the chunk layout is exercised past two blocks, with a partial one"
    body = cs[: len(cs) - len(cs) % 3]
    assert all(c.kind == ("ord", "inf", "same")[i % 3] for i, c in enumerate(body))
    assert {c.rep for c in cs} == {1, 2, 3}
    assert any(a.rep != b.rep for a, b in zip(cs, cs[1:]))
    # nothing of the list of the plain addition is lost by the reordering
    assert {c.tag for c in cs} == {c.tag for c in xm.cases(name, "add")}


def test_gpu_test_runs_the_whole_list():
    """no skip, filter or retry between the generated list and the device: the GPU test takes cases() as it is"""
    import test_gpu_xyzz as t

    cv = xm.CURVES["g1"]
    cs = xm.cases("g1", "madd")
    a, la, b, lb, rep = t.pack_cases(cv, cs)
    assert len(a) == len(la) == len(b) == len(lb) == len(rep) == len(cs)


def test_check_result_rejects_what_it_should():
    cv = G1
    P = xm.curve_points("g1", 2)[0]
    op = xm.scale(cv, P, (12345,))

    def limbs(vals):
        return [[(v >> (30 * i)) & ((1 << 30) - 1) if i < 12 else v >> 360 for i in range(13)] for v in vals]

    good = [op[0][0] + 7 * Q, op[1][0] + 3 * Q, op[2][0] + Q, op[3][0] + Q]
    assert xm.check_result(cv, limbs(good), P) is None
    assert xm.split(cv, limbs(good)) == (op, ((7,), (3,), (1,), (1,)))
    for k in range(4):
        bad = list(good)
        bad[k] += Q  # right modulo q, one q above its bound
        assert "bound" in xm.check_result(cv, limbs(bad), P)
    wrapped = limbs(good)
    wrapped[0][3] += 1 << 30
    wrapped[0][4] -= 1
    assert "2^30" in xm.check_result(cv, wrapped, P)
    assert xm.check_result(cv, limbs(good), xm.law_add(cv, P, P)) == "decodes to another point"
    assert xm.check_result(cv, limbs([good[0], good[1], good[2], good[3] + 1]), P) == "ZZ^3 != ZZZ^2"
    assert xm.check_result(cv, limbs([0, 0, 0, 0]), None) is None
    assert xm.check_result(cv, limbs([0, 0, Q, 0]), None) is not None and xm.check_result(cv, limbs(good), None) is not None
    assert xm.check_result(cv, limbs([good[0], good[1], Q, Q]), P) == "ZZ = 0 (mod q) on a finite result"
