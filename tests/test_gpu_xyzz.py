"""
The XYZZ group formulas of the MSM (csrc/curve30.cuh, csrc/curve30_g2.cuh) one operation at a time, at chosen representatives, through
the test hooks zk_dbg_xyzz_op / zk_dbg_xyzz2_op -- against the affine chord / tangent map of tests/xyzz_model.py on exact integers.

Every raw device result is checked for: the point it decodes to (infinity = all-zero limbs), ZZ^3 == ZZZ^2 with ZZ != 0, the static
bounds X < 8q, Y < 4q, ZZ < 2q, ZZZ < 2q as exact integers, and limbs 0..11 below 2^30.  The chain tests feed the raw results back in as
residue + lift, so the invariants are shown to be closed under iteration from the worst start.  Every generated case runs.
"""
import numpy as np
import pytest

import pyoracle as po
import xyzz_model as xm
from zkhip._lib import test_hooks as zk_test_hooks

pytestmark = pytest.mark.gpu

CURVE_NAMES = ("g1", "g2")
STEPS, LANES = 64, 256


def pack_cases(cv, cs):
    """the case list as the five host arrays of one hook call (unary modes: b repeats a and is not read)"""
    a, la = xm.pack_ops(cv, [c.a for c in cs]), xm.pack_lifts(cv, [c.la for c in cs])
    b = xm.pack_ops(cv, [c.a if c.b is None else c.b for c in cs])
    lb = xm.pack_lifts(cv, [c.la if c.b is None else c.lb for c in cs])
    return a, la, b, lb, np.array([c.rep for c in cs], dtype=np.uint32)


def run(ctx, cv, mode, a, la, b, lb, rep):
    """one hook call on host arrays -> raw limbs [n, 4 * deg, 13]"""
    n = len(a)
    return ctx.dbg_xyzz(cv.deg == 2, mode, ctx.to_device(a), ctx.to_device(la), ctx.to_device(b), ctx.to_device(lb), ctx.to_device(rep), n)


def run_cases(ctx, cv, mode, cs):
    return run(ctx, cv, mode, *pack_cases(cv, cs))


@pytest.mark.parametrize("mode", xm.MODES)
@pytest.mark.parametrize("name", CURVE_NAMES)
def test_every_mode_on_every_input_class(ctx, name, mode):
    cv = xm.CURVES[name]
    cs = xm.cases(name, mode)
    if mode in ("add_quad", "acc_quad"):
        assert len(cs) > 128 and len(cs) % 64, "the chunk layout: more than two blocks of 64 points, the last one partial"
    got = run_cases(ctx, cv, mode, cs)
    bad = []
    for i, c in enumerate(cs):
        err = xm.check_result(cv, got[i], xm.expected(cv, mode, c))
        if err:
            bad.append(f"[{i}] {c.tag} (rep {c.rep}): {err}")
    assert not bad, f"{name} {mode}: {len(bad)} of {len(cs)} wrong:\n" + "\n".join(bad[:20])


@pytest.mark.parametrize("name", CURVE_NAMES)
def test_quad_forms_agree_with_the_single_lane_addition(ctx, name):
    """the same operands through add, add_quad and acc_quad (one trip) decode to the same point"""
    cv = xm.CURVES[name]
    cs = [c._replace(rep=1) for c in xm.cases(name, "add_quad")]
    one, quad, acc = (run_cases(ctx, cv, m, cs) for m in ("add", "add_quad", "acc_quad"))
    for i, c in enumerate(cs):
        ops = [xm.split(cv, r[i])[0] for r in (one, quad, acc)]
        pts = [xm.point(cv, op) for op in ops]
        assert pts[0] == pts[1] == pts[2] == xm.expected(cv, "add", c), (i, c.tag)


# ---- chains: the raw output goes back in as residue + lift ------------------------------------------------------------------------
def _chain_start(cv, rng):
    """LANES accumulators at the worst start: maximal lifts on edge residues, curve points, and a few lanes at infinity"""
    E = xm._extreme_elems(cv)
    pts = xm.curve_points(cv.name, 24)
    ops = []
    for l in range(LANES):
        if l % 32 == 31:
            ops.append(xm.inf_op(cv))
        elif l % 2:
            ops.append(xm.scale(cv, pts[l % 24], cv.rand_nonzero(rng)))
        else:
            ops.append(xm.raw(cv, E[l % len(E)], E[(l // 2 + 2) % len(E)], cv.rand_nonzero(rng)))
    return ops, [xm.lifts(cv, op, "max", rng) for op in ops]


def _chain_operand(cv, rng, step, lane, cur, affine):
    """the step's second operand: mostly fresh pairs (on and off the curve); now and then the accumulator's own point, so that the
    chain also runs through the doubling and cancellation branches and restarts from infinity"""
    z = cv.one if affine else cv.rand_nonzero(rng)
    if cur is not None and cur[1] != cv.zero and (step + lane) % 37 == 5:
        return xm.scale(cv, cur if lane % 2 else xm.law_neg(cv, cur), z)
    if (step + lane) % 41 == 7:
        return xm.inf_op(cv)
    if lane % 3 == 0:
        return xm.scale(cv, xm.curve_points(cv.name, 24)[(step * 7 + lane) % 24], z)
    return xm.raw(cv, cv.rand(rng), cv.rand_nonzero(rng), z)


@pytest.mark.parametrize("kind", ["madd", "add", "acc_quad"])
@pytest.mark.parametrize("name", CURVE_NAMES)
def test_invariants_are_closed_under_iteration(ctx, name, kind):
    """64 steps on 256 independent lanes: madd with alternating sign, add folding XYZZ operands under maximal lifts, acc_quad adding every
    operand three times.  After every step each lane is the running affine sum, inside its bounds, and goes back in exactly as it came out."""
    cv = xm.CURVES[name]
    rng = po.SplitMix64(0xC4A1 + cv.deg + len(kind))
    ops, lfs = _chain_start(cv, rng)
    cur = [xm.point(cv, op) for op in ops]
    affine = kind == "madd"
    rep = np.full(LANES, 3 if kind == "acc_quad" else 1, dtype=np.uint32)
    branches = set()
    for step in range(STEPS):
        mode = ("madd", "madd_neg")[step % 2] if affine else kind
        bs = [_chain_operand(cv, rng, step, l, cur[l], affine) for l in range(LANES)]
        lbs = [xm.ZERO_LIFT[cv.deg] if affine else xm.lifts(cv, b, "max", rng) for b in bs]
        got = run(ctx, cv, mode, xm.pack_ops(cv, ops), xm.pack_lifts(cv, lfs), xm.pack_ops(cv, bs), xm.pack_lifts(cv, lbs), rep)
        for l in range(LANES):
            B = xm.affine_point(cv, bs[l]) if affine else xm.point(cv, bs[l])
            if mode == "madd_neg":
                B = xm.law_neg(cv, B)
            for _ in range(int(rep[l])):
                if cur[l] is not None and B is not None and cur[l][0] == B[0]:
                    branches.add("double" if cur[l] == B else "cancel")
                branches.add("from_inf" if cur[l] is None else "b_inf" if B is None else "finite")
                cur[l] = xm.law_add(cv, cur[l], B)
            err = xm.check_result(cv, got[l], cur[l])
            assert err is None, f"{name} {kind} step {step} ({mode}) lane {l}: {err}"
            ops[l], lfs[l] = xm.split(cv, got[l])
    assert branches == {"double", "cancel", "from_inf", "b_inf", "finite"}


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CURVE_NAMES)
def test_refusals(ctx, name):
    cv = xm.CURVES[name]
    fn = zk_test_hooks().zk_dbg_xyzz2_op if cv.deg == 2 else zk_test_hooks().zk_dbg_xyzz_op
    cs = xm.cases(name, "add")[:5]
    n = len(cs)
    a, la, b, lb, rep = (ctx.to_device(x) for x in pack_cases(cv, cs))
    mark = np.full((n, 64 * cv.deg), 0xA5A5A5A5, dtype=np.uint32)
    out = ctx.to_device(mark)

    def untouched():
        return (out.download(mark.shape, np.uint32) == mark).all()

    for mode in (-1, len(xm.MODES), 1 << 20):
        assert fn(ctx.h, mode, a.ptr, la.ptr, b.ptr, lb.ptr, rep.ptr, out.ptr, n) == -1 and untouched(), mode
    for mode in range(len(xm.MODES)):
        binary = xm.MODES[mode] not in xm.UNARY
        nulls = [0, 1, 5] + ([2, 3] if binary else []) + ([4] if xm.MODES[mode] == "acc_quad" else [])
        for k in nulls:
            args = [a.ptr, la.ptr, b.ptr, lb.ptr, rep.ptr, out.ptr]
            args[k] = None
            assert fn(ctx.h, mode, *args, n) == -1 and untouched(), (mode, k)
        assert fn(ctx.h, mode, a.ptr, la.ptr, b.ptr, lb.ptr, rep.ptr, out.ptr, 0) == 0 and untouched(), mode
    assert fn(None, 2, a.ptr, la.ptr, b.ptr, lb.ptr, rep.ptr, out.ptr, n) == -1 and untouched()
    # and after the refusals the hook still works
    assert fn(ctx.h, 2, a.ptr, la.ptr, b.ptr, lb.ptr, rep.ptr, out.ptr, n) == 0 and not untouched()
    got = out.download((n, 4 * cv.deg, 16), np.uint32)[:, :, :13]
    for i, c in enumerate(cs):
        assert xm.check_result(cv, got[i], xm.expected(cv, "add", c)) is None
