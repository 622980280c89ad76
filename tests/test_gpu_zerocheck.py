"""
Gate ZeroCheck on the GPU: zk_eq_table and zk_sumcheck_gate bit-exact against the big-int model (zerocheck_model.py), the large
sizes closed at both ends by existing device code, and the prover / verifier end to end through the device pairing.
"""
import os

import numpy as np
import pytest

import pyoracle as po
import zerocheck_model as zm
from helpers import jac_norm_to_affine, pt_ints, rand_fr

R = po.R_MOD
pytestmark = pytest.mark.gpu


def _up(ctx, tabs):
    return {k: ctx.to_device(zm.mont(v)) for k, v in tabs.items()}


def _run(ctx, dev, n, chal_m):
    return ctx.sumcheck_gate(dev["eq"], dev["q1"], dev["q2"], dev["a"], dev["b"], dev["c"], dev["in"], 1 << n, chal_m)


def _check_against_model(ctx, tabs, chal, label=""):
    n = len(chal)
    dev = _up(ctx, tabs)
    want_rounds, want_last = zm.sumcheck_gate(tabs, chal)
    got_rounds, got_last = _run(ctx, dev, n, zm.mont(chal))
    assert got_rounds.shape == (n, 5, 4) and got_last.shape == (7, 4)
    for i in range(n):
        assert zm.ints(got_rounds[i]) == want_rounds[i], (label, n, i)
    assert zm.ints(got_last) == want_last, (label, n)
    for k in zm.TABLES:  # inputs unchanged
        assert (dev[k].download((1 << n, 4)) == zm.mont(tabs[k])).all(), (label, k)


def _tabs(n, seed, satisfied):
    rng = po.SplitMix64(seed)
    tau, chal = rng.fr_vec(n), rng.fr_vec(n)
    tabs = zm.circuit(n, seed + 1, satisfied=satisfied)
    tabs["eq"] = zm.eq_table(tau)
    return tabs, tau, chal


@pytest.mark.parametrize("n", range(0, 13))
def test_eq_table_matches_model(ctx, n):
    tau = po.SplitMix64(40 + n).fr_vec(n)
    got = ctx.eq_table(zm.mont(tau).reshape(n, 4)).download((1 << n, 4))
    assert zm.ints(got) == zm.eq_table(tau)


def test_eq_table_n20_properties(ctx):
    n = 20
    tau, r = rand_fr(n, 71), rand_fr(n, 72)
    eq = ctx.eq_table(tau)
    pairs, _ = ctx.sumcheck(eq, 1 << n, r)
    assert (po.fr_from_mont_limbs(pairs[0][0]) + po.fr_from_mont_limbs(pairs[0][1])) % R == 1
    from zkhip.zerocheck import eq_eval

    assert zm.ints(ctx.fold(eq, 1 << n, r).download((1, 4)))[0] == eq_eval(zm.ints(tau), zm.ints(r))


@pytest.mark.parametrize("n", range(1, 15))
def test_sumcheck_gate_matches_model(ctx, n):
    for satisfied in (False, True):
        tabs, _, chal = _tabs(n, 1000 + 2 * n + satisfied, satisfied)
        _check_against_model(ctx, tabs, chal, "satisfied" if satisfied else "random")


@pytest.mark.parametrize("n", [1, 4, 10, 11])
def test_sumcheck_gate_edge_values(ctx, n):
    m = 1 << n
    rnd = po.SplitMix64(5 + n).fr_vec(n)
    _check_against_model(ctx, {k: [0] * m for k in zm.TABLES}, rnd, "zero")
    _check_against_model(ctx, {k: [R - 1] * m for k in zm.TABLES}, rnd, "r-1")
    tabs, _, _ = _tabs(n, 60 + n, False)
    _check_against_model(ctx, tabs, [0] * n, "chal 0")
    _check_against_model(ctx, tabs, [1] * n, "chal 1")
    _check_against_model(ctx, tabs, [(i & 1) for i in range(n)], "chal 0/1")
    _check_against_model(ctx, tabs, [R - 1] * n, "chal r-1")


@pytest.mark.parametrize("local_e", [1, 2, 4, 8, 16, 32, 64, 128, 256, 512])
def test_sumcheck_gate_every_handover_point(ctx, local_e):
    """knob gate_local_e: the HBM passes run down to tables of local_e elements (1: to the very end), the LDS stage takes the rest"""
    try:
        ctx.dbg_tune("gate_local_e", local_e)
        for n in (1, 3, 7, 10, 12):
            tabs, _, chal = _tabs(n, 3000 + 16 * n + local_e, n % 2 == 0)
            _check_against_model(ctx, tabs, chal, f"local_e={local_e}")
        ctx.dbg_tune("gate_pass_wg", 1)
        tabs, _, chal = _tabs(11, 3900 + local_e, False)
        _check_against_model(ctx, tabs, chal, f"local_e={local_e} wg=1")
    finally:
        ctx.dbg_tune("gate_local_e", 512)
        ctx.dbg_tune("gate_pass_wg", 0)


def _big(ctx, n, seed):
    """no big-int model: both ends of the chain from existing device code"""
    from zkhip.zerocheck import gate_value, round_poly_at

    m = 1 << n
    tau, chal = rand_fr(n, seed), rand_fr(n, seed + 1)
    d = {k: ctx.to_device(rand_fr(m, seed + 2 + i)) for i, k in enumerate(("q1", "q2", "a", "b", "c", "in"))}
    d["eq"] = ctx.eq_table(tau)
    rounds, last = _run(ctx, d, n, chal)
    # sum_x G(x) with the element-wise kernels and the plain sumcheck's first pair
    inner = ctx.fr_add(ctx.fr_mul(d["q1"], ctx.fr_add(d["a"], d["b"], m), m), ctx.fr_mul(ctx.fr_mul(d["q2"], d["a"], m), d["b"], m), m)
    inner = ctx.fr_add(ctx.fr_sub(inner, d["c"], m), d["in"], m)
    pairs, _ = ctx.sumcheck(ctx.fr_mul(d["eq"], inner, m), m, chal)
    total = (po.fr_from_mont_limbs(pairs[0][0]) + po.fr_from_mont_limbs(pairs[0][1])) % R
    ch = zm.ints(chal)
    target = total
    for i in range(n):
        p = zm.ints(rounds[i])
        assert (p[0] + p[1]) % R == target, (n, i)
        target = round_poly_at(p, ch[i])
    folded = [zm.ints(ctx.fold(d[k], m, chal).download((1, 4)))[0] for k in zm.TABLES]
    assert zm.ints(last) == folded
    assert target == gate_value(*folded)


def test_sumcheck_gate_n20_chain_closed_by_existing_kernels(ctx):
    _big(ctx, 20, 8100)


@pytest.mark.skipif(os.environ.get("ZK_SLOW_TESTS") != "1", reason="n = 24: 3.5 GiB of tables and as much scratch (ZK_SLOW_TESTS=1)")
def test_sumcheck_gate_n24_chain_closed_by_existing_kernels(ctx):
    _big(ctx, 24, 8200)


def _mont(xs):
    return zm.mont(xs)


@pytest.mark.parametrize("n", [10, 16])
def test_end_to_end_prove_and_verify(ctx, n):
    from zkhip import dist_primitive as dp
    from zkhip import pairing as pr
    from zkhip import zerocheck as zc
    from zkhip.field import fr_mont

    def prove(break_gate=None):
        tabs, tau, chal, s = zc.satisfied_circuit(ctx, n, 7, break_gate)
        cub = dp.PolynomialCommitmentCub.new(ctx, s)
        return zc.gate_zerocheck_prove(ctx, cub.mature(), tabs, tau, chal), tau, chal, s

    proof, tau, chal, s = prove()
    pg2 = pr.powers_of_g2(zm.ints(s))
    vk = dp.pcs_vk(ctx, pg2)
    assert zc.verify_rounds(proof, tau, chal) is True
    assert zc.gate_zerocheck_verify(ctx, vk, proof, tau, chal) is True

    def host_verdict(p):
        """the same decision with the host big-int pairing on the same openings"""
        return zc.verify_rounds(p, tau, chal) and all(dp.verify(pg2, c, v, pf, chal) for c, v, pf in p["openings"])

    def clone(p):
        return {"rounds": p["rounds"].copy(), "openings": [(c.copy(), v.copy(), pf.copy()) for c, v, pf in p["openings"]]}

    muts = {}
    muts["broken gate"] = prove(break_gate=5)[0]
    m = clone(proof)
    m["rounds"][n // 2][3] = fr_mont(zm.ints(m["rounds"][n // 2][3])[0] + 1)
    muts["round value + 1"] = m
    m = clone(proof)
    c, v, pf = m["openings"][2]
    m["openings"][2] = (c, fr_mont(zm.ints(v)[0] + 1), pf)
    muts["opened value + 1"] = m
    m = clone(proof)
    c, v, pf = m["openings"][4]
    other = po.g1_add(pt_ints(jac_norm_to_affine(pf[n // 2])), po.G1_GEN)  # another valid curve point
    pf[n // 2] = np.concatenate([np.array(po.fq_to_mont_limbs(other[0]) + po.fq_to_mont_limbs(other[1]), dtype=np.uint64), pf[n // 2][12:]])
    muts["opening proof point replaced"] = m
    for name, mp in muts.items():
        assert zc.gate_zerocheck_verify(ctx, vk, mp, tau, chal) is False, name
        # the host big-int pairing on the same openings (three mutants stop in the field checks; `all` stops at the first bad opening)
        assert host_verdict(mp) is False, name
    assert host_verdict(proof) is True
    # the proof-point mutation passes the field checks: it is the pairing that rejects it, on both sides
    assert zc.verify_rounds(muts["opening proof point replaced"], tau, chal) is True
    for k, (c, v, pf) in enumerate(muts["opening proof point replaced"]["openings"]):
        assert dp.verify_device(ctx, vk, c, v, pf, chal) == (k != 4), k


def test_sumcheck_gate_errors_leave_outputs_untouched(ctx):
    import zkhip
    from zkhip.api import _h, _ptr

    n = 4
    d = ctx.to_device(rand_fr(1 << n, 1))
    chal = rand_fr(n, 2)
    out = np.full((n, 5, 4), 0xA5, dtype=np.uint64)
    last = np.full((7, 4), 0xA5, dtype=np.uint64)
    p = _ptr(d)

    def call(ptrs, length):
        return ctx.lib.zk_sumcheck_gate(ctx.h, *ptrs, length, _h(chal), _h(out), _h(last))

    for length in (0, 1, 3, 12, 17):
        assert call([p] * 7, length) == -1, length  # ZK_ERR_INVALID
    for k in range(7):
        ptrs = [p] * 7
        ptrs[k] = None
        assert call(ptrs, 1 << n) == -1
    assert ctx.lib.zk_sumcheck_gate(ctx.h, *([p] * 7), 1 << n, None, _h(out), _h(last)) == -1
    assert ctx.lib.zk_eq_table(ctx.h, _h(chal), n, None) == -1
    assert ctx.lib.zk_eq_table(ctx.h, None, n, p) == -1
    assert (out == 0xA5).all() and (last == 0xA5).all()
    with pytest.raises(zkhip.ZkError):
        ctx.sumcheck_gate(d, d, d, d, d, d, d, 12, chal)


def test_second_proof_after_arena_plan_import_allocates_nothing():
    import zkhip

    def work(c):
        n = 15
        tau, chal = rand_fr(n, 11), rand_fr(n, 12)
        t = [c.to_device(rand_fr(1 << n, 20 + i)) for i in range(6)]
        eq = c.eq_table(tau)
        return c.sumcheck_gate(eq, *t, 1 << n, chal)

    a = zkhip.Ctx(0)
    ref = work(a)
    plan = a.arena_plan_export()
    assert plan[2:].any()
    a.close()
    b = zkhip.Ctx(0)
    b.arena_plan_import(plan)
    before = b.arena_plan_export()
    got = work(b)
    assert (b.arena_plan_export() == before).all(), "the gate sumcheck grew an arena although the plan was imported"
    assert (ref[0] == got[0]).all() and (ref[1] == got[1]).all()
    b.close()
