"""
Wiring PermCheck on the GPU: zk_sumcheck_wiring bit-exact against the big-int model (wiring_model.py), the large sizes closed at
both ends by existing device code, and the prover / verifier end to end through the device pairing.
"""
import os

import numpy as np
import pytest

import pyoracle as po
import wiring_model as wm
from helpers import jac_norm_to_affine, pt_ints, rand_fr

R = po.R_MOD
pytestmark = pytest.mark.gpu


def _check_against_model(ctx, tabs, tree, gamma, chal, label=""):
    """tabs: the seven tables as ints (eq, num, den are uploaded; the four views are only the model's), tree: 2N ints"""
    mu = len(chal)
    N = 1 << mu
    d_eq, d_num, d_den, d_tree = (ctx.to_device(wm.mont(x)) for x in (tabs["eq"], tabs["num"], tabs["den"], tree))
    want_rounds, want_last = wm.sumcheck_wiring(tabs, gamma, chal)
    got_rounds, got_last = ctx.sumcheck_wiring(d_eq, d_tree, d_num, d_den, N, wm.mont([gamma])[0], wm.mont(chal))
    assert got_rounds.shape == (mu, 4, 4) and got_last.shape == (7, 4)
    for i in range(mu):
        assert wm.ints(got_rounds[i]) == want_rounds[i], (label, mu, i)
    assert wm.ints(got_last) == want_last, (label, mu)
    # inputs unchanged, the tree included
    assert (d_tree.download((2 * N, 4)) == wm.mont(tree)).all(), label
    for d, k in ((d_eq, "eq"), (d_num, "num"), (d_den, "den")):
        assert (d.download((N, 4)) == wm.mont(tabs[k])).all(), (label, k)


def _valid(mu, seed):
    rng = po.SplitMix64(seed)
    alpha, beta, gamma = rng.fr(), rng.fr(), rng.fr()
    tau, chal = rng.fr_vec(mu), rng.fr_vec(mu)
    tabs, tree = wm.tables(*wm.shuffled_circuit(mu, seed + 1), alpha, beta, tau)
    return tabs, tree, gamma, chal


def _random(mu, seed):
    """unrelated random tables: the tree is any 2N elements, the claimed sum is not 0"""
    rng = po.SplitMix64(seed)
    N = 1 << mu
    gamma, chal = rng.fr(), rng.fr_vec(mu)
    tree = rng.fr_vec(2 * N)
    tabs = wm.views(tree)
    tabs.update(eq=rng.fr_vec(N), num=rng.fr_vec(N), den=rng.fr_vec(N))
    return tabs, tree, gamma, chal


def _const(mu, value):
    N = 1 << mu
    tree = [value] * (2 * N)
    tabs = wm.views(tree)
    tabs.update(eq=[value] * N, num=[value] * N, den=[value] * N)
    return tabs, tree


@pytest.mark.parametrize("mu", range(1, 15))
def test_sumcheck_wiring_matches_model(ctx, mu):
    _check_against_model(ctx, *_valid(mu, 1000 + 2 * mu), "valid")
    _check_against_model(ctx, *_random(mu, 1001 + 2 * mu), "random")


@pytest.mark.parametrize("mu", [1, 4, 10, 11])
def test_sumcheck_wiring_edge_values(ctx, mu):
    rng = po.SplitMix64(5 + mu)
    rnd, g = rng.fr_vec(mu), rng.fr()
    _check_against_model(ctx, *_const(mu, 0), g, rnd, "zero")
    _check_against_model(ctx, *_const(mu, R - 1), g, rnd, "r-1")
    _check_against_model(ctx, *_const(mu, R - 1), R - 1, [R - 1] * mu, "everything r-1")
    tabs, tree, gamma, _ = _random(mu, 60 + mu)
    _check_against_model(ctx, tabs, tree, gamma, [0] * mu, "chal 0")
    _check_against_model(ctx, tabs, tree, gamma, [1] * mu, "chal 1")
    _check_against_model(ctx, tabs, tree, gamma, [(i & 1) for i in range(mu)], "chal 0/1")
    _check_against_model(ctx, tabs, tree, gamma, [R - 1] * mu, "chal r-1")
    _check_against_model(ctx, tabs, tree, 0, rnd, "gamma 0")
    _check_against_model(ctx, tabs, tree, 1, rnd, "gamma 1")


@pytest.mark.parametrize("local_e", [1, 2, 4, 8, 16, 32, 64, 128, 256, 512])
def test_sumcheck_wiring_every_handover_point(ctx, local_e):
    """knob wiring_local_e: the HBM passes run down to tables of local_e elements (1: to the very end), the LDS stage takes the rest;
    knob wiring_pass_wg: one and (the default) two workgroups per CU"""
    try:
        ctx.dbg_tune("wiring_local_e", local_e)
        for wg in (0, 1):
            ctx.dbg_tune("wiring_pass_wg", wg)
            for mu in (1, 3, 7, 10, 12) if wg == 0 else (11,):
                case = _valid(mu, 3000 + 16 * mu + local_e) if mu % 2 == 0 else _random(mu, 3000 + 16 * mu + local_e)
                _check_against_model(ctx, *case, f"local_e={local_e} wg={wg}")
    finally:
        ctx.dbg_tune("wiring_local_e", 512)
        ctx.dbg_tune("wiring_pass_wg", 0)


def _big(ctx, mu, seed):
    """no big-int model: both ends of the chain from existing device code (element-wise kernels, zk_fr_deinterleave, the plain
    sumcheck's first pair, seven zk_fold calls)"""
    from zkhip.wiring import round_poly_at, wiring_value

    N = 1 << mu
    gamma, chal = rand_fr(1, seed)[0], rand_fr(mu, seed + 1)
    d_eq, d_num, d_den = (ctx.to_device(rand_fr(N, seed + 2 + i)) for i in range(3))
    tree_h = rand_fr(2 * N, seed + 5)
    d_tree = ctx.to_device(tree_h)
    rounds, last = ctx.sumcheck_wiring(d_eq, d_tree, d_num, d_den, N, gamma, chal)
    vx0, vx1 = ctx.fr_deinterleave(d_tree, N)
    h, v1x = d_tree.at(0), d_tree.at(32 * N)
    # sum_x F(x): eq [v1x - vx0 vx1 + gamma (den h - num)]
    inner = ctx.fr_scale(ctx.fr_sub(ctx.fr_mul(d_den, h, N), d_num, N), gamma, N)
    inner = ctx.fr_add(ctx.fr_sub(v1x, ctx.fr_mul(vx0, vx1, N), N), inner, N)
    pairs, _ = ctx.sumcheck(ctx.fr_mul(d_eq, inner, N), N, chal)
    total = (po.fr_from_mont_limbs(pairs[0][0]) + po.fr_from_mont_limbs(pairs[0][1])) % R
    ch = wm.ints(chal)
    target = total
    for i in range(mu):
        p = wm.ints(rounds[i])
        assert (p[0] + p[1]) % R == target, (mu, i)
        target = round_poly_at(p, ch[i])
    folded = [wm.ints(ctx.fold(t, N, chal).download((1, 4)))[0] for t in (d_eq, v1x, vx0, vx1, h, d_num, d_den)]
    assert wm.ints(last) == folded
    assert target == wiring_value(*folded, wm.ints(gamma)[0])
    assert (d_tree.download((2 * N, 4)) == tree_h).all()


def test_sumcheck_wiring_mu20_chain_closed_by_existing_kernels(ctx):
    _big(ctx, 20, 8100)


@pytest.mark.skipif(os.environ.get("ZK_SLOW_TESTS") != "1", reason="mu = 24: 2.5 GiB of tables and 3.5 GiB of scratch (ZK_SLOW_TESTS=1)")
def test_sumcheck_wiring_mu24_chain_closed_by_existing_kernels(ctx):
    _big(ctx, 24, 8200)


@pytest.mark.parametrize("mu", [10, 16])
def test_end_to_end_prove_and_verify(ctx, mu):
    from zkhip import dist_primitive as dp
    from zkhip import pairing as pr
    from zkhip import wiring as wr
    from zkhip.field import fr_mont

    def prove(break_wire=None):
        w, sid, ssigma, alpha, beta, gamma, tau, chal, s = wr.permuted_circuit(ctx, mu, 7, break_wire)
        cub = dp.PolynomialCommitmentCub.new(ctx, s)
        return wr.wiring_prove(ctx, cub.mature(), w, sid, ssigma, 1 << mu, alpha, beta, gamma, tau, chal), (alpha, beta, gamma, tau, chal), s

    proof, sc, s = prove()
    chal = sc[4]
    pg2 = pr.powers_of_g2(wm.ints(s))
    pg2_mu = [pg2[0]] + pg2[2:]
    vk_mu, vk_mu1 = wr.verifying_keys(ctx, pg2)
    assert wr.verify_rounds(proof, *sc) is True
    assert wr.wiring_verify(ctx, vk_mu, vk_mu1, proof, *sc) is True
    vp = wr.v_points(chal)

    def host_verdict(p):
        """the same decision with the host big-int pairing on the same openings"""
        return (wr.verify_rounds(p, *sc) and all(dp.verify(pg2_mu, c, v, pf, chal) for c, v, pf in p["openings"])
                and all(dp.verify(pg2, p["v_commitment"], v, pf, pt) for (v, pf), pt in zip(p["v_openings"], vp)))

    def clone(p):
        return {"rounds": p["rounds"].copy(), "openings": [(c.copy(), v.copy(), pf.copy()) for c, v, pf in p["openings"]],
                "v_commitment": p["v_commitment"].copy(), "v_openings": [(v.copy(), pf.copy()) for v, pf in p["v_openings"]]}

    muts = {}
    muts["broken wire"] = prove(break_wire=5)[0]
    assert wr.failed_checks(muts["broken wire"], *sc) == [3]
    m = clone(proof)
    m["rounds"][mu // 2][3] = fr_mont(wm.ints(m["rounds"][mu // 2][3])[0] + 1)
    muts["round value + 1"] = m
    m = clone(proof)
    c, v, pf = m["openings"][2]
    m["openings"][2] = (c, fr_mont(wm.ints(v)[0] + 1), pf)
    muts["opened value + 1"] = m
    m = clone(proof)
    v, pf = m["v_openings"][2]
    m["v_openings"][2] = (fr_mont(wm.ints(v)[0] + 1), pf)
    muts["opened tree value + 1"] = m
    m = clone(proof)
    v, pf = m["v_openings"][3]
    other = po.g1_add(pt_ints(jac_norm_to_affine(pf[mu // 2])), po.G1_GEN)  # another valid curve point
    pf[mu // 2] = np.concatenate([np.array(po.fq_to_mont_limbs(other[0]) + po.fq_to_mont_limbs(other[1]), dtype=np.uint64), pf[mu // 2][12:]])
    muts["v opening proof point replaced"] = m
    for name, mp in muts.items():
        assert wr.wiring_verify(ctx, vk_mu, vk_mu1, mp, *sc) is False, name
        assert host_verdict(mp) is False, name
    assert host_verdict(proof) is True
    # the proof-point mutation passes the field checks: it is the pairing that rejects it, on both sides
    bad = muts["v opening proof point replaced"]
    assert wr.verify_rounds(bad, *sc) is True
    for k, ((v, pf), pt) in enumerate(zip(bad["v_openings"], vp)):
        assert dp.verify_device(ctx, vk_mu1, bad["v_commitment"], v, pf, pt) == (k != 3), k
    # a mu-variate opening does NOT verify against the full key
    c, v, pf = proof["openings"][0]
    assert dp.verify_device(ctx, dp.pcs_vk(ctx, pg2[: mu + 1]), c, v, pf, chal) is False


def test_zero_denominator_is_reported(ctx):
    """den[K] = 0 surfaces as ZK_ERR_DIV_ZERO from zk_fr_batch_div (ZeroDivisionError in the Python host)"""
    from zkhip import dist_primitive as dp
    from zkhip import wiring as wr
    from zkhip.field import fr_from_mont, fr_mont

    mu = 4
    w, sid, ssigma, alpha, beta, gamma, tau, chal, s = wr.permuted_circuit(ctx, mu, 3)
    K = 6
    wk, sk = (fr_from_mont(b.download((1, 4), offset=32 * K)[0]) for b in (w, ssigma))
    beta0 = fr_mont(-(wk + fr_from_mont(alpha) * sk))  # w[K] + alpha ssigma[K] + beta = 0
    cub = dp.PolynomialCommitmentCub.new(ctx, s)
    with pytest.raises(ZeroDivisionError):
        wr.wiring_prove(ctx, cub.mature(), w, sid, ssigma, 1 << mu, alpha, beta0, gamma, tau, chal)


def test_sumcheck_wiring_errors_leave_outputs_untouched(ctx):
    import zkhip
    from zkhip.api import _h, _ptr

    mu = 4
    d = ctx.to_device(rand_fr(2 << mu, 1))
    chal, gamma = rand_fr(mu, 2), rand_fr(1, 3)[0]
    out = np.full((mu, 4, 4), 0xA5, dtype=np.uint64)
    last = np.full((7, 4), 0xA5, dtype=np.uint64)
    p = _ptr(d)

    def call(ptrs, N, g=gamma, ch=chal):
        return ctx.lib.zk_sumcheck_wiring(ctx.h, *ptrs, N, None if g is None else _h(g), None if ch is None else _h(ch), _h(out), _h(last))

    for N in (0, 1, 3, 12, 17, 1 << 36):
        assert call([p] * 4, N) == -1, N  # ZK_ERR_INVALID
    for k in range(4):
        ptrs = [p] * 4
        ptrs[k] = None
        assert call(ptrs, 1 << mu) == -1
    assert call([p] * 4, 1 << mu, g=None) == -1
    assert call([p] * 4, 1 << mu, ch=None) == -1
    assert ctx.lib.zk_sumcheck_wiring(ctx.h, *([p] * 4), 1 << mu, _h(gamma), _h(chal), None, _h(last)) == -1
    assert ctx.lib.zk_sumcheck_wiring(ctx.h, *([p] * 4), 1 << mu, _h(gamma), _h(chal), _h(out), None) == -1
    assert (out == 0xA5).all() and (last == 0xA5).all()
    with pytest.raises(zkhip.ZkError):
        ctx.sumcheck_wiring(d, d, d, d, 12, gamma, chal)


def test_second_proof_after_arena_plan_import_allocates_nothing():
    import zkhip

    def work(c):
        mu = 15
        chal, gamma = rand_fr(mu, 12), rand_fr(1, 13)[0]
        eq, num, den = (c.to_device(rand_fr(1 << mu, 20 + i)) for i in range(3))
        tree = c.to_device(rand_fr(2 << mu, 24))
        return c.sumcheck_wiring(eq, tree, num, den, 1 << mu, gamma, chal)

    a = zkhip.Ctx(0)
    ref = work(a)
    plan = a.arena_plan_export()
    assert plan[2:].any()
    a.close()
    b = zkhip.Ctx(0)
    b.arena_plan_import(plan)
    before = b.arena_plan_export()
    got = work(b)
    assert (b.arena_plan_export() == before).all(), "the wiring sumcheck grew an arena although the plan was imported"
    assert (ref[0] == got[0]).all() and (ref[1] == got[1]).all()
    b.close()
