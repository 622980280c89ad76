"""
Wiring PermCheck without a GPU: the big-int model (wiring_model.py) against the existing oracle, the product code's host verifier
(zkhip.wiring.verify_rounds) against the model's transcripts, the verifying-key shift of lower-level openings with the host big-int
pairing, the symbol's presence, and the test circuit's permutation.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import pyoracle as po
import wiring_model as wm

R = po.R_MOD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _setup(mu, seed, break_wire=None):
    rng = po.SplitMix64(seed * 37 + 3)
    alpha, beta, gamma = rng.fr(), rng.fr(), rng.fr()
    tau, chal = rng.fr_vec(mu), rng.fr_vec(mu)
    assert all(t not in (0, 1) for t in tau)  # eq(tau, .) is then non-zero on the whole cube
    w, sid, ssigma = wm.shuffled_circuit(mu, seed, break_wire)
    tabs, tree = wm.tables(w, sid, ssigma, alpha, beta, tau)
    return dict(w=w, sid=sid, ssigma=ssigma, alpha=alpha, beta=beta, gamma=gamma, tau=tau, chal=chal, tabs=tabs, tree=tree)


def _record(rounds, c, chal=None):
    """the model's transcript in the product code's record layout; opened values by the ORACLE's fix_variable"""
    from zkhip.wiring import OPENED

    chal = c["chal"] if chal is None else chal
    mu = len(chal)
    opened = {k: po.fix_variable(c[k], chal)[0] for k in OPENED}
    v_opened = [po.fix_variable(c["tree"], pt)[0] for pt in wm.v_points(chal)]
    z18 = np.zeros(18, dtype=np.uint64)
    rec = {"rounds": np.stack([wm.mont(p[:4]) for p in rounds]),
           "openings": [(z18, wm.mont([opened[k]])[0], np.zeros((mu, 18), dtype=np.uint64)) for k in OPENED],
           "v_commitment": z18,
           "v_openings": [(wm.mont([v])[0], np.zeros((mu + 1, 18), dtype=np.uint64)) for v in v_opened]}
    return rec, opened, v_opened


def _scalars(c):
    return [wm.mont([c[k]])[0] for k in ("alpha", "beta", "gamma")] + [wm.mont(c["tau"]), wm.mont(c["chal"])]


@pytest.mark.parametrize("mu", range(1, 9))
def test_model_chain_and_oracle_anchor(mu):
    c = _setup(mu, 100 + mu)
    N, tabs, tree, chal, gamma = 1 << mu, c["tabs"], c["tree"], c["chal"], c["gamma"]
    # the tree and its views are the oracle's
    vx0, vx1, v1x = po.acc_product(tabs["h"])
    assert tree == po.product_tree(tabs["h"])
    assert (tabs["vx0"], tabs["vx1"], tabs["v1x"]) == (vx0, vx1, v1x)
    assert all(d * h % R == n for n, d, h in zip(tabs["num"], tabs["den"], tabs["h"]))
    assert tree[2 * N - 2] == 1 and tree[2 * N - 1] == 0
    rounds, last = wm.sumcheck_wiring(tabs, gamma, chal, evals=5)
    # every term of F vanishes on the cube, so the claimed sum is 0
    assert all(wm.F(*[tabs[k][x] for k in wm.TABLES], gamma) == 0 for x in range(N))
    assert (rounds[0][0] + rounds[0][1]) % R == 0
    for i in range(1, mu):
        assert (rounds[i][0] + rounds[i][1]) % R == wm.interpolate4(rounds[i - 1][:4], chal[i - 1])
    for p in rounds:  # degree 3: the fifth value lies on the cubic through the first four
        assert p[4] == wm.interpolate4(p[:4], 4)
    anchor = [po.fix_variable(tabs[k], chal)[0] for k in wm.TABLES]  # shares nothing with the model
    assert last == anchor
    assert wm.interpolate4(rounds[-1][:4], chal[-1]) == wm.F(*anchor, gamma)
    assert anchor[0] == wm.eq_point(c["tau"], chal)
    # num (and den) at r follow from the openings of w, sid, ssigma
    wr, sr, ssr = (po.fix_variable(c[k], chal)[0] for k in ("w", "sid", "ssigma"))
    assert anchor[5] == (wr + c["alpha"] * sr + c["beta"]) % R
    assert anchor[6] == (wr + c["alpha"] * ssr + c["beta"]) % R
    # the four views at r are the tree at four (mu + 1)-points; the fifth point is the grand product
    at = [po.fix_variable(tree, pt)[0] for pt in wm.v_points(chal)]
    assert at[:4] == [anchor[4], anchor[1], anchor[2], anchor[3]]
    assert at[4] == tree[2 * N - 2]


@pytest.mark.parametrize("mu", [1, 2, 3, 6])
def test_broken_wire_changes_the_grand_product(mu):
    for K in {0, (1 << mu) - 1, (1 << mu) // 3}:
        c = _setup(mu, 150 + mu, break_wire=K)
        assert c["tree"][2 * (1 << mu) - 2] != 1
        # the sumcheck itself still closes (the tree is consistent): it is check 3 that fails
        rounds, _ = wm.sumcheck_wiring(c["tabs"], c["gamma"], c["chal"])
        rec, opened, v_opened = _record(rounds, c)
        assert wm.verify_rounds(rounds, opened, v_opened, c["alpha"], c["beta"], c["gamma"], c["tau"], c["chal"]) == [3]


@pytest.mark.parametrize("mu", [1, 2, 5, 8])
def test_verify_rounds_accepts_and_rejects(mu):
    from zkhip.wiring import OPENED, V_POINTS, failed_checks, verify_rounds

    c = _setup(mu, 200 + mu)
    rounds, _ = wm.sumcheck_wiring(c["tabs"], c["gamma"], c["chal"])
    rec, opened, v_opened = _record(rounds, c)
    sc = _scalars(c)
    assert wm.verify_rounds(rounds, opened, v_opened, c["alpha"], c["beta"], c["gamma"], c["tau"], c["chal"]) == []
    assert verify_rounds(rec, *sc) is True
    # (a) a broken wire: the grand product is not 1
    for K in {0, (1 << mu) - 1, (1 << mu) // 3}:
        b = _setup(mu, 200 + mu, break_wire=K)
        br, _ = wm.sumcheck_wiring(b["tabs"], b["gamma"], b["chal"])
        assert failed_checks(_record(br, b)[0], *sc) == [3]
    # (b) every single round value + 1
    for i in range(mu):
        for t in range(4):
            mut = [list(p) for p in rounds]
            mut[i][t] = (mut[i][t] + 1) % R
            assert verify_rounds(_record(mut, c)[0], *sc) is False, (i, t)
    # (c) every opened value + 1
    for k in range(len(OPENED)):
        mut, _, _ = _record(rounds, c)
        cm, v, pf = mut["openings"][k]
        mut["openings"][k] = (cm, wm.mont([wm.ints(v)[0] + 1])[0], pf)
        assert verify_rounds(mut, *sc) is False, OPENED[k]
    for k in range(len(V_POINTS)):
        mut, _, _ = _record(rounds, c)
        v, pf = mut["v_openings"][k]
        mut["v_openings"][k] = (wm.mont([wm.ints(v)[0] + 1])[0], pf)
        assert verify_rounds(mut, *sc) is False, V_POINTS[k]
        assert failed_checks(mut, *sc) == ([3] if k == 4 else [2])
    # (d) a swapped pair of challenges
    if mu >= 2:
        sw = list(c["chal"])
        sw[0], sw[1] = sw[1], sw[0]
        assert verify_rounds(rec, *sc[:4], wm.mont(sw)) is False
    # wrong shapes are refused, not accepted
    assert verify_rounds(rec, *sc[:3], sc[3][:-1], sc[4][:-1]) is False
    short = dict(rec, v_openings=rec["v_openings"][:4])
    assert verify_rounds(short, *sc) is False
    assert verify_rounds(dict(rec, openings=rec["openings"][:2]), *sc) is False


def test_round_poly_at_is_the_models_interpolation():
    from zkhip.wiring import round_poly_at

    rng = po.SplitMix64(9)
    ev, x = rng.fr_vec(4), rng.fr()
    for k in range(4):
        assert round_poly_at(ev, k) == ev[k]
    assert round_poly_at(ev, x) == wm.interpolate4(ev, x)


@pytest.mark.parametrize("mu", [1, 2])
def test_lower_level_opening_verifies_against_the_shifted_key(mu):
    """the SRS has mu + 1 variables; level mu uses the LAST mu of them, so a mu-variate opening verifies against
    [g2, s_1 g2, .., s_mu g2] = [pg2[0]] + pg2[2:] and fails against the full powers_of_g2 (host big-int pairing)"""
    from zkhip import pairing as pr

    rng = po.SplitMix64(300 + mu)
    s = rng.fr_vec(mu + 1)
    levels = po.srs_powers(po.G1_GEN, s)
    pg2 = pr.powers_of_g2(s)
    table, point = rng.fr_vec(1 << mu), rng.fr_vec(mu)
    com = po.commit(levels, table)
    value, proof = po.open_(levels, table, point)
    assert value == po.fix_variable(table, point)[0]
    assert pr.verify(po.G1_GEN, [pg2[0]] + pg2[2:], com, value, proof, point) is True
    assert pr.verify(po.G1_GEN, pg2, com, value, proof, point) is False
    # the tree's level: mu + 1 variables, the full list
    tree, pt1 = rng.fr_vec(2 << mu), rng.fr_vec(mu + 1)
    v1, pf1 = po.open_(levels, tree, pt1)
    assert pr.verify(po.G1_GEN, pg2, po.commit(levels, tree), v1, pf1, pt1) is True


def test_symbol_declared_exported_and_bound():
    import zkhip
    from zkhip import _lib

    hdr = open(os.path.join(ROOT, "include", "zkhip.h")).read()
    bound = {s[0] for s in _lib.SYMBOLS}
    exported = subprocess.run(["nm", "-D", "--defined-only", zkhip.LIB_PATH], capture_output=True, text=True, check=True).stdout
    name = "zk_sumcheck_wiring"
    assert re.search(r"\bint %s\(" % name, hdr)
    assert name in bound
    assert re.search(r"\bT %s\b" % name, exported)


@pytest.mark.parametrize("mu", [1, 2, 3, 4, 9])
def test_block_permutation_is_a_permutation_that_keeps_the_wire_values(mu):
    from zkhip.wiring import block_permutation, wire_values

    for seed in (0, 1, 2, 3, 7):
        sigma = block_permutation(mu, seed)
        n = 1 << mu
        assert sorted(sigma.tolist()) == list(range(n))
        w = wire_values(mu, seed)
        assert w.shape == (n, 4) and (w[sigma.astype(np.int64)] == w).all()
        # one cycle per aligned block of min(8, n)
        blk = min(8, n)
        i, seen = 0, 0
        while True:
            i, seen = int(sigma[i]), seen + 1
            if i == 0:
                break
        assert seen == blk
