"""
Gate ZeroCheck without a GPU: the big-int model (zerocheck_model.py) against the existing oracle, and the product code's host
verifier (zkhip.zerocheck.verify_rounds, eq_eval) against the model's transcripts.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import pyoracle as po
import zerocheck_model as zm

R = po.R_MOD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _setup(n, seed, **kw):
    rng = po.SplitMix64(seed * 31 + 5)
    tau, chal = rng.fr_vec(n), rng.fr_vec(n)
    assert all(t not in (0, 1) for t in tau)  # eq(tau, .) is then non-zero on the whole cube
    tabs = zm.circuit(n, seed, **kw)
    tabs["eq"] = zm.eq_table(tau)
    return tabs, tau, chal


def _record(rounds, tabs, chal):
    """the model's transcript in the product code's record layout; opened values by the ORACLE's fix_variable"""
    from zkhip.zerocheck import OPENED

    opened = {k: po.fix_variable(tabs[k], chal)[0] for k in OPENED}
    rec = {"rounds": np.stack([zm.mont(p) for p in rounds]),
           "openings": [(np.zeros(18, dtype=np.uint64), zm.mont([opened[k]])[0], np.zeros((len(chal), 18), dtype=np.uint64)) for k in OPENED]}
    return rec, opened


@pytest.mark.parametrize("n", range(1, 9))
def test_model_chain_and_oracle_anchor(n):
    tabs, tau, chal = _setup(n, 100 + n, satisfied=False)
    rounds, last = zm.sumcheck_gate(tabs, chal)
    assert len(rounds) == n and all(len(p) == 5 for p in rounds)
    # the claimed sum is the plain sum of G over the cube
    total = sum(zm.gate(*[tabs[k][x] for k in zm.TABLES]) for x in range(1 << n)) % R
    assert (rounds[0][0] + rounds[0][1]) % R == total
    for i in range(1, n):
        assert (rounds[i][0] + rounds[i][1]) % R == zm.interpolate5(rounds[i - 1], chal[i - 1])
    anchor = [po.fix_variable(tabs[k], chal)[0] for k in zm.TABLES]  # shares nothing with the model
    assert last == anchor
    assert zm.interpolate5(rounds[-1], chal[-1]) == zm.gate(*anchor)
    assert anchor[0] == zm.eq_point(tau, chal)
    assert sum(tabs["eq"]) % R == 1


@pytest.mark.parametrize("n", [1, 2, 5, 8])
def test_verify_rounds_accepts_and_rejects(n):
    from zkhip.zerocheck import OPENED, verify_rounds

    tabs, tau, chal = _setup(n, 200 + n)
    rounds, _ = zm.sumcheck_gate(tabs, chal)
    rec, opened = _record(rounds, tabs, chal)
    tm, cm = zm.mont(tau), zm.mont(chal)
    assert zm.verify_rounds(rounds, opened, tau, chal)
    assert verify_rounds(rec, tm, cm) is True
    # (a) one broken gate: the claimed sum is eq(tau, K) != 0
    for K in {0, (1 << n) - 1, (1 << n) // 3}:
        bt, _, _ = _setup(n, 200 + n, break_gate=K)
        br, _ = zm.sumcheck_gate(bt, chal)
        assert (br[0][0] + br[0][1]) % R == (-bt["eq"][K]) % R != 0
        assert verify_rounds(_record(br, bt, chal)[0], tm, cm) is False
    # (b) every single round value + 1
    for i in range(n):
        for t in range(5):
            mut = [list(p) for p in rounds]
            mut[i][t] = (mut[i][t] + 1) % R
            assert verify_rounds(_record(mut, tabs, chal)[0], tm, cm) is False, (i, t)
    # (c) every opened value + 1
    for k in range(len(OPENED)):
        mut, _ = _record(rounds, tabs, chal)
        c, v, pf = mut["openings"][k]
        mut["openings"][k] = (c, zm.mont([zm.ints(v)[0] + 1])[0], pf)
        assert verify_rounds(mut, tm, cm) is False, OPENED[k]
    # (d) a swapped pair of challenges
    if n >= 2:
        sw = list(chal)
        sw[0], sw[1] = sw[1], sw[0]
        assert verify_rounds(rec, tm, zm.mont(sw)) is False
    # wrong shapes are refused, not accepted
    assert verify_rounds(rec, tm[:-1], cm[:-1]) is False


@pytest.mark.parametrize("n", [1, 3, 7, 10])
def test_eq_eval_against_folded_model_table(n):
    from zkhip.zerocheck import eq_eval, round_poly_at

    rng = po.SplitMix64(77 + n)
    tau, r = rng.fr_vec(n), rng.fr_vec(n)
    assert eq_eval(tau, r) == po.fix_variable(zm.eq_table(tau), r)[0]
    ev = rng.fr_vec(5)
    for x in (0, 1, 2, 3, 4):
        assert round_poly_at(ev, x) == ev[x]
    assert round_poly_at(ev, r[0]) == zm.interpolate5(ev, r[0])


def test_symbols_declared_exported_and_bound():
    import zkhip
    from zkhip import _lib

    hdr = open(os.path.join(ROOT, "include", "zkhip.h")).read()
    bound = {s[0] for s in _lib.SYMBOLS}
    exported = subprocess.run(["nm", "-D", "--defined-only", zkhip.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("zk_eq_table", "zk_sumcheck_gate"):
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in bound, name
        assert re.search(r"\bT %s\b" % name, exported), name
