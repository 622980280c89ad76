"""
Batch opening without a GPU: the big-int model (batch_open_model.py) against its own identity and against the oracle's product
sumcheck, and the verifier's field checks of zkhip.batch_open on the model's proofs and on mutants of them.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import batch_open_model as bm
import pyoracle as po

R = po.R_MOD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n,J,K", [(1, 1, 1), (2, 1, 5), (3, 2, 4), (4, 3, 7), (5, 4, 9)])
def test_identity_sum_of_products_equals_the_weighted_claims(n, J, K):
    """sum_x sum_j E_j f_j == sum_k a_k f_{j_k}(z_k), boolean and repeated points included, alpha in {0, 1, r - 1, random}"""
    from zkhip import batch_open as bo

    tables, claims, alpha, _ = bm.instance(n, J, K, 100 + n)
    for a in (0, 1, R - 1, alpha):
        es = bm.combined_eq_tables(J, n, claims, a)
        lhs = sum(e * f for et, ft in zip(es, tables) for e, f in zip(et, ft)) % R
        assert lhs == bm.claimed_sum(claims, a), (n, a)
        assert lhs == bo.claimed_sum(bm.claims_mont(claims), bm.mont([a])[0]), (n, a)  # the product's S


def test_boolean_point_is_a_single_entry():
    from zkhip import batch_open as bo

    n = 4
    claims = [(0, [1] * (n - 1) + [0], 0)]
    es = bm.combined_eq_tables(1, n, claims, 7)
    assert es[0] == [0] * ((1 << n) - 2) + [1, 0]
    # the product's e_j = E_j(rho) at the cube's corners reads the table back
    for x in range(1 << n):
        corner = [(x >> (n - 1 - i)) & 1 for i in range(n)]
        assert bo.eq_coefficients(1, bm.claims_mont(claims), bm.mont([7])[0], bm.mont(corner)) == [es[0][x]]


@pytest.mark.parametrize("n,J,K", [(1, 2, 3), (3, 3, 5), (5, 4, 9)])
def test_triples_are_the_sum_of_the_oracles_product_sumchecks(n, J, K):
    tables, claims, alpha, rho = bm.instance(n, J, K, 200 + n)
    es = bm.combined_eq_tables(J, n, claims, alpha)
    rounds, last_e, last_f = bm.sumcheck_multi(es, tables, rho)
    per = [po.sumcheck_product(e, f, rho) for e, f in zip(es, tables)]
    for i in range(n):
        assert rounds[i] == [sum(p[i][t] for p in per) % R for t in range(3)], i
    assert last_e == bm.eq_coefficients(J, claims, alpha, rho)
    from zkhip import batch_open as bo
    from zkhip.verify import product_round_target

    assert last_e == bo.eq_coefficients(J, bm.claims_mont(claims), bm.mont([alpha])[0], bm.mont(rho))
    target = bo.claimed_sum(bm.claims_mont(claims), bm.mont([alpha])[0])
    for tr, x in zip(rounds, rho):  # the product's chain on the oracle-anchored triples
        assert (tr[0] + tr[1]) % R == target
        target = product_round_target(*tr, x)
    assert target == sum(e * f for e, f in zip(last_e, last_f)) % R
    assert last_f == [po.fix_variable(f, rho)[0] for f in tables]
    # the oracle's verifier accepts the transcript from S, closed by g(rho) = sum_j e_j f_j(rho)
    y = sum(e * f for e, f in zip(last_e, last_f)) % R
    assert po.check_sumcheck_product([tuple(r) for r in rounds] + [(0, y, 0)], rho, bm.claimed_sum(claims, alpha))
    assert bm.evaluate(bm.lincomb(last_e, tables), rho) == y


@pytest.mark.parametrize("n,J,K", [(2, 1, 5), (4, 3, 7), (5, 4, 9)])
def test_failed_checks_accepts_the_models_proofs_and_names_the_mutants_check(n, J, K):
    from zkhip import batch_open as bo

    tables, claims, alpha, rho = bm.instance(n, J, K, 300 + n)
    rec, finals = bm.prove(tables, claims, alpha, rho)
    cm, am, rm, fm = bm.claims_mont(claims), bm.mont([alpha])[0], bm.mont(rho), bm.mont(finals)
    assert bo.failed_checks(J, cm, rec, am, rm) == []
    assert bo.failed_checks(J, cm, rec, am, rm, finals=fm) == []
    assert bo.verify_rounds(J, cm, rec, am, rm, finals=fm) is True
    assert bo.claimed_sum(cm, am) == bm.claimed_sum(claims, alpha)
    assert bo.eq_coefficients(J, cm, am, rm) == bm.eq_coefficients(J, claims, alpha, rho)
    # a flipped limb of one t2 (not the last round's: that one only moves y)
    m = {"rounds": rec["rounds"].copy(), "opening": rec["opening"]}
    m["rounds"][0][2][1] ^= np.uint64(1)
    assert bo.failed_checks(J, cm, m, am, rm, finals=fm) == [1]
    m = {"rounds": rec["rounds"].copy(), "opening": rec["opening"]}
    m["rounds"][n - 1][2][1] ^= np.uint64(1)
    assert bo.failed_checks(J, cm, m, am, rm, finals=fm) == [2]
    # one wrong v_k
    bad = list(claims)
    bad[K // 2] = (bad[K // 2][0], bad[K // 2][1], (bad[K // 2][2] + 1) % R)
    assert bo.failed_checks(J, bm.claims_mont(bad), rec, am, rm, finals=fm) == [1]
    # two claims' points swapped (values kept): S is unchanged, the e_j are not -- the closing value catches it
    a, b = 0, K - 1
    assert claims[a][1] != claims[b][1]
    sw = list(claims)
    sw[a], sw[b] = (claims[a][0], claims[b][1], claims[a][2]), (claims[b][0], claims[a][1], claims[b][2])
    assert bo.failed_checks(J, bm.claims_mont(sw), rec, am, rm) == []
    assert bo.failed_checks(J, bm.claims_mont(sw), rec, am, rm, finals=fm) == [2]
    # a wrong alpha, a wrong rho
    assert bo.failed_checks(J, cm, rec, bm.mont([alpha + 1])[0], rm, finals=fm) == [1]
    r2 = list(rho)
    r2[0] = (r2[0] + 1) % R
    assert bo.failed_checks(J, cm, rec, am, bm.mont(r2), finals=fm) == ([1] if n > 1 else [2])
    r2 = list(rho)
    r2[n - 1] = (r2[n - 1] + 1) % R
    assert bo.failed_checks(J, cm, rec, am, bm.mont(r2), finals=fm) == [2]
    # malformed
    assert bo.failed_checks(J, cm, {"rounds": rec["rounds"][:-1], "opening": rec["opening"]}, am, rm) == [0]
    assert bo.failed_checks(J, cm, {"rounds": rec["rounds"]}, am, rm) == [0]


def test_bad_claims_are_value_errors_not_device_calls():
    from zkhip import batch_open as bo

    z, v = bm.mont([1, 2, 3]), bm.mont([5])[0]
    rho, alpha = bm.mont([4, 5, 6]), bm.mont([9])[0]
    for claims in ([(2, z, v)], [(-1, z, v)], [(0, z[:2], v)], []):
        with pytest.raises(ValueError):
            bo.batch_open_prove(None, None, [None, None], 8, claims, alpha, rho)
        with pytest.raises(ValueError):
            bo.combined_eq_tables(None, 2, 3, claims, alpha)
        assert bo.failed_checks(2, claims, {"rounds": np.zeros((3, 3, 4), dtype=np.uint64), "opening": np.zeros((3, 18), dtype=np.uint64)}, alpha, rho) == [0]


def test_batch_open_check_builds_and_refuses_without_a_gpu():
    host = os.path.join(ROOT, "scalable-collaborative-zksnark_amd", "host")
    subprocess.check_call(["make", "-C", host, "-s", "bin/batch_open_check"])
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([os.path.join(host, "bin", "batch_open_check")], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "no CPU fallback" in r.stderr, (r.returncode, r.stdout, r.stderr)


def test_symbols_declared_exported_and_bound():
    import zkhip
    from zkhip import _lib

    hdr = open(os.path.join(ROOT, "include", "zkhip.h")).read()
    rs = open(os.path.join(ROOT, "rust", "zkhip_sys.rs")).read()
    bound = {s[0] for s in _lib.SYMBOLS}
    exported = subprocess.run(["nm", "-D", "--defined-only", zkhip.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in ("zk_eq_table_acc", "zk_fr_lincomb", "zk_sumcheck_multi"):
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert re.search(r"\bpub fn %s\(" % name, rs), name
        assert name in bound, name
        assert re.search(r"\bT %s\b" % name, exported), name
    assert callable(zkhip.Ctx.eq_table_acc) and callable(zkhip.Ctx.fr_lincomb) and callable(zkhip.Ctx.sumcheck_multi)
