"""
The lookup argument without a GPU: the big-int model of the identity and its sumcheck (lookup_model.py), and the verifier's field
arithmetic of zkhip.lookup on records the model wrote.
"""
import numpy as np
import pytest

import lookup_model as lm
import pyoracle as po

R = po.R_MOD


def _sample(n, seed, distinct=None):
    """the product's sampler as ints: (t, f, idx)"""
    from zkhip import lookup as lk

    t, f, idx = lk.sample_lookup(n, seed, distinct)
    return lm.ints(t), lm.ints(f), [int(i) for i in idx]


def _round0_sum(f, t, m, seed, hf=None):
    rng = po.SplitMix64(seed)
    beta, gamma, lam = rng.fr_vec(3)
    n = len(f).bit_length() - 1
    tabs = lm.tables(f, t, m, beta, lam, rng.fr_vec(n), hf=hf)
    rounds, _ = lm.sumcheck_lookup(tabs, gamma, rng.fr_vec(n))
    return (rounds[0][0] + rounds[0][1]) % R, tabs


@pytest.mark.parametrize("n,distinct", [(1, 1), (2, 3), (4, 5), (5, 32), (6, None)])
def test_the_chain_closes_at_zero_for_satisfied_samples(n, distinct):
    t, f, idx = _sample(n, 3 + n, distinct)
    assert all(f[x] == t[idx[x]] for x in range(1 << n))
    rng = po.SplitMix64(100 + n)
    beta, gamma, lam = rng.fr_vec(3)
    tau, chal = rng.fr_vec(n), rng.fr_vec(n)
    tabs = lm.tables(f, t, lm.multiplicities(idx, 1 << n), beta, lam, tau)
    rounds, last = lm.sumcheck_lookup(tabs, gamma, chal)
    ok, end = lm.chain(rounds, chal)
    assert ok and end == lm.L(*last, gamma)
    E, df, dt, m, hf, ht = last
    assert E == lam * lm.eq_point(tau, chal) % R


def test_round_zero_is_not_zero_for_wrong_witnesses():
    n = 4
    t, f, idx = _sample(n, 9, 6)
    m = lm.multiplicities(idx, 1 << n)
    assert _round0_sum(f, t, m, 1)[0] == 0
    outside = list(f)
    outside[5] = (max(t) + 1) % R  # not a table entry (the entries are random: their maximum plus one is none of them)
    assert outside[5] not in t and _round0_sum(outside, t, m, 1)[0] != 0
    off = list(m)
    off[idx[0]] += 1
    assert _round0_sum(f, t, off, 1)[0] != 0
    _, tabs = _round0_sum(f, t, m, 1)
    wrong = list(tabs["hf"])
    wrong[7] = (wrong[7] + 1) % R
    assert _round0_sum(f, t, m, 1, hf=wrong)[0] != 0


@pytest.fixture(scope="module")
def model_run():
    n = 4
    t, f, idx = _sample(n, 2, 7)
    c_t = lm.fake_commitment("t", t)
    mo = lm.prove(f, t, idx, c_t, lm.fake_commitment)
    return {"n": n, "commitment": c_t, "pcs": None}, mo, lm.model_record(mo)


def _bump(a, idx):
    a = np.array(a, copy=True)
    a[idx] = lm.mont([(lm.ints(a[idx])[0] + 1) % R])[0]
    return a


def test_failed_checks_on_model_records(model_run):
    from zkhip import lookup as lk

    vk, mo, rec = model_run
    assert lk.failed_checks(vk, rec) == [] and lk.failed_checks(vk, rec, finals=lm.mont(mo["finals"])) == []
    assert lk.field_checks(vk, rec) is True
    # the first failing check is the one reported (a tampered part changes every challenge drawn after it)
    assert lk.failed_checks(vk, dict(rec, rounds=_bump(rec["rounds"], (2, 1)))) == [1]
    assert lk.failed_checks(vk, dict(rec, rounds=_bump(rec["rounds"], (vk["n"] - 1, 3)))) == [2]  # p(3) of the last round: only its value at r moves
    assert lk.failed_checks(vk, dict(rec, values=_bump(rec["values"], 3))) == [2]  # a claimed value enters the identity first
    assert lk.failed_checks(vk, dict(rec, batch=dict(rec["batch"], rounds=_bump(rec["batch"]["rounds"], (1, 0))))) == [3]
    wrong_final = _bump(lm.mont(mo["finals"]), 2)
    assert lk.failed_checks(vk, rec, finals=wrong_final) == [3]
    assert lk.failed_checks(vk, dict(rec, rounds=rec["rounds"][:-1])) == [0]
    assert lk.failed_checks(vk, dict(rec, batch=dict(rec["batch"], rounds=rec["batch"]["rounds"][1:]))) == [0]
    assert lk.failed_checks(vk, {k: v for k, v in rec.items() if k != "values"}) == [0]
    assert lk.failed_checks(dict(vk, n=5), rec) == [0]


def test_a_wrong_provers_record_is_rejected():
    """hf wrong at one row, committed as it is: the chain cannot start at 0"""
    from zkhip import lookup as lk

    n = 3
    t, f, idx = _sample(n, 4, 4)
    c_t = lm.fake_commitment("t", t)
    hf_of = lambda hf: [(v + 1) % R if x == 2 else v for x, v in enumerate(hf)]
    rec = lm.model_record(lm.prove(f, t, idx, c_t, lm.fake_commitment, hf_of=hf_of))
    assert [1] == lk.failed_checks({"n": n, "commitment": c_t, "pcs": None}, rec)


def test_the_replay_equals_the_models_schedule(model_run):
    from zkhip import lookup as lk

    vk, mo, rec = model_run
    c = lk.challenges(vk, rec)
    for key in ("beta", "gamma", "lambda", "b_alpha"):
        assert lm.ints(c[key]) == [mo[key]], key
    for key in ("tau", "chal", "rho"):
        assert lm.ints(c[key]) == mo[key], key
    assert lk.challenges(vk, rec, label=b"other")["beta"].tolist() != c["beta"].tolist()


def test_the_sampler():
    from zkhip import lookup as lk

    t, f, idx = lk.sample_lookup(5, 1, 9)
    assert t.shape == (32, 4) and f.shape == (32, 4) and idx.dtype == np.uint32 and idx.max() < 9
    assert len({tuple(r) for r in t.tolist()}) == 9 and (t[9:] == t[8]).all() and (f == t[idx]).all()
    assert lk.sample_digest(t, f, idx) == lk.sample_digest(*lk.sample_lookup(5, 1, 9)) != lk.sample_digest(*lk.sample_lookup(5, 2, 9))
    with pytest.raises(ValueError):
        lk.sample_lookup(3, 1, 9)
