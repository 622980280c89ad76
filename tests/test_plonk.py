"""
One-circuit HyperPlonk without a GPU: the big-int model of the three-column wiring sumcheck (plonk_model.py) against its own
invariants and pyoracle, the verifier's closed forms against explicit tables, zkhip.plonk.field_checks on the model prover's records,
the test-circuit generator, and the presence of the new entry points in the built library and the header.  The pairing step needs
the device: the opening proofs of a record are all-zero here, and a flip inside them is the pairing's to see (tests/test_gpu_plonk.py).
"""
import ctypes
import os

import numpy as np
import pytest

import plonk_model as pm
import pyoracle as po
import wiring_model as wm
import zerocheck_model as zm

R = po.R_MOD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("zk_sumcheck_perm3", "zk_sumcheck_perm3_fs", "zk_perm3_terms")


def _rng_vec(n, seed):
    return po.SplitMix64(seed).fr_vec(n)


# ---- the eleven-table sumcheck ----
@pytest.mark.parametrize("mu", range(1, 9))
def test_model_chain_degree_and_last_values(mu):
    w, ss = pm.random_columns(mu, 40 + mu)
    alpha, beta, gamma = _rng_vec(3, mu)
    tau, chal = _rng_vec(mu, 100 + mu), _rng_vec(mu, 200 + mu)
    tabs, tree = pm.tables(w, ss, alpha, beta, tau)
    assert tree == po.product_tree(tabs["h"])
    rounds, last = pm.sumcheck_perm3(tabs, gamma, chal, evals=7)
    target = 0
    for p, r in zip(rounds, chal):
        assert (p[0] + p[1]) % R == target  # the chain, from a claimed sum of 0
        assert pm.interpolate(p[:6], 6) == p[6]  # degree 5: the seventh value lies on the quintic through the first six
        target = pm.interpolate(p[:6], r)
    assert last == [po.fix_variable(tabs[k], chal)[0] for k in pm.TABLES]
    assert target == pm.F(*last, gamma)


@pytest.mark.parametrize("mu", range(2, 9))
def test_grand_product_of_generated_circuits(mu):
    from zkhip import plonk

    alpha, beta = _rng_vec(2, mu)
    for kw, want_one in (({}, True), ({"break_wire": (1 << mu) - 1}, False)):
        t = pm.circuit_ints(plonk.sample_circuit(mu, 3, **kw))
        N = 1 << mu
        _n, _d, _P, _Q, h = pm.terms([t["a"], t["b"], t["c"]], [t["s0"], t["s1"], t["s2"]], alpha, beta)
        tree = wm.tree_of(h)
        assert tree == po.product_tree(h)
        assert (tree[2 * N - 2] == 1) is want_one


# ---- the verifier's closed forms ----
@pytest.mark.parametrize("mu,l", [(1, 1), (2, 2), (3, 1), (4, 4), (5, 4), (6, 8)])
def test_closed_forms_against_explicit_tables(mu, l):
    from zkhip import plonk

    N = 1 << mu
    r, pi = _rng_vec(mu, 7 * mu + l), _rng_vec(l, 9)
    assert plonk.in_eval(pi, r) == po.fix_variable(pm.in_table(pi, N), r)[0]
    assert plonk.slot_eval(r) == po.fix_variable(list(range(N)), r)[0]
    for j in range(3):  # the slot numbers of column j: j N + x
        assert (j * N + plonk.slot_eval(r)) % R == po.fix_variable([j * N + x for x in range(N)], r)[0]
    ev = _rng_vec(6, mu)
    assert plonk.round_poly_at(ev, r[0]) == pm.interpolate(ev, r[0])


# ---- the generator ----
@pytest.mark.parametrize("mu,seed", [(2, 1), (3, 2), (5, 7), (8, 3), (10, 4)])
def test_generator(mu, seed):
    from zkhip import plonk

    c = plonk.sample_circuit(mu, seed)
    N, l = 1 << mu, c["l"]
    assert l == min(4, N // 2)
    t = pm.circuit_ints(c)
    sigma = t["s0"] + t["s1"] + t["s2"]
    assert sorted(sigma) == list(range(3 * N))  # a permutation of the 3N slots
    vals = t["a"] + t["b"] + t["c"]
    assert all(vals[s] == vals[sigma[s]] for s in range(3 * N))  # values constant on its cycles
    inp = pm.in_table(t["pi"], N)
    assert all(zm.gate(1, t["q1"][x], t["q2"][x], t["a"][x], t["b"][x], t["c"][x], inp[x]) == 0 for x in range(N))  # every gate holds
    assert t["c"][:l] == t["pi"] and not any(t["q1"][:l]) and not any(t["q2"][:l])
    moved = sum(1 for s in range(3 * N) if sigma[s] != s)
    assert moved >= 2 * (N - l)  # every a / b slot past the input rows is on a cycle
    # break_gate: exactly one gate fails; break_wire: every gate holds, a copy constraint fails
    g = pm.circuit_ints(plonk.sample_circuit(mu, seed, break_gate=N - 1))
    assert [x for x in range(N) if zm.gate(1, g["q1"][x], g["q2"][x], g["a"][x], g["b"][x], g["c"][x], inp[x])] == [N - 1]
    bw = pm.circuit_ints(plonk.sample_circuit(mu, seed, break_wire=N - 1))
    assert all(zm.gate(1, bw["q1"][x], bw["q2"][x], bw["a"][x], bw["b"][x], bw["c"][x], inp[x]) == 0 for x in range(N))
    bv = bw["a"] + bw["b"] + bw["c"]
    assert any(bv[s] != bv[sigma[s]] for s in range(3 * N))
    with pytest.raises(ValueError):
        plonk.sample_circuit(mu, seed, break_wire=0)


# ---- field_checks on the model prover's records ----
def words(n, seed):
    """n stand-ins for commitments: [n, 18] words of a seeded stream (the model has no curve arithmetic)"""
    raw = b"".join(int(x).to_bytes(32, "little") for x in po.SplitMix64(seed).fr_vec(5 * n))
    return np.frombuffer(raw, dtype="<u8").astype(np.uint64)[: 18 * n].reshape(n, 18)


def _model_record(mu, seed, vk_seed=None, **kw):
    from zkhip import plonk

    c = plonk.sample_circuit(mu, seed, **kw)
    t = pm.circuit_ints(c)
    vk_comms, comms = words(5, 1000 + (seed if vk_seed is None else vk_seed)), words(3, 2000 + seed)
    m = pm.prove(t, mu, c["l"], vk_comms, comms, lambda tree: words(1, 3000 + tree[0] % 1000)[0])
    vk = {"mu": mu, "l": c["l"], "commitments": vk_comms, "pcs": None}
    return vk, c["public_inputs"], pm.record(m, comms), zm.mont(m["finals"]), zm.mont(m["v_finals"]), m


@pytest.mark.parametrize("mu", [2, 3, 4])
def test_field_checks_accept_model_records(mu):
    from zkhip import plonk

    vk, pi, rec, finals, v_finals, m = _model_record(mu, 5)
    c = plonk.challenges(vk, pi, rec)
    for k in ("alpha", "beta", "gamma", "b_alpha"):
        assert zm.ints(c[k]) == [m[k]], k
    for k in ("tau_p", "r_p", "tau_g", "r_g", "rho_mu", "rho_mu1"):
        assert zm.ints(c[k]) == m[k], k
    assert plonk.failed_checks(vk, pi, rec, finals, v_finals) == []
    assert plonk.field_checks(vk, pi, rec, finals, v_finals) is True
    assert plonk.field_checks(vk, pi, rec) is True  # without the finals: the chains alone
    assert len(plonk.proof_digest(rec)) == 64


def test_field_checks_reject_broken_circuits():
    from zkhip import plonk

    vk, pi, rec, finals, v_finals, _m = _model_record(3, 5, break_gate=6)
    assert 2 in plonk.failed_checks(vk, pi, rec, finals, v_finals) or 3 in plonk.failed_checks(vk, pi, rec, finals, v_finals)
    vk, pi, rec, finals, v_finals, _m = _model_record(3, 5, break_wire=6)
    assert plonk.failed_checks(vk, pi, rec, finals, v_finals) == [5]  # every identity holds; the grand product is not 1


def test_field_checks_reject_every_flip_a_wrong_input_and_another_vk():
    from zkhip import plonk

    mu = 3
    vk, pi, rec, finals, v_finals, _m = _model_record(mu, 5)
    assert plonk.field_checks(vk, pi, rec, finals, v_finals) is True

    def flipped(a, idx):
        a = np.array(a, dtype=np.uint64, copy=True)
        flat = a.reshape(-1)
        flat[idx] ^= np.uint64(1)
        return a

    count = 0
    for key in pm.FIELD_PARTS:
        for idx in range(np.asarray(rec[key]).size):  # every limb of every field
            bad = dict(rec)
            bad[key] = flipped(rec[key], idx)
            assert plonk.field_checks(vk, pi, bad, finals, v_finals) is False, (key, idx)
            count += 1
    for b in ("batch", "v_batch"):
        for idx in range(rec[b]["rounds"].size):
            bad = dict(rec)
            bad[b] = dict(rec[b], rounds=flipped(rec[b]["rounds"], idx))
            assert plonk.field_checks(vk, pi, bad, finals, v_finals) is False, (b, idx)
            count += 1
    assert count == 18 * 4 + 4 * (6 * mu + 5 * mu + 5 + 6 + 5) + 12 * (2 * mu + 1)  # every limb of the record outside the opening proofs
    for key, val in (("mu", mu + 1), ("l", 2 * rec["l"])):
        assert plonk.field_checks(vk, pi, dict(rec, **{key: val}), finals, v_finals) is False
    for idx in range(pi.size):  # a wrong public input
        assert plonk.field_checks(vk, flipped(pi, idx), rec, finals, v_finals) is False, idx
    assert plonk.field_checks(vk, pi[:2], rec, finals, v_finals) is False
    other, *_ = _model_record(mu, 5, vk_seed=6)  # the vk of another seed
    assert plonk.field_checks(other, pi, rec, finals, v_finals) is False
    # wrong finals: the values the batch chains end in are not those of the tables
    assert plonk.field_checks(vk, pi, rec, flipped(finals, 0), v_finals) is False
    assert plonk.field_checks(vk, pi, rec, finals, flipped(v_finals, 0)) is False
    for key in ("p_rounds", "batch", "g_values"):  # malformed
        bad = dict(rec)
        del bad[key]
        assert plonk.failed_checks(vk, pi, bad, finals, v_finals) == [0]


# ---- the entry points exist ----
def test_symbols_in_the_library_and_the_header():
    import zkhip

    header = open(os.path.join(ROOT, "include", "zkhip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "zkhip_sys.rs")).read()
    lib = ctypes.CDLL(zkhip.LIB_PATH)
    for s in SYMBOLS:
        assert f"int {s}(" in header, s
        assert f"pub fn {s}(" in rust, s
        assert getattr(lib, s) is not None, s
    assert all(hasattr(zkhip.Ctx, m) for m in ("perm3_terms", "sumcheck_perm3", "sumcheck_perm3_fs"))
