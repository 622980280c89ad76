"""
The wide Plonk gate without a GPU: the big-int model (widegate_model.py) against the basic gate's model and its own degree, the
test-circuit generator, zkhip.plonk.failed_checks on the model prover's wide records, the pinned digest of a basic record (the basic
kind is unmoved), and the presence of the new entry points in the built library, the header and the Rust binding.
"""
import ctypes
import os

import numpy as np
import pytest

import plonk_model as pm
import pyoracle as po
import widegate_model as wg
import zerocheck_model as zm

R = po.R_MOD
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("zk_sumcheck_gate_wide", "zk_sumcheck_gate_wide_fs")
# zkhip.plonk.proof_digest of the basic model record for (mu, seed) = (4, 7) (widegate_model.basic_model_record), computed by this same
# code on the commit before the wide gate
BASIC_MODEL_DIGEST_4_7 = "ed159608699daa350abd264e00b26c2fdab3140064e3eee39095eb43052e0121"


# ---- the model against closed forms ----
@pytest.mark.parametrize("mu", range(1, 7))
def test_model_reduces_to_the_basic_gate(mu):
    """qH = 0, qL = qR = q1, qM = q2, qO = 1, qC = 0: evaluations 0 .. 4 are zerocheck_model's, 5 .. 7 lie on the quartic through them"""
    N = 1 << mu
    basic = zm.circuit(mu, 30 + mu, satisfied=False)
    basic["eq"] = zm.eq_table(po.SplitMix64(50 + mu).fr_vec(mu))
    chal = po.SplitMix64(70 + mu).fr_vec(mu)
    wide = {"eq": basic["eq"], "qL": basic["q1"], "qR": basic["q1"], "qM": basic["q2"], "qO": [1] * N, "qC": [0] * N, "qH": [0] * N, "a": basic["a"],
            "b": basic["b"], "c": basic["c"], "in": basic["in"]}
    rounds, last = wg.sumcheck_gate_wide(wide, chal)
    b_rounds, b_last = zm.sumcheck_gate(basic, chal)
    for p, q in zip(rounds, b_rounds):
        assert p[:5] == q
        assert [pm.interpolate(q, t) for t in (5, 6, 7)] == p[5:]
    assert [last[wg.TABLES.index(k)] for k in ("eq", "qL", "qM", "a", "b", "c", "in")] == b_last


@pytest.mark.parametrize("mu", range(1, 8))
def test_model_chain_degree_and_last_values(mu):
    tabs = wg.random_tables(mu, 40 + mu)
    chal = po.SplitMix64(200 + mu).fr_vec(mu)
    rounds, last = wg.sumcheck_gate_wide(tabs, chal, evals=9)
    target = sum(wg.W(*[tabs[k][x] for k in wg.TABLES]) for x in range(1 << mu)) % R
    for p, r in zip(rounds, chal):
        assert (p[0] + p[1]) % R == target
        assert pm.interpolate(p[:8], 8) == p[8]  # degree 7: the ninth value lies on the polynomial through the first eight
        assert pm.interpolate(p[:7], 7) != p[7]  # and no lower (random tables)
        target = pm.interpolate(p[:8], r)
    assert last == [po.fix_variable(tabs[k], chal)[0] for k in wg.TABLES]
    assert target == wg.W(*last)


def test_wide_gate_value_is_the_models():
    from zkhip.zerocheck import wide_gate_value

    v = po.SplitMix64(9).fr_vec(11)
    assert wide_gate_value(*v) == wg.W(*v)


# ---- the generator ----
def _broken_cycles(t, N):
    sigma = t["s0"] + t["s1"] + t["s2"]
    vals = t["a"] + t["b"] + t["c"]
    seen, bad = [False] * (3 * N), 0
    for s in range(3 * N):
        if not seen[s]:
            cyc, x = [], s
            while not seen[x]:
                seen[x] = True
                cyc.append(vals[x])
                x = sigma[x]
            bad += len(set(cyc)) > 1
    return bad


@pytest.mark.parametrize("mu", range(2, 9))
def test_generator(mu):
    from zkhip import plonk

    seed = 3
    c = plonk.sample_circuit_wide(mu, seed)
    N, l = 1 << mu, c["l"]
    assert c["gate"] == "wide" and l == min(4, N // 2)
    t = wg.circuit_ints(c)
    assert sorted(t["s0"] + t["s1"] + t["s2"]) == list(range(3 * N))
    assert not any(wg.row_values(t, N))  # the bracket is 0 on every row
    assert _broken_cycles(t, N) == 0     # every cycle of sigma carries one value
    assert t["c"][:l] == t["pi"] and t["qO"][:l] == [1] * l and not any(t[k][x] for k in ("qL", "qR", "qM", "qC", "qH") for x in range(l))
    # the row kinds by their selector patterns: linear, product, S-box, full
    kinds = set()
    for x in range(l, N):
        nz = tuple(k for k in wg.SELECTORS if t[k][x])
        kinds.add({("qL", "qR", "qO", "qC"): 0, ("qM", "qO", "qC"): 1, ("qO", "qC", "qH"): 2, wg.SELECTORS: 3}[nz])
        if nz == ("qO", "qC", "qH"):
            assert t["qH"][x] == 1 and t["qO"][x] == 1 and t["c"][x] == (pow(t["a"][x], 5, R) + t["qC"][x]) % R
    if mu >= 5:
        assert kinds == {0, 1, 2, 3}
    K = N - 1
    g = wg.circuit_ints(plonk.sample_circuit_wide(mu, seed, break_gate=K))
    assert [x for x, v in enumerate(wg.row_values(g, N)) if v] == [K]
    bw = wg.circuit_ints(plonk.sample_circuit_wide(mu, seed, break_wire=K))
    assert not any(wg.row_values(bw, N)) and _broken_cycles(bw, N) == 1
    with pytest.raises(ValueError):
        plonk.sample_circuit_wide(mu, seed, break_wire=0)
    # the streams the two generators share give the same public inputs, picks (so sigma) and trapdoor
    b = plonk.sample_circuit(mu, seed)
    assert all((b[k] == c[k]).all() for k in ("public_inputs", "sigma", "s"))


# ---- failed_checks on the model prover's records ----
def _flip(a, idx):
    a = np.array(a, dtype=np.uint64, copy=True)
    a.reshape(-1)[idx] ^= np.uint64(1)
    return a


@pytest.mark.parametrize("mu", [2, 3, 4])
def test_failed_checks_on_model_records(mu):
    from zkhip import plonk

    vk, pi, rec, finals, v_finals, m = wg.model_record(mu, 5)
    c = plonk.challenges(vk, pi, rec)
    for k in ("tau_p", "r_p", "tau_g", "r_g", "rho_mu", "rho_mu1"):
        assert zm.ints(c[k]) == m[k], k
    assert rec["g_rounds"].shape == (mu, 8, 4) and rec["g_values"].shape == (9, 4)
    assert plonk.failed_checks(vk, pi, rec, finals, v_finals) == []
    assert plonk.field_checks(vk, pi, rec) is True
    # a changed evaluation at node 7 of one round: the chain (the last round's: the closed form)
    for i in range(mu):
        bad = dict(rec, g_rounds=_flip(rec["g_rounds"], (i * 8 + 7) * 4))
        assert plonk.failed_checks(vk, pi, bad, finals, v_finals)[0] == (2 if i + 1 < mu else 3), i  # (6 follows: every later challenge moved)
    # a changed g_values[5] = qH: the closed form (and the batch instance that certifies the value)
    assert wg.G_VALUES[5] == "qH"
    assert plonk.failed_checks(vk, pi, dict(rec, g_values=_flip(rec["g_values"], 5 * 4)), finals, v_finals) == [3, 6]
    # the other gate kind on either side
    b_vk, b_pi, b_rec, b_finals, b_v_finals = wg.basic_model_record(mu, 5)
    assert plonk.failed_checks(b_vk, b_pi, b_rec, b_finals, b_v_finals) == []
    assert plonk.failed_checks(vk, pi, b_rec) == [0] and plonk.failed_checks(b_vk, b_pi, rec) == [0]
    assert plonk.failed_checks(vk, pi, {k: v for k, v in rec.items() if k != "gate"}) == [0]
    assert plonk.failed_checks(dict(vk, gate="other"), pi, rec) == [0]


def test_failed_checks_reject_broken_circuits():
    from zkhip import plonk

    vk, pi, rec, finals, v_finals, _m = wg.model_record(3, 5, break_gate=6)
    assert plonk.failed_checks(vk, pi, rec, finals, v_finals) == [2]  # the claimed sum is not 0
    vk, pi, rec, finals, v_finals, _m = wg.model_record(3, 5, break_wire=6)
    assert plonk.failed_checks(vk, pi, rec, finals, v_finals) == [5]  # every identity holds; the grand product is not 1


# ---- the basic kind is unmoved ----
def test_basic_record_digest_is_pinned():
    from zkhip import plonk

    vk, pi, rec, finals, v_finals = wg.basic_model_record(4, 7)
    assert "gate" not in rec and plonk.failed_checks(vk, pi, rec, finals, v_finals) == []
    assert plonk.proof_digest(rec) == BASIC_MODEL_DIGEST_4_7


# ---- the entry points exist ----
def test_symbols_in_the_library_the_header_and_the_binding():
    import zkhip

    header = open(os.path.join(ROOT, "include", "zkhip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "zkhip_sys.rs")).read()
    lib = ctypes.CDLL(zkhip.LIB_PATH)
    for s in SYMBOLS:
        assert f"int {s}(" in header, s
        assert f"pub fn {s}(" in rust, s
        assert getattr(lib, s) is not None, s
    assert all(hasattr(zkhip.Ctx, m) for m in ("sumcheck_gate_wide", "sumcheck_gate_wide_fs"))
    val = ctypes.c_long(0)
    assert lib.zk_dbg_tune_get(b"gatew_local_e", ctypes.byref(val)) == 0 and val.value == 256
