"""
Big-int statement of the wide Plonk gate's sumcheck and of the one-circuit schedule with it (a helper of test_widegate.py /
test_host_widegate.py / test_gpu_widegate.py, not a test), written from the formulas

    W(x)   = eq(x) [ qL a + qR b + qM a b + qH a^5 - qO c + qC + in ]
    p_i(t) = sum_j W((1 - t) lo_j + t hi_j),  t = 0 .. 7,  then every table is folded with chal[i]

on top of zerocheck_model / plonk_model / batch_open_model / fs_model -- not from the product code.  Values are canonical python ints.
"""
import numpy as np

import batch_open_model as bm
import fs_model as fm
import plonk_model as pm
import pyoracle as po
import wiring_model as wm
import zerocheck_model as zm

R = po.R_MOD
TABLES = ("eq", "qL", "qR", "qM", "qO", "qC", "qH", "a", "b", "c", "in")
SELECTORS = TABLES[1:7]
G_VALUES = SELECTORS + ("a", "b", "c")
BATCH_TABLES = G_VALUES + ("s0", "s1", "s2")
EVALS = 8


def bracket(qL, qR, qM, qO, qC, qH, a, b, c, inp):
    return (qL * a + qR * b + qM * a * b + qH * a * a * a * a * a - qO * c + qC + inp) % R


def W(eq, *rest):
    return eq * bracket(*rest) % R


def sumcheck_gate_wide(tabs, chal, evals=EVALS):
    """tabs: dict name -> list of 2^n ints.  -> (rounds: n x [p(0) .. p(evals-1)], last: the eleven remaining values in TABLES order)"""
    cur = {k: list(tabs[k]) for k in TABLES}
    n = len(cur["eq"]).bit_length() - 1
    rounds = []
    for i in range(n):
        half = len(cur["eq"]) // 2
        ev = []
        for t in range(evals):
            s = 0
            for j in range(half):
                s += W(*[((1 - t) * cur[k][j] + t * cur[k][j + half]) % R for k in TABLES])
            ev.append(s % R)
        rounds.append(ev)
        r = chal[i]
        cur = {k: [((1 - r) * v[j] + r * v[j + half]) % R for j in range(half)] for k, v in cur.items()}
    return rounds, [cur[k][0] for k in TABLES]


def random_tables(n, seed):
    """eleven tables of 2^n uniform ints (the rounds are defined for ANY tables, satisfied or not)"""
    rng = po.SplitMix64(seed)
    return {k: rng.fr_vec(1 << n) for k in TABLES}


def circuit_ints(c):
    """a circuit of zkhip.plonk.sample_circuit_wide -> dict of int tables: the six selectors, a, b, c, s0, s1, s2, pi"""
    N = 1 << c["mu"]
    t = {k: zm.ints(c[k]) for k in G_VALUES}
    sg = [int(x) for x in c["sigma"]]
    t.update(s0=sg[:N], s1=sg[N:2 * N], s2=sg[2 * N:], pi=zm.ints(c["public_inputs"]))
    return t


def row_values(t, N):
    """the bracket of every row of circuit_ints's tables"""
    inp = pm.in_table(t["pi"], N)
    return [bracket(*[t[k][x] for k in G_VALUES], inp[x]) for x in range(N)]


def prove(t, mu, l, vk_commitments, commitments, v_commitment_of, label=b"plonk-wide"):
    """plonk_model.prove with the wide gate: nine vk commitments, eight evaluations per gate round, nine values at r_g, twelve batch tables"""
    N = 1 << mu
    tr = fm.Model(label)
    tr.absorb_u64(mu).absorb_u64(l).absorb(fm.words_bytes(vk_commitments)).absorb_fr(t["pi"])
    alpha, beta = tr.absorb(fm.words_bytes(commitments)).challenges(2)
    w, ss = [t["a"], t["b"], t["c"]], [t["s0"], t["s1"], t["s2"]]
    n, d, _P, _Q, h = pm.terms(w, ss, alpha, beta)
    tree = wm.tree_of(h)
    v_comm = v_commitment_of(tree)
    gamma = tr.absorb(fm.words_bytes(v_comm)).challenge()
    tau_p = tr.challenges(mu)
    tabs = wm.views(tree)
    tabs.update(eq=zm.eq_table(tau_p), n0=n[0], n1=n[1], n2=n[2], d0=d[0], d1=d[1], d2=d[2])
    p_rounds, _last, r_p = fm._stepwise(tr, tabs, lambda cur, ch: pm.sumcheck_perm3(cur, gamma, ch)[0])
    tau_g = tr.challenges(mu)
    gt = {k: t[k] for k in G_VALUES}
    gt.update({"eq": zm.eq_table(tau_g), "in": pm.in_table(t["pi"], N)})
    g_rounds, g_at, r_g = fm._stepwise(tr, gt, lambda cur, ch: sumcheck_gate_wide(cur, ch)[0])
    g_values = [g_at[k] for k in G_VALUES]
    p_values = [bm.evaluate(x, r_p) for x in w + ss]
    v_values = [bm.evaluate(tree, z) for z in wm.v_points(r_p)]
    b_alpha = tr.absorb_fr(g_values).absorb_fr(p_values).absorb_fr(v_values).challenge()
    claims = [(BATCH_TABLES.index(k), r_g, v) for k, v in zip(G_VALUES, g_values)] + [(len(SELECTORS) + i, r_p, v) for i, v in enumerate(p_values)]
    b_rounds, rho_mu, finals = fm.batch_prove(tr, [t[k] for k in BATCH_TABLES], claims, b_alpha)
    v_rounds, rho_mu1, v_finals = fm.batch_prove(tr, [tree], [(0, z, v) for z, v in zip(wm.v_points(r_p), v_values)], b_alpha)
    return {"mu": mu, "l": l, "alpha": alpha, "beta": beta, "gamma": gamma, "tau_p": tau_p, "r_p": r_p, "tau_g": tau_g, "r_g": r_g, "p_rounds": p_rounds,
            "g_rounds": g_rounds, "g_values": g_values, "p_values": p_values, "v_values": v_values, "v_commitment": v_comm, "b_alpha": b_alpha,
            "b_rounds": b_rounds, "rho_mu": rho_mu, "finals": finals, "v_rounds": v_rounds, "rho_mu1": rho_mu1, "v_finals": v_finals, "tree": tree}


def record(m, commitments):
    """the model's run in the product's record layout (zero opening proofs)"""
    return dict(pm.record(m, commitments), gate="wide")


def words(n, seed):
    """n stand-ins for commitments: [n, 18] words of a seeded stream (the model has no curve arithmetic)"""
    raw = b"".join(int(x).to_bytes(32, "little") for x in po.SplitMix64(seed).fr_vec(5 * n))
    return np.frombuffer(raw, dtype="<u8").astype(np.uint64)[: 18 * n].reshape(n, 18)


def model_record(mu, seed, **kw):
    """sample_circuit_wide(mu, seed) proved by the model on stand-in commitments -> (vk, public inputs, record, finals, v_finals, the model's run)"""
    from zkhip import plonk

    c = plonk.sample_circuit_wide(mu, seed, **kw)
    vk_comms, comms = words(9, 1000 + seed), words(3, 2000 + seed)
    m = prove(circuit_ints(c), mu, c["l"], vk_comms, comms, lambda tree: words(1, 3000 + tree[0] % 1000)[0])
    vk = {"gate": "wide", "mu": mu, "l": c["l"], "commitments": vk_comms, "pcs": None}
    return vk, c["public_inputs"], record(m, comms), zm.mont(m["finals"]), zm.mont(m["v_finals"]), m


def basic_model_record(mu, seed):
    """the same for the basic kind (plonk_model.prove on sample_circuit): the record whose digest pins the basic kind"""
    from zkhip import plonk

    c = plonk.sample_circuit(mu, seed)
    vk_comms, comms = words(5, 1000 + seed), words(3, 2000 + seed)
    m = pm.prove(pm.circuit_ints(c), mu, c["l"], vk_comms, comms, lambda tree: words(1, 3000 + tree[0] % 1000)[0])
    vk = {"mu": mu, "l": c["l"], "commitments": vk_comms, "pcs": None}
    return vk, c["public_inputs"], pm.record(m, comms), zm.mont(m["finals"]), zm.mont(m["v_finals"])
