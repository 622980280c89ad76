"""
Big-int statement of the selector-gated three-column lookup and of the one-circuit HyperPlonk schedule WITH it (a helper of
test_plonk_lookup.py / test_gpu_plonk_lookup.py, not a test), written from the formulas

    f = a + zeta b + zeta^2 c,  t = t0 + zeta t1 + zeta^2 t2,  df = beta + f,  dt = beta + t,  hf = qk / df,  ht = m / dt,
    m[y] = #{x : qk(x) = 1, idx[x] = y}
    L(x) = hf(x) - ht(x) + E(x) [ hf(x) df(x) - qk(x) + gamma ( ht(x) dt(x) - m(x) ) ],     E = lambda eq(tau, .),     sum_x L(x) = 0

on top of lookup_model / plonk_model / widegate_model / fs_model -- not from the product code.  Values are canonical python ints mod r.
Commitments cannot be modelled here (no curve arithmetic): the schedule takes them as given words.
"""
import hashlib

import numpy as np

import batch_open_model as bm
import fs_model as fm
import lookup_model as lm
import plonk_model as pm
import pyoracle as po
import widegate_model as wg
import wiring_model as wm
import zerocheck_model as zm

R = po.R_MOD
TABLES = lm.TABLES + ("qk",)  # E, df, dt, m, hf, ht, qk
L_VALUES = ("a", "b", "c", "qk", "t0", "t1", "t2", "m", "hf", "ht")
L_BATCH_TABLES = L_VALUES[3:]


def L(E, df, dt, m, hf, ht, qk, gamma):
    return (hf - ht + E * (hf * df - qk + gamma * (ht * dt - m))) % R


def multiplicities3(w, t, qk, idx, check=True):
    """w = (a, b, c), t = (t0, t1, t2): columns of N ints; qk: N ints; idx: N ints -> m.  check: a selected row must name an entry < N that
    equals its triple and qk must be 0 or 1 (ValueError with the count of bad rows); check=False counts a selected row whatever it holds"""
    N = len(qk)
    m, bad = [0] * N, 0
    for x in range(N):
        if qk[x] == 0:
            continue
        y = idx[x]
        if check and (qk[x] != 1 or y >= N or any(w[j][x] != t[j][y] for j in range(3))):
            bad += 1
            continue
        m[y] += 1
    if bad:
        raise ValueError(f"{bad} of {N} rows")
    return m


def terms(w, t, zeta, beta):
    """-> (df, dt)"""
    N = len(w[0])
    comb = lambda c: [(beta + c[0][x] + zeta * c[1][x] + zeta * zeta * c[2][x]) % R for x in range(N)]
    return comb(w), comb(t)


def tables(w, t, qk, m, zeta, beta, lam, tau):
    """the seven tables of the sumcheck"""
    df, dt = terms(w, t, zeta, beta)
    hf = [q * pow(d, -1, R) % R for q, d in zip(qk, df)]
    ht = [mm * pow(d, -1, R) % R for mm, d in zip(m, dt)]
    return {"E": [lam * e % R for e in zm.eq_table(tau)], "df": df, "dt": dt, "m": [x % R for x in m], "hf": hf, "ht": ht, "qk": list(qk)}


def sumcheck_lookup_sel(tabs, gamma, chal, evals=4):
    """tabs: dict name -> list of 2^n ints.  -> (rounds: n x [p(0) .. p(evals-1)], last: the seven remaining values in TABLES order)"""
    cur = {k: list(tabs[k]) for k in TABLES}
    n = len(cur["E"]).bit_length() - 1
    rounds = []
    for i in range(n):
        half = len(cur["E"]) // 2
        ev = []
        for t in range(evals):
            s = 0
            for j in range(half):
                s += L(*[((1 - t) * cur[k][j] + t * cur[k][j + half]) % R for k in TABLES], gamma)
            ev.append(s % R)
        rounds.append(ev)
        r = chal[i]
        cur = {k: [((1 - r) * v[j] + r * v[j + half]) % R for j in range(half)] for k, v in cur.items()}
    return rounds, [cur[k][0] for k in TABLES]


def random_tables(n, seed):
    """seven tables of 2^n uniform ints (the rounds are defined for ANY tables, satisfied or not)"""
    rng = po.SplitMix64(seed)
    return {k: rng.fr_vec(1 << n) for k in TABLES}


def lookup_ints(c):
    """the lookup part of a circuit of zkhip.plonk.sample_circuit_lookup -> (dict of int tables qk, t0, t1, t2, idx as ints)"""
    return {k: zm.ints(c["lookup"][k]) for k in ("qk", "t0", "t1", "t2")}, [int(i) for i in c["idx"]]


KINDS = {
    None: (b"plonk-lookup", pm.G_VALUES, pm.BATCH_TABLES, lambda cur, ch: zm.sumcheck_gate(cur, ch)[0]),
    "wide": (b"plonk-wide-lookup", wg.G_VALUES, wg.BATCH_TABLES, lambda cur, ch: wg.sumcheck_gate_wide(cur, ch)[0]),
}


def prove(t, lk, idx, mu, l, vk_commitments, commitments, commitment_of, gate=None, check=True):
    """
    The schedule of zkhip.plonk with a lookup, straight-line, on int tables (t: plonk_model.circuit_ints / widegate_model.circuit_ints;
    lk, idx: lookup_ints).  vk_commitments [5 + 4 or 9 + 4, 18] and commitments [3, 18] are words as given; commitment_of(name, table ints)
    -> [18] words for name in ("v", "m", "hf", "ht").  check=False: the prover does not check its rows against the table.
    -> dict of ints: every challenge, the rounds, the claimed values and the finals of the three batch instances
    """
    label, g_names, bt_names, gate_run = KINDS[gate]
    N = 1 << mu
    w, ss, tt = [t["a"], t["b"], t["c"]], [t["s0"], t["s1"], t["s2"]], [lk["t0"], lk["t1"], lk["t2"]]
    tr = fm.Model(label)
    tr.absorb_u64(mu).absorb_u64(l).absorb(fm.words_bytes(vk_commitments)).absorb_fr(t["pi"])
    alpha, beta = tr.absorb(fm.words_bytes(commitments)).challenges(2)
    m = multiplicities3(w, tt, lk["qk"], idx, check)                                               # 2L
    c_m = commitment_of("m", m)
    zeta, beta_l = tr.absorb(fm.words_bytes(c_m)).challenges(2)
    n, d, _P, _Q, h = pm.terms(w, ss, alpha, beta)
    tree = wm.tree_of(h)
    v_comm = commitment_of("v", tree)
    gamma = tr.absorb(fm.words_bytes(v_comm)).challenge()
    lt = tables(w, tt, lk["qk"], m, zeta, beta_l, 1, [0] * mu)                                     # 3L
    c_hf, c_ht = commitment_of("hf", lt["hf"]), commitment_of("ht", lt["ht"])
    gamma_l, lam = tr.absorb(fm.words_bytes(np.stack([c_hf, c_ht]))).challenges(2)
    tau_p = tr.challenges(mu)
    tabs = wm.views(tree)
    tabs.update(eq=zm.eq_table(tau_p), n0=n[0], n1=n[1], n2=n[2], d0=d[0], d1=d[1], d2=d[2])
    p_rounds, _last, r_p = fm._stepwise(tr, tabs, lambda cur, ch: pm.sumcheck_perm3(cur, gamma, ch)[0])
    tau_g = tr.challenges(mu)
    gt = {k: t[k] for k in g_names}
    gt.update({"eq": zm.eq_table(tau_g), "in": pm.in_table(t["pi"], N)})
    g_rounds, g_at, r_g = fm._stepwise(tr, gt, gate_run)
    tau_l = tr.challenges(mu)                                                                      # 5L
    lt["E"] = [lam * e % R for e in zm.eq_table(tau_l)]
    l_rounds, l_at, r_l = fm._stepwise(tr, lt, lambda cur, ch: sumcheck_lookup_sel(cur, gamma_l, ch)[0])
    g_values = [g_at[k] for k in g_names]
    p_values = [bm.evaluate(x, r_p) for x in w + ss]
    v_values = [bm.evaluate(tree, z) for z in wm.v_points(r_p)]
    src = dict(lk, a=t["a"], b=t["b"], c=t["c"], m=lt["m"], hf=lt["hf"], ht=lt["ht"])
    l_values = [bm.evaluate(src[k], r_l) for k in L_VALUES]
    assert [l_values[L_VALUES.index(k)] for k in ("qk", "m", "hf", "ht")] == [l_at[k] for k in ("qk", "m", "hf", "ht")]
    b_alpha = tr.absorb_fr(g_values).absorb_fr(p_values).absorb_fr(v_values).absorb_fr(l_values).challenge()
    ns = len(g_names) - 3
    claims = [(bt_names.index(k), r_g, v) for k, v in zip(g_names, g_values)] + [(ns + i, r_p, v) for i, v in enumerate(p_values)]
    claims += [(ns + i, r_l, l_values[i]) for i in range(3)]
    b_rounds, rho_mu, finals = fm.batch_prove(tr, [t[k] for k in bt_names], claims, b_alpha)
    v_rounds, rho_mu1, v_finals = fm.batch_prove(tr, [tree], [(0, z, v) for z, v in zip(wm.v_points(r_p), v_values)], b_alpha)
    lb_rounds, rho_l, l_finals = fm.batch_prove(tr, [src[k] for k in L_BATCH_TABLES], [(j, r_l, l_values[3 + j]) for j in range(7)], b_alpha)
    return {"mu": mu, "l": l, "gate": gate, "alpha": alpha, "beta": beta, "gamma": gamma, "tau_p": tau_p, "r_p": r_p, "tau_g": tau_g, "r_g": r_g,
            "p_rounds": p_rounds, "g_rounds": g_rounds, "g_values": g_values, "p_values": p_values, "v_values": v_values, "v_commitment": v_comm,
            "b_alpha": b_alpha, "b_rounds": b_rounds, "rho_mu": rho_mu, "finals": finals, "v_rounds": v_rounds, "rho_mu1": rho_mu1,
            "v_finals": v_finals, "tree": tree,
            "zeta": zeta, "beta_l": beta_l, "gamma_l": gamma_l, "lambda": lam, "tau_l": tau_l, "r_l": r_l, "rho_l": rho_l, "m": m,
            "l_commitments": np.stack([c_m, c_hf, c_ht]), "l_rounds": l_rounds, "l_values": l_values, "lb_rounds": lb_rounds, "l_finals": l_finals}


def record(m, commitments):
    """the model's run in the product's record layout (zero opening proofs)"""
    mu = m["mu"]
    rec = pm.record(m, commitments)
    if m["gate"] is not None:
        rec["gate"] = m["gate"]
    rec["lookup"] = {"commitments": np.asarray(m["l_commitments"], dtype=np.uint64).reshape(3, 18), "rounds": np.stack([zm.mont(p) for p in m["l_rounds"]]),
                     "values": zm.mont(m["l_values"]), "batch": fm._batch_record(m["lb_rounds"], mu)}
    return rec


def fake_commitment(name, table):
    return lm.fake_commitment(name, table)


def model_record(mu, seed, gate=None, check=True, commitment_of=fake_commitment, **kw):
    """sample_circuit_lookup(mu, seed, gate, **kw) proved by the model on stand-in commitments
    -> (vk, public inputs, record, finals, v_finals, l_finals, the model's run)"""
    from zkhip import plonk

    c = plonk.sample_circuit_lookup(mu, seed, gate=gate, **kw)
    t = (wg if gate == "wide" else pm).circuit_ints(c)
    lk, idx = lookup_ints(c)
    n_vk = (9 if gate == "wide" else 5) + 4
    vk_comms, comms = wg.words(n_vk, 1000 + seed), wg.words(3, 2000 + seed)
    m = prove(t, lk, idx, mu, c["l"], vk_comms, comms, commitment_of, gate=gate, check=check)
    vk = {"mu": mu, "l": c["l"], "commitments": vk_comms, "pcs": None, "lookup": True}
    if gate is not None:
        vk["gate"] = gate
    return vk, c["public_inputs"], record(m, comms), zm.mont(m["finals"]), zm.mont(m["v_finals"]), zm.mont(m["l_finals"]), m


def parent_digest(rec) -> str:
    """zkhip.plonk.proof_digest as it stood before the lookup, restated: SHA-256 over mu, l and the parts of a record WITHOUT a lookup in
    the order of the schedule"""
    h = hashlib.sha256()
    put = lambda part: h.update(np.ascontiguousarray(part, dtype="<u8").tobytes())
    h.update(int(rec["mu"]).to_bytes(8, "little") + int(rec["l"]).to_bytes(8, "little"))
    for k in pm.FIELD_PARTS:
        put(rec[k])
    for b in ("batch", "v_batch"):
        put(rec[b]["rounds"]), put(rec[b]["opening"])
    return h.hexdigest()
