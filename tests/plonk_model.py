"""
Big-int statement of the three-column wiring identity and of the one-circuit HyperPlonk schedule (a helper of test_plonk.py /
test_gpu_plonk.py, not a test), written from the formulas

    n_j = w_j + alpha (j N + x) + beta,  d_j = w_j + alpha ssigma_j + beta,  h = n_0 n_1 n_2 / (d_0 d_1 d_2)   (exact Fractions mod r)
    tree = wiring_model.tree_of(h) and its four views
    F(x)   = eq(x) [ v(1,x) - v(x,0) v(x,1) + gamma ( h(x) d_0 d_1 d_2 - n_0 n_1 n_2 ) ]
    p_i(t) = sum_j F((1 - t) lo_j + t hi_j),  t = 0 .. 5 (and 6, for the degree check), then every table is folded with chal[i]

on top of wiring_model / zerocheck_model / batch_open_model / fs_model -- not from the product code.  Values are canonical python ints.
"""
from fractions import Fraction

import numpy as np

import batch_open_model as bm
import fs_model as fm
import pyoracle as po
import wiring_model as wm
import zerocheck_model as zm

R = po.R_MOD
TABLES = ("eq", "v1x", "vx0", "vx1", "h", "n0", "n1", "n2", "d0", "d1", "d2")
G_VALUES = ("q1", "q2", "a", "b", "c")
BATCH_TABLES = ("q1", "q2", "a", "b", "c", "s0", "s1", "s2")


def terms(w, ssigma, alpha, beta):
    """w, ssigma: three columns of N ints -> (n [3][N], d [3][N], P, Q, h)"""
    N = len(w[0])
    n = [[(w[j][x] + alpha * (j * N + x) + beta) % R for x in range(N)] for j in range(3)]
    d = [[(w[j][x] + alpha * ssigma[j][x] + beta) % R for x in range(N)] for j in range(3)]
    P = [n[0][x] * n[1][x] * n[2][x] % R for x in range(N)]
    Q = [d[0][x] * d[1][x] * d[2][x] % R for x in range(N)]
    h = []
    for p, q in zip(P, Q):
        f = Fraction(p, q)  # ZeroDivisionError on a zero denominator
        h.append(f.numerator * pow(f.denominator, -1, R) % R)
    return n, d, P, Q, h


def F(eq, v1x, vx0, vx1, h, n0, n1, n2, d0, d1, d2, gamma):
    return eq * (v1x - vx0 * vx1 + gamma * (h * d0 * d1 * d2 - n0 * n1 * n2)) % R


def tables(w, ssigma, alpha, beta, tau):
    """the eleven tables of the sumcheck and the tree"""
    n, d, _P, _Q, h = terms(w, ssigma, alpha, beta)
    tree = wm.tree_of(h)
    t = wm.views(tree)
    t.update(eq=zm.eq_table(tau), n0=n[0], n1=n[1], n2=n[2], d0=d[0], d1=d[1], d2=d[2])
    return t, tree


def sumcheck_perm3(tabs, gamma, chal, evals=6):
    """tabs: dict name -> list of 2^mu ints.  -> (rounds: mu x [p(0) .. p(evals-1)], last: the eleven remaining values in TABLES order)"""
    cur = {k: list(tabs[k]) for k in TABLES}
    mu = len(cur["eq"]).bit_length() - 1
    rounds = []
    for i in range(mu):
        half = len(cur["eq"]) // 2
        ev = []
        for t in range(evals):
            s = 0
            for j in range(half):
                s += F(*[((1 - t) * cur[k][j] + t * cur[k][j + half]) % R for k in TABLES], gamma)
            ev.append(s % R)
        rounds.append(ev)
        r = chal[i]
        cur = {k: [((1 - r) * v[j] + r * v[j + half]) % R for j in range(half)] for k, v in cur.items()}
    return rounds, [cur[k][0] for k in TABLES]


def interpolate(evals, x):
    """Lagrange on the nodes 0 .. len(evals) - 1"""
    acc, n = 0, len(evals)
    for k in range(n):
        num, den = 1, 1
        for m in range(n):
            if m != k:
                num = num * (x - m) % R
                den = den * (k - m) % R
        acc += evals[k] * num * pow(den, -1, R)
    return acc % R


def random_columns(mu, seed):
    """three wire columns and three columns of slot numbers of a random permutation of the 3N slots (for the kernel tests: the identity
    holds for ANY tables, satisfied or not)"""
    import random

    N = 1 << mu
    rng = po.SplitMix64(seed)
    sigma = list(range(3 * N))
    random.Random(seed).shuffle(sigma)
    return [rng.fr_vec(N) for _ in range(3)], [sigma[j * N:(j + 1) * N] for j in range(3)]


def in_table(public_inputs, N):
    return list(public_inputs) + [0] * (N - len(public_inputs))


def circuit_ints(c):
    """a circuit of zkhip.plonk.sample_circuit -> dict of int tables: q1, q2, a, b, c, s0, s1, s2, pi"""
    N = 1 << c["mu"]
    t = {k: zm.ints(c[k]) for k in ("q1", "q2", "a", "b", "c")}
    sg = [int(x) for x in c["sigma"]]
    t.update(s0=sg[:N], s1=sg[N:2 * N], s2=sg[2 * N:], pi=zm.ints(c["public_inputs"]))
    return t


def prove(t, mu, l, vk_commitments, commitments, v_commitment_of, label=b"plonk"):
    """
    The schedule of zkhip.plonk on int tables (t: circuit_ints).  Commitments cannot be modelled (no curve arithmetic): vk_commitments
    [5, 18] and commitments [3, 18] are words as given; v_commitment_of(tree ints) -> [18] words.
    -> dict of ints: every challenge, the rounds, the claimed values and the finals of the two batch instances
    """
    N = 1 << mu
    tr = fm.Model(label)
    tr.absorb_u64(mu).absorb_u64(l).absorb(fm.words_bytes(vk_commitments)).absorb_fr(t["pi"])
    alpha, beta = tr.absorb(fm.words_bytes(commitments)).challenges(2)
    w, ss = [t["a"], t["b"], t["c"]], [t["s0"], t["s1"], t["s2"]]
    n, d, _P, _Q, h = terms(w, ss, alpha, beta)
    tree = wm.tree_of(h)
    v_comm = v_commitment_of(tree)
    gamma = tr.absorb(fm.words_bytes(v_comm)).challenge()
    tau_p = tr.challenges(mu)
    tabs = wm.views(tree)
    tabs.update(eq=zm.eq_table(tau_p), n0=n[0], n1=n[1], n2=n[2], d0=d[0], d1=d[1], d2=d[2])
    p_rounds, _last, r_p = fm._stepwise(tr, tabs, lambda cur, ch: sumcheck_perm3(cur, gamma, ch)[0])
    tau_g = tr.challenges(mu)
    gt = {k: t[k] for k in G_VALUES}
    gt.update({"eq": zm.eq_table(tau_g), "in": in_table(t["pi"], N)})
    g_rounds, g_at, r_g = fm._stepwise(tr, gt, lambda cur, ch: zm.sumcheck_gate(cur, ch)[0])
    g_values = [g_at[k] for k in G_VALUES]
    p_values = [bm.evaluate(x, r_p) for x in w + ss]
    v_values = [bm.evaluate(tree, z) for z in wm.v_points(r_p)]
    b_alpha = tr.absorb_fr(g_values).absorb_fr(p_values).absorb_fr(v_values).challenge()
    claims = [(BATCH_TABLES.index(k), r_g, v) for k, v in zip(G_VALUES, g_values)] + [(2 + i, r_p, v) for i, v in enumerate(p_values)]
    b_rounds, rho_mu, finals = fm.batch_prove(tr, [t[k] for k in BATCH_TABLES], claims, b_alpha)
    v_rounds, rho_mu1, v_finals = fm.batch_prove(tr, [tree], [(0, z, v) for z, v in zip(wm.v_points(r_p), v_values)], b_alpha)
    return {"mu": mu, "l": l, "alpha": alpha, "beta": beta, "gamma": gamma, "tau_p": tau_p, "r_p": r_p, "tau_g": tau_g, "r_g": r_g, "p_rounds": p_rounds,
            "g_rounds": g_rounds, "g_values": g_values, "p_values": p_values, "v_values": v_values, "v_commitment": v_comm, "b_alpha": b_alpha,
            "b_rounds": b_rounds, "rho_mu": rho_mu, "finals": finals, "v_rounds": v_rounds, "rho_mu1": rho_mu1, "v_finals": v_finals, "tree": tree}


def record(m, commitments):
    """the model's run in the product's record layout (zero opening proofs)"""
    mu = m["mu"]
    st = lambda rounds: np.stack([zm.mont(p) for p in rounds])
    return {"mu": mu, "l": m["l"], "commitments": np.asarray(commitments, dtype=np.uint64).reshape(3, 18),
            "v_commitment": np.asarray(m["v_commitment"], dtype=np.uint64).reshape(18), "p_rounds": st(m["p_rounds"]), "g_rounds": st(m["g_rounds"]),
            "g_values": zm.mont(m["g_values"]), "p_values": zm.mont(m["p_values"]), "v_values": zm.mont(m["v_values"]),
            "batch": {"rounds": st(m["b_rounds"]), "opening": np.zeros((mu, 18), dtype=np.uint64)},
            "v_batch": {"rounds": st(m["v_rounds"]), "opening": np.zeros((mu + 1, 18), dtype=np.uint64)}}


FIELD_PARTS = ("commitments", "v_commitment", "p_rounds", "g_rounds", "g_values", "p_values", "v_values")


def field_digest(rec) -> str:
    """SHA-256 over the parts of a record the model can state: everything but the opening proofs"""
    import hashlib

    h = hashlib.sha256()
    put = lambda part: h.update(np.ascontiguousarray(part, dtype="<u8").tobytes())
    h.update(int(rec["mu"]).to_bytes(8, "little") + int(rec["l"]).to_bytes(8, "little"))
    for k in FIELD_PARTS:
        put(rec[k])
    put(rec["batch"]["rounds"]), put(rec["v_batch"]["rounds"])
    return h.hexdigest()
