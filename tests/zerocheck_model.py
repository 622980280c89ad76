"""
Big-int statement of the gate ZeroCheck (a helper of test_zerocheck.py / test_gpu_zerocheck.py, not a test): the eq table, the
gate sumcheck's five evaluations per round and the verifier's field checks, written from the formulas

    eq(tau, x) = prod_i (x_i ? tau_i : 1 - tau_i),   x_0 = the TOP index bit
    G(x)       = eq(x) [ q1(x) (a(x) + b(x)) + q2(x) a(x) b(x) - c(x) + in(x) ]
    p_i(t)     = sum_j G((1 - t) lo_j + t hi_j),      t = 0 .. 4,   then every table is folded with challenge[i]

-- not from the product code.  Values are canonical python ints mod r.
"""
import numpy as np
import pyoracle as po

R = po.R_MOD
TABLES = ("eq", "q1", "q2", "a", "b", "c", "in")


def eq_table(tau):
    """n-factor product per element (the product code builds it by doubling)"""
    n = len(tau)
    out = []
    for x in range(1 << n):
        v = 1
        for i in range(n):
            bit = (x >> (n - 1 - i)) & 1
            v = v * (tau[i] if bit else (1 - tau[i])) % R
        out.append(v)
    return out


def gate(eq, q1, q2, a, b, c, inp):
    return eq * (q1 * (a + b) + q2 * a * b - c + inp) % R


def sumcheck_gate(tabs, chal):
    """tabs: dict name -> list of 2^n ints.  -> (rounds: n x [p(0) .. p(4)], last: the seven remaining values in TABLES order)"""
    cur = {k: list(tabs[k]) for k in TABLES}
    n = len(cur["eq"]).bit_length() - 1
    rounds = []
    for i in range(n):
        h = len(cur["eq"]) // 2
        evals = []
        for t in range(5):
            s = 0
            for j in range(h):
                s += gate(*[((1 - t) * cur[k][j] + t * cur[k][j + h]) % R for k in TABLES])
            evals.append(s % R)
        rounds.append(evals)
        r = chal[i]
        cur = {k: [((1 - r) * v[j] + r * v[j + h]) % R for j in range(h)] for k, v in cur.items()}
    return rounds, [cur[k][0] for k in TABLES]


def interpolate5(evals, x):
    """Lagrange on the nodes 0 .. 4"""
    acc = 0
    for k in range(5):
        num, den = 1, 1
        for m in range(5):
            if m != k:
                num = num * (x - m) % R
                den = den * (k - m) % R
        acc += evals[k] * num * pow(den, -1, R)
    return acc % R


def eq_point(tau, r):
    v = 1
    for t, x in zip(tau, r):
        v = v * (t * x + (1 - t) * (1 - x)) % R
    return v


def verify_rounds(rounds, opened, tau, chal):
    """opened: dict a, b, c, in, q1, q2 -> value at chal.  Steps 1-3 of the verifier."""
    target = 0
    for p, r in zip(rounds, chal):
        if (p[0] + p[1]) % R != target:
            return False
        target = interpolate5(p, r)
    return target == gate(eq_point(tau, chal), opened["q1"], opened["q2"], opened["a"], opened["b"], opened["c"], opened["in"])


def circuit(n, seed, satisfied=True, break_gate=None):
    """random tables of 2^n ints; satisfied: c = q1 (a + b) + q2 a b + in"""
    rng = po.SplitMix64(seed)
    m = 1 << n
    t = {k: rng.fr_vec(m) for k in ("q1", "q2", "a", "b", "c", "in")}
    if satisfied:
        t["c"] = [(q1 * (a + b) + q2 * a * b + i) % R for q1, q2, a, b, i in zip(t["q1"], t["q2"], t["a"], t["b"], t["in"])]
    if break_gate is not None:
        t["c"][break_gate] = (t["c"][break_gate] + 1) % R
    return t


def mont(xs):
    """ints -> [len, 4] Montgomery limbs"""
    return np.array([po.fr_to_mont_limbs(x % R) for x in xs], dtype=np.uint64).reshape(-1, 4)


def ints(a):
    return [po.fr_from_mont_limbs(x) for x in np.asarray(a, dtype=np.uint64).reshape(-1, 4)]
