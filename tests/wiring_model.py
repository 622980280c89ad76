"""
Big-int statement of the wiring PermCheck (a helper of test_wiring.py / test_gpu_wiring.py, not a test), written from the formulas

    num = w + alpha sid + beta,  den = w + alpha ssigma + beta,  h = num / den         (python Fractions reduced mod r)
    tree[0..N) = h,  tree[i] = tree[a] tree[b] with (a, b) = sub_index(i) for N <= i < 2N - 1,  tree[2N-1] = 0
    v(0,x) = tree[x],  v(1,x) = tree[N + x],  v(x,0) = tree[2x],  v(x,1) = tree[2x + 1]    (index bit 0 = the TOP bit)
    F(x)   = eq(x) [ v(1,x) - v(x,0) v(x,1) + gamma ( den(x) h(x) - num(x) ) ]
    p_i(t) = sum_j F((1 - t) lo_j + t hi_j),  t = 0 .. 3 (and 4, for the degree check), then every table is folded with chal[i]

-- not from the product code.  Values are canonical python ints mod r.
"""
import random
from fractions import Fraction

import numpy as np
import pyoracle as po
from zerocheck_model import eq_point, eq_table, ints, mont  # noqa: F401  (re-exported for the tests)

R = po.R_MOD
TABLES = ("eq", "v1x", "vx0", "vx1", "h", "num", "den")


def sub_index(i):
    """the children of inner node i: clear its top set bit, shift left (dacc_product.rs:18-23, restated)"""
    top = 1
    while top * 2 <= i:
        top *= 2
    x = (i - top) * 2
    return x, x + 1


def fractions(w, sid, ssigma, alpha, beta):
    """-> (num, den, h) as lists of ints; h through an exact Fraction, then numerator * denominator^-1 mod r"""
    num = [(a + alpha * b + beta) % R for a, b in zip(w, sid)]
    den = [(a + alpha * b + beta) % R for a, b in zip(w, ssigma)]
    h = []
    for n, d in zip(num, den):
        f = Fraction(n, d)  # ZeroDivisionError on a zero denominator
        h.append(f.numerator * pow(f.denominator, -1, R) % R)
    return num, den, h


def tree_of(h):
    N = len(h)
    tree = list(h) + [0] * N
    for i in range(N, 2 * N - 1):
        a, b = sub_index(i)
        tree[i] = tree[a] * tree[b] % R
    return tree


def views(tree):
    """-> dict v1x, vx0, vx1, h of N ints each"""
    N = len(tree) // 2
    return {"h": [tree[x] for x in range(N)], "v1x": [tree[N + x] for x in range(N)], "vx0": [tree[2 * x] for x in range(N)],
            "vx1": [tree[2 * x + 1] for x in range(N)]}


def F(eq, v1x, vx0, vx1, h, num, den, gamma):
    return eq * (v1x - vx0 * vx1 + gamma * (den * h - num)) % R


def tables(w, sid, ssigma, alpha, beta, tau):
    """the seven tables of the sumcheck and the tree"""
    num, den, h = fractions(w, sid, ssigma, alpha, beta)
    tree = tree_of(h)
    t = views(tree)
    t.update(eq=eq_table(tau), num=num, den=den)
    return t, tree


def sumcheck_wiring(tabs, gamma, chal, evals=4):
    """tabs: dict name -> list of 2^mu ints.  -> (rounds: mu x [p(0) .. p(evals-1)], last: the seven remaining values in TABLES order)"""
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


def interpolate4(evals, x):
    """Lagrange on the nodes 0 .. 3"""
    acc = 0
    for k in range(4):
        num, den = 1, 1
        for m in range(4):
            if m != k:
                num = num * (x - m) % R
                den = den * (k - m) % R
        acc += evals[k] * num * pow(den, -1, R)
    return acc % R


def v_points(r):
    """the five (mu + 1)-points at which the tree is opened: (0,r), (1,r), (r,0), (r,1), (1,..,1,0)"""
    r = list(r)
    return [[0] + r, [1] + r, r + [0], r + [1], [1] * len(r) + [0]]


def verify_rounds(rounds, opened, v_opened, alpha, beta, gamma, tau, chal):
    """opened: dict w, sid, ssigma -> value at chal; v_opened: the tree at v_points(chal).  -> the list of failed checks 1 .. 3"""
    bad, target = [], 0
    for p, r in zip(rounds, chal):
        if (p[0] + p[1]) % R != target:
            return [1]
        target = interpolate4(p[:4], r)
    num = (opened["w"] + alpha * opened["sid"] + beta) % R
    den = (opened["w"] + alpha * opened["ssigma"] + beta) % R
    v0r, v1r, vr0, vr1, prod = v_opened
    if target != F(eq_point(tau, chal), v1r, vr0, vr1, v0r, num, den, gamma):
        bad.append(2)
    if prod != 1:
        bad.append(3)
    return bad


def shuffled_circuit(mu, seed, break_wire=None):
    """w, sid, ssigma of 2^mu ints: sigma a random permutation without fixed points (random.shuffle, repeated), w constant on its cycles, sid[i] = i"""
    n = 1 << mu
    rnd = random.Random(seed)
    sigma = list(range(n))
    while any(sigma[i] == i for i in range(n)):  # no fixed point: a fixed slot constrains nothing, so breaking it would change nothing
        rnd.shuffle(sigma)
    rng = po.SplitMix64(seed + 17)
    w = [None] * n
    for i in range(n):
        if w[i] is None:
            val, j = rng.fr(), i
            while w[j] is None:
                w[j] = val
                j = sigma[j]
    if break_wire is not None:
        w[break_wire] = (w[break_wire] + 1) % R
    return w, list(range(n)), sigma
