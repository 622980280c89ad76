"""
Big-int statement of the batch opening (a helper of test_batch_open.py / test_gpu_batch_open.py, not a test), written from the
formulas

    a_k    = alpha^k
    E_j(x) = sum_{k : j_k = j} a_k eq(z_k, x),          x_0 = the TOP index bit
    S      = sum_k a_k v_k = sum_x sum_j E_j(x) f_j(x)
    p_i(t) = sum_j sum_x E_j((1 - t) lo + t hi) f_j((1 - t) lo + t hi),   t = 0, 1, 2,  then every table is folded with rho[i]
    e_j    = E_j(rho),   g = sum_j e_j f_j,   g(rho) = p_{n-1}(rho_{n-1})

-- not from the product code.  Values are canonical python ints mod r.  Claims are (j, z, v) with z a list of n ints.
"""
import pyoracle as po
from zerocheck_model import eq_point, eq_table, ints, mont  # noqa: F401  (re-exported for the tests)

R = po.R_MOD


def weights(alpha, count):
    return [pow(alpha, k, R) for k in range(count)]


def evaluate(table, z):
    """f(z) of a multilinear table: sum_x eq(z, x) f(x)"""
    return sum(e * f for e, f in zip(eq_table(z), table)) % R


def combined_eq_tables(n_tables, n, claims, alpha):
    out = [[0] * (1 << n) for _ in range(n_tables)]
    for a, (j, z, _) in zip(weights(alpha, len(claims)), claims):
        out[j] = [(o + a * e) % R for o, e in zip(out[j], eq_table(z))]
    return out


def claimed_sum(claims, alpha):
    return sum(a * v for a, (_, _, v) in zip(weights(alpha, len(claims)), claims)) % R


def fold(tab, r):
    h = len(tab) // 2
    return [((1 - r) * tab[i] + r * tab[i + h]) % R for i in range(h)]


def sumcheck_multi(es, fs, rho):
    """-> (rounds: n x [t0, t1, t2], last_e, last_f)"""
    es, fs = [list(e) for e in es], [list(f) for f in fs]
    n = len(es[0]).bit_length() - 1
    rounds = []
    for i in range(n):
        h = len(es[0]) // 2
        tr = []
        for t in range(3):
            s = 0
            for e, f in zip(es, fs):
                for x in range(h):
                    s += (((1 - t) * e[x] + t * e[x + h]) % R) * (((1 - t) * f[x] + t * f[x + h]) % R)
            tr.append(s % R)
        rounds.append(tr)
        es, fs = [fold(e, rho[i]) for e in es], [fold(f, rho[i]) for f in fs]
    return rounds, [e[0] for e in es], [f[0] for f in fs]


def eq_coefficients(n_tables, claims, alpha, rho):
    e = [0] * n_tables
    for a, (j, z, _) in zip(weights(alpha, len(claims)), claims):
        e[j] = (e[j] + a * eq_point(z, rho)) % R
    return e


def lincomb(coeffs, tabs):
    return [sum(c * t[x] for c, t in zip(coeffs, tabs)) % R for x in range(len(tabs[0]))]


def mixed_points(n, count, rng):
    """random, repeated and boolean points in turn; the last boolean one is (1,..,1,0)"""
    pts = []
    for k in range(count):
        if k % 3 == 0:
            pts.append(rng.fr_vec(n))
        elif k % 3 == 1:
            pts.append(list(pts[-1]))
        elif k == count - 1 or k == 2:
            pts.append([1] * (n - 1) + [0])
        else:
            pts.append([(k + i) & 1 for i in range(n)])
    return pts


def instance(n, n_tables, n_claims, seed):
    """-> (tables, claims with honest values, alpha, rho)"""
    rng = po.SplitMix64(seed)
    tables = [rng.fr_vec(1 << n) for _ in range(n_tables)]
    claims = [(k % n_tables, z, evaluate(tables[k % n_tables], z)) for k, z in enumerate(mixed_points(n, n_claims, rng))]
    return tables, claims, rng.fr(), rng.fr_vec(n)


def prove(tables, claims, alpha, rho):
    """-> (record as the product's: rounds [n, 3, 4] Montgomery limbs + a zero opening, finals f_j(rho))"""
    import numpy as np

    n = len(rho)
    es = combined_eq_tables(len(tables), n, claims, alpha)
    rounds, _le, lf = sumcheck_multi(es, tables, rho)
    rec = {"rounds": np.stack([mont(tr) for tr in rounds]), "opening": np.zeros((n, 18), dtype=np.uint64)}
    return rec, lf


def claims_mont(claims):
    return [(j, mont(z), mont([v])[0]) for j, z, v in claims]
