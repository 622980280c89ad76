"""
Big-int statement of the lookup argument (a helper of test_lookup.py / test_gpu_lookup.py, not a test), written from the definition

    df = beta + f,  dt = beta + t,  hf = 1 / df,  ht = m / dt,  m[y] = #{x : idx[x] = y}
    L(x) = hf(x) - ht(x) + E(x) [ hf(x) df(x) - 1 + gamma ( ht(x) dt(x) - m(x) ) ],     E = lambda eq(tau, .),     sum_x L(x) = 0

on top of zerocheck_model / batch_open_model / fs_model -- not from the product code.  Values are canonical python ints mod r.
Commitments cannot be modelled here (no curve arithmetic): the schedule takes them as given words.
"""
import numpy as np

import batch_open_model as bm
import fs_model as fm
import pyoracle as po
from zerocheck_model import eq_point, eq_table, ints, mont  # noqa: F401  (re-exported for the tests)

R = po.R_MOD
TABLES = ("E", "df", "dt", "m", "hf", "ht")
OPENED = ("f", "t", "m", "hf", "ht")


def L(E, df, dt, m, hf, ht, gamma):
    return (hf - ht + E * (hf * df - 1 + gamma * (ht * dt - m))) % R


def multiplicities(idx, N):
    m = [0] * N
    for y in idx:
        m[y] += 1
    return m


def tables(f, t, m, beta, lam, tau, hf=None, ht=None):
    """the six tables of the sumcheck (hf / ht: the prover's, when a test wants wrong ones)"""
    df, dt = [(beta + x) % R for x in f], [(beta + x) % R for x in t]
    hf = hf if hf is not None else [pow(d, -1, R) for d in df]
    ht = ht if ht is not None else [mm * pow(d, -1, R) % R for mm, d in zip(m, dt)]
    return {"E": [lam * e % R for e in eq_table(tau)], "df": df, "dt": dt, "m": [x % R for x in m], "hf": hf, "ht": ht}


def sumcheck_lookup(tabs, gamma, chal, evals=4):
    """tabs: dict name -> list of 2^n ints.  -> (rounds: n x [p(0) .. p(3)], last: the six remaining values in TABLES order)"""
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


def chain(rounds, chal):
    """the round chain from 0 -> (holds, the value it ends in)"""
    target = 0
    for p, r in zip(rounds, chal):
        if (p[0] + p[1]) % R != target:
            return False, None
        target = interpolate4(p, r)
    return True, target


def prove(f, t, idx, commitment_t, commitments_of, label=b"lookup", m=None, hf_of=None):
    """the schedule of zkhip.lookup on the model transcript.  commitments_of(name, table ints) -> [18] words (the caller's commitments:
    m, hf, ht depend on idx and beta).  m / hf_of(hf ints) -> hf: a wrong prover's tables.  -> dict of ints and words"""
    N = len(f)
    n = N.bit_length() - 1
    m = multiplicities(idx, N) if m is None else m
    tr = fm.Model(label)
    tr.absorb_u64(n).absorb(fm.words_bytes(commitment_t))
    c_f, c_m = commitments_of("f", f), commitments_of("m", m)
    beta = tr.absorb(fm.words_bytes(np.stack([c_f, c_m]))).challenge()
    tabs = tables(f, t, m, beta, 1, [0] * n)
    hf, ht = tabs["hf"], tabs["ht"]
    if hf_of is not None:
        hf = hf_of(hf)
    c_hf, c_ht = commitments_of("hf", hf), commitments_of("ht", ht)
    gamma, lam = tr.absorb(fm.words_bytes(np.stack([c_hf, c_ht]))).challenges(2)
    tau = tr.challenges(n)
    tabs = tables(f, t, m, beta, lam, tau, hf, ht)
    rounds, last, chal = fm._stepwise(tr, tabs, lambda cur, ch: sumcheck_lookup(cur, gamma, ch)[0])
    values = [(last["df"] - beta) % R, (last["dt"] - beta) % R, last["m"], last["hf"], last["ht"]]
    b_alpha = tr.absorb_fr(values).challenge()
    src = [f, t, m, hf, ht]
    b_rounds, rho, finals = fm.batch_prove(tr, src, [(j, chal, values[j]) for j in range(5)], b_alpha)
    return {"n": n, "beta": beta, "gamma": gamma, "lambda": lam, "tau": tau, "rounds": rounds, "chal": chal, "values": values, "b_alpha": b_alpha,
            "b_rounds": b_rounds, "rho": rho, "finals": finals, "commitments": np.stack([c_f, c_m, c_hf, c_ht]), "state": tr.state}


def model_record(mo):
    """the model's run in the product's record layout (zero opening proof)"""
    return {"n": mo["n"], "commitments": np.asarray(mo["commitments"], dtype=np.uint64).reshape(4, 18), "rounds": np.stack([mont(p) for p in mo["rounds"]]),
            "values": mont(mo["values"]), "batch": fm._batch_record(mo["b_rounds"], mo["n"])}


def field_digest(rec) -> str:
    """SHA-256 over the parts of a record the model can state: everything but the opening proof"""
    import hashlib

    h = hashlib.sha256()
    put = lambda part: h.update(np.ascontiguousarray(part, dtype="<u8").tobytes())
    h.update(int(rec["n"]).to_bytes(8, "little"))
    put(rec["commitments"]), put(rec["rounds"]), put(rec["values"]), put(rec["batch"]["rounds"])
    return h.hexdigest()


def fake_commitment(name, table):
    """18 words that depend on the table: stands for a commitment where no curve arithmetic is at hand"""
    import hashlib

    d = hashlib.sha256(name.encode() + b"".join(int(x % R).to_bytes(32, "little") for x in table)).digest()
    return np.frombuffer((d * 5)[:144], dtype="<u8").astype(np.uint64)
