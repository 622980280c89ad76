"""
The witness rules WITH a lookup (zkhip.plonk module text, WITNESS; include/zkhip.h) in pure Python ints, on top of witness_model.py: the
function rule of the table, the two kinds of computing rows, sources, levels and launches, evaluation (c = 0 on a miss) and the check with
its six numbers.  Written from the rules, not from the sampler: test_witness_lookup.py holds it against sample_circuit_lookup_fn.

A circuit is the dict of zkhip.plonk with "lookup": {"qk", "t0", "t1", "t2"}; values are canonical ints, as in witness_model.py.
"""
import numpy as np

import witness_model as wm

GATE, LOOKUP = 1, 2  # the kind of a computing row (0: it computes nothing)


def table(circuit: dict) -> dict:
    """-> {"qk": N ints, "t": N triples, "first": pair -> the smallest entry with that pair}.  ValueError: a qk entry that is neither 0 nor
    1 ("K of N entries of qk ..." and the smallest such row), or a table that is no function of its first two columns ("K of N table
    entries repeat the pair (t0, t1) of an earlier entry with another t2" -- K counts the entries whose t2 differs from the t2 of the FIRST
    entry of their pair -- and the smallest of them)"""
    lk = circuit["lookup"]
    qk = wm.ints(lk["qk"])
    N = len(qk)
    bad = [x for x in range(N) if qk[x] not in (0, 1)]
    if bad:
        raise ValueError(f"{len(bad)} of {N} entries of qk are neither 0 nor 1; the first is row {bad[0]}")
    t = list(zip(wm.ints(lk["t0"]), wm.ints(lk["t1"]), wm.ints(lk["t2"])))
    first = {}
    for y in range(N):
        first.setdefault(t[y][:2], y)
    bad = [y for y in range(N) if t[y][2] != t[first[t[y][:2]]][2]]
    if bad:
        raise ValueError(f"{len(bad)} of {N} table entries repeat the pair (t0, t1) of an earlier entry with another t2; the first is entry {bad[0]}")
    return {"qk": qk, "t": t, "first": first}


def kinds(circuit: dict, tab: dict) -> list:
    """per row GATE, LOOKUP or 0: gate-computing as witness_model.computing_rows says; lookup-computing when qk = 1 and not gate-computing"""
    gate = wm.computing_rows(circuit)
    return [GATE if g else (LOOKUP if q else 0) for g, q in zip(gate, tab["qk"])]


def plan(circuit: dict) -> dict:
    """witness_model.plan with both kinds of rows computing, plus "kind" (per row) and "table".  ValueError as `table` and
    witness_model.plan raise it"""
    tab = table(circuit)
    kind = kinds(circuit, tab)
    p = wm.plan(circuit["sigma"], 1 << circuit["mu"], [k != 0 for k in kind])
    p.update(kind=kind, table=tab)
    return p


launches, info = wm.launches, wm.info


def generate(circuit: dict, p: dict, public_inputs, free=None):
    """-> (a, b, c) canonical ints.  A lookup-computing row takes c = t2[y] for the smallest y with (t0, t1)[y] = (a, b), or 0"""
    N, wide, sel, inp = p["N"], circuit.get("gate") == "wide", wm.selectors(circuit), wm._in(circuit, public_inputs)
    tab = p["table"]
    w = [[0] * N for _ in range(3)]
    value = lambda s: (free[s[1]] % wm.R if free is not None else 0) if s[0] else w[2][s[1]]
    for rows in p["levels"]:
        for x in rows:
            w[0][x], w[1][x] = value(p["src"][x]), value(p["src"][N + x])
            if p["kind"][x] == LOOKUP:
                y = tab["first"].get((w[0][x], w[1][x]))
                w[2][x] = tab["t"][y][2] if y is not None else 0
            else:
                w[2][x] = wm.out_value(sel, wide, x, w[0][x], w[1][x], inp[x])
    for x in range(N):
        if p["level"][x] is None:
            for j in range(3):
                w[j][x] = value(p["src"][j * N + x])
    return w[0], w[1], w[2]


def check(circuit: dict, p: dict, a, b, c, public_inputs) -> dict:
    """witness_model.check plus the bad lookups: the rows with qk = 1 whose (a, b, c) is no table entry, of either kind"""
    out = wm.check(circuit, p, a, b, c, public_inputs)
    entries = set(p["table"]["t"])
    rows = [x for x in range(p["N"]) if p["table"]["qk"][x] and (a[x], b[x], c[x]) not in entries]
    out.update(bad_lookups=len(rows), first_bad_lookup=rows[0] if rows else None)
    return out


def find_indices(p: dict, a, b, c) -> list:
    """what zk_lookup3_find gives: per row with qk = 1 the smallest y with (t0, t1, t2)[y] = (a, b, c) (None: no entry), 0 elsewhere"""
    first = {}
    for y, e in enumerate(p["table"]["t"]):
        first.setdefault(e, y)
    return [first.get((a[x], b[x], c[x])) if q else 0 for x, q in enumerate(p["table"]["qk"])]


# ---- hand-built circuits: the wide gate, l input rows, an XOR table on k bits ----
def xor_table(N: int, k: int) -> dict:
    """entry y < 4^k is (y >> k, y & (2^k - 1), their XOR), padded to N by repeating the last one; canonical ints per column"""
    ys = [min(y, (1 << 2 * k) - 1) for y in range(N)]
    low = (1 << k) - 1
    return {"t0": [y >> k for y in ys], "t1": [y & low for y in ys], "t2": [(y >> k) ^ (y & low) for y in ys]}


def _circuit(mu: int, l: int, classes, qk, tab: dict, free) -> dict:
    """input rows 0 .. l - 1 (qO = 1), every other row with the gate switched off; -> the circuit plus "free": 3N canonical ints"""
    N = 1 << mu
    sel = {q: [0] * N for q in wm.WIDE}
    for x in range(l):
        sel["qO"][x] = 1
    c = {"gate": "wide", "mu": mu, "l": l, "sigma": wm.sigma_of(N, classes), "public_inputs": wm.limbs([3 + 5 * x for x in range(l)]), "free": free}
    c.update({q: wm.limbs(v) for q, v in sel.items()})
    c["lookup"] = dict({q: wm.limbs(v) for q, v in tab.items()}, qk=wm.limbs(qk))
    return c


def chain(mu: int = 10, l: int = 4, k: int = 4) -> dict:
    """every row x >= l is a lookup row with a = c[x - 1] (row l: free) and a free b: row x has level x - l, one row per level -- N - l
    levels next to the input rows' in ONE single-workgroup run"""
    N = 1 << mu
    low = (1 << k) - 1
    free = [0] * (3 * N)
    free[l] = 5 & low
    for x in range(l, N):
        free[N + x] = (7 * x + 3) & low
    classes = [[2 * N + x - 1, x] for x in range(l + 1, N)]
    return _circuit(mu, l, classes, [0] * l + [1] * (N - l), xor_table(N, k), free)


def flat(mu: int = 10, l: int = 4, k: int = 4) -> dict:
    """every row x >= l is a lookup row on two free inputs: ONE level of N rows (the input rows are on it too), one grid launch"""
    N = 1 << mu
    low = (1 << k) - 1
    free = [0] * (3 * N)
    for x in range(l, N):
        free[x], free[N + x] = (3 * x + 1) & low, (x * x + 11) & low
    return _circuit(mu, l, [], [0] * l + [1] * (N - l), xor_table(N, k), free)


def self_dependent(mu: int = 6, row: int = 33, l: int = 4, k: int = 3) -> dict:
    """the flat circuit, but the a slot of lookup row `row` sits in the class of its own c slot, and row + 1 reads that c"""
    N = 1 << mu
    c = flat(mu, l, k)
    c["sigma"] = wm.sigma_of(N, [[2 * N + row, row, row + 1]])
    return c
