"""
The witness rules WITH advice (zkhip.plonk module text, WITNESS; include/zkhip.h) in pure Python ints, on top of witness_model.py and
witness_lookup_model.py: the codes, the three kinds of computing rows, the refusals with their numbers, sources, levels and launches,
evaluation and the check -- which does not look at the codes.  Written from the rules, not from the builder: test_advice.py holds the
builder's gadgets against it.

A circuit is the dict of zkhip.plonk with "advice": N u32 codes (absent: none) and, for `lookup=True`, "lookup"; values are canonical ints.
"""
import numpy as np

import witness_lookup_model as wlm
import witness_model as wm

GATE, LOOKUP, ADVICE = 1, 2, 3  # the kind of a computing row (0: it computes nothing)
INV0 = 1


def bits(shift: int, width: int) -> int:
    """the code of a bit field, put together without any check (the tests also need unknown ones)"""
    return 2 | shift << 8 | width << 16


def known(code: int) -> bool:
    kind, shift, width = code & 0xFF, (code >> 8) & 0xFF, (code >> 16) & 0xFF
    if code >> 24:
        return False
    if kind in (0, 1):
        return code == kind
    return kind == 2 and 1 <= width <= 64 and shift + width <= 255


def value(code: int, a: int) -> int:
    """the c of an advice row whose a holds the canonical integer a"""
    if code == INV0:
        return pow(a, -1, wm.R) if a else 0
    return (a >> ((code >> 8) & 0xFF)) % (1 << ((code >> 16) & 0xFF))


def codes(circuit: dict) -> list:
    N = 1 << circuit["mu"]
    return [int(v) for v in circuit["advice"]] if "advice" in circuit else [0] * N


def plan(circuit: dict, lookup: bool = False) -> dict:
    """witness_model.plan with the three kinds of rows computing, plus "kind" and "advice" (per row) and, with lookup, "table".
    ValueError: "K of N advice codes are unknown; the first is row X", "K of N advice rows also compute by the gate or the table; the
    first is row X", and what the two models below raise"""
    N = 1 << circuit["mu"]
    adv = codes(circuit)
    bad = [x for x in range(N) if not known(adv[x])]
    if bad:
        raise ValueError(f"{len(bad)} of {N} advice codes are unknown; the first is row {bad[0]}")
    tab = wlm.table(circuit) if lookup else None
    kind = wlm.kinds(circuit, tab) if lookup else [GATE if g else 0 for g in wm.computing_rows(circuit)]
    bad = [x for x in range(N) if adv[x] and kind[x]]
    if bad:
        raise ValueError(f"{len(bad)} of {N} advice rows also compute by the gate or the table; the first is row {bad[0]}")
    kind = [ADVICE if adv[x] else kind[x] for x in range(N)]
    p = wm.plan(circuit["sigma"], N, [k != 0 for k in kind])
    p.update(kind=kind, advice=adv)
    if lookup:
        p["table"] = tab
    return p


launches, info = wm.launches, wm.info


def generate(circuit: dict, p: dict, public_inputs, free=None):
    """-> (a, b, c) canonical ints: an advice row takes its c from its code and a, a lookup row from the table, every other from the gate"""
    N, wide, sel, inp = p["N"], circuit.get("gate") == "wide", wm.selectors(circuit), wm._in(circuit, public_inputs)
    w = [[0] * N for _ in range(3)]
    val = lambda s: (free[s[1]] % wm.R if free is not None else 0) if s[0] else w[2][s[1]]
    for rows in p["levels"]:
        for x in rows:
            w[0][x], w[1][x] = val(p["src"][x]), val(p["src"][N + x])
            if p["kind"][x] == ADVICE:
                w[2][x] = value(p["advice"][x], w[0][x])
            elif p["kind"][x] == LOOKUP:
                y = p["table"]["first"].get((w[0][x], w[1][x]))
                w[2][x] = p["table"]["t"][y][2] if y is not None else 0
            else:
                w[2][x] = wm.out_value(sel, wide, x, w[0][x], w[1][x], inp[x])
    for x in range(N):
        if p["level"][x] is None:
            for j in range(3):
                w[j][x] = val(p["src"][j * N + x])
    return w[0], w[1], w[2]


def check(circuit: dict, p: dict, a, b, c, public_inputs) -> dict:
    """the check of the plan's kind -- four numbers, six with a lookup; no advice value is tested"""
    return (wlm.check if "table" in p else wm.check)(circuit, p, a, b, c, public_inputs)


# ---- hand-built circuits: the wide gate, l input rows, the rows after them given one by one ----
def gate_row(a=None, b=None, **sel) -> dict:
    """a computing gate row: sel holds qL, qR, qM, qC, qH (qO = 1 unless given).  a, b: ("c", row), ("free", value) or None (free, 0)"""
    return {"sel": dict({"qO": 1}, **sel), "a": a, "b": b}


def advice_row(code: int, a=None, b=None, **sel) -> dict:
    return {"sel": sel, "adv": code, "a": a, "b": b}


def lookup_row(a=None, b=None) -> dict:
    return {"sel": {}, "qk": 1, "a": a, "b": b}


def circuit_of(mu: int, l: int, rows, table: dict | None = None) -> dict:
    """input rows 0 .. l - 1 (qO = 1), then `rows` (row l + i is rows[i]), then rows with every selector 0.  -> the circuit plus "free": 3N
    canonical ints (values at or above r are kept as given) and "public_inputs".  table: the columns t0, t1, t2 of a lookup (N ints each)"""
    N = 1 << mu
    assert l + len(rows) <= N
    sel = {q: [0] * N for q in wm.WIDE}
    for x in range(l):
        sel["qO"][x] = 1
    adv, qk, free, cls = [0] * N, [0] * N, [0] * (3 * N), {}
    for i, r in enumerate(rows):
        x = l + i
        for q, v in r["sel"].items():
            sel[q][x] = v % wm.R
        adv[x], qk[x] = r.get("adv", 0), r.get("qk", 0)
        for j, s in enumerate((r["a"], r["b"])):
            if s is None:
                continue
            if s[0] == "c":
                cls.setdefault(s[1], []).append(j * N + x)
            else:
                free[j * N + x] = s[1]
    classes = [[2 * N + y] + slots for y, slots in cls.items()]
    c = {"gate": "wide", "mu": mu, "l": l, "sigma": wm.sigma_of(N, classes), "public_inputs": wm.limbs([3 + 5 * x for x in range(l)]), "free": free,
         "advice": np.array(adv, dtype=np.uint32)}
    c.update({q: wm.limbs(v) for q, v in sel.items()})
    if table is not None:
        c["lookup"] = dict({q: wm.limbs(v) for q, v in table.items()}, qk=wm.limbs(qk))
    return c


def free_limbs(free) -> np.ndarray:
    """3N integers below 2^256 -> the [3N, 4] array a caller hands over: Montgomery forms, and a value at or above r AS IT STANDS"""
    return np.frombuffer(b"".join((v if v >= wm.R else (v << 256) % wm.R).to_bytes(32, "little") for v in free), dtype="<u8").astype(np.uint64).reshape(-1, 4)


def free_values(free) -> list:
    """what the generator reads of free_limbs(free), as canonical ints: a stored value at or above r is reduced, then taken out of Montgomery form"""
    return [v % wm.R * wm._RINV % wm.R if v >= wm.R else v for v in free]


def flat(mu: int, l: int, items) -> dict:
    """row l + i is an advice row with code items[i][0] on the free value items[i][1]: ONE level (the input rows are on it too)"""
    return circuit_of(mu, l, [advice_row(code, ("free", v)) for code, v in items])


def inverse_chain(mu: int, l: int, levels: int, start: int = 12345) -> dict:
    """one row per level: a gate row c = a + b on two free values, then alternately an INV0 row and a gate row c = a of the row before --
    levels + 1 levels in ONE single-workgroup run; the inverse of an inverse returns the value"""
    rows = [gate_row(("free", start), ("free", 1), qL=1, qR=1)]
    for k in range(levels):
        prev = ("c", l + len(rows) - 1)
        rows.append(advice_row(INV0, prev) if k % 2 == 0 else gate_row(prev, qL=1))
    return circuit_of(mu, l, rows)


def mixed(mu: int, l: int, width: int, depth: int) -> dict:
    """`depth` levels of `width` rows each above the input rows; row j of a level reads the c of row j of the level below (level 0: a free
    value) and is, by j + level, a gate row c = 3 a + 1, an INV0 row or a bit field of 13 bits at bit 7 * (j mod 30)"""
    rows = []
    for k in range(depth):
        for j in range(width):
            a = ("c", l + (k - 1) * width + j) if k else ("free", 1000003 * j + 17)
            t = (j + k) % 3
            rows.append(gate_row(a, qL=3, qC=1) if t == 0 else advice_row(INV0 if t == 1 else bits(7 * (j % 30), 13), a))
    return circuit_of(mu, l, rows)
