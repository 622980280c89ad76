"""
The witness rules of zkhip.plonk (module text, WITNESS) in pure Python ints: cycles, sources, levels, evaluation and check.  Written from
the rules, not from the samplers: test_witness.py holds it against them.

A circuit is the dict of zkhip.plonk (selectors as [N, 4] Montgomery limbs, "sigma", "mu", "l", optionally "gate": "wide"); values are
CANONICAL ints here and turned into Montgomery limbs only by `limbs`.
"""
import numpy as np

from zkhip.field import R_MOD

R = R_MOD
_RINV = pow(1 << 256, -1, R)
BASIC, WIDE = ("q1", "q2"), ("qL", "qR", "qM", "qO", "qC", "qH")


def ints(a) -> list:
    """[n, 4] Montgomery limbs -> canonical ints (limbs at or above r are reduced first)"""
    raw = np.ascontiguousarray(a, dtype="<u8").tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") % R * _RINV % R for i in range(0, len(raw), 32)]


def limbs(xs) -> np.ndarray:
    """canonical ints -> [n, 4] fully reduced Montgomery limbs"""
    return np.frombuffer(b"".join(((x << 256) % R).to_bytes(32, "little") for x in xs), dtype="<u8").astype(np.uint64).reshape(-1, 4)


def selectors(circuit: dict) -> dict:
    return {k: ints(circuit[k]) for k in (WIDE if circuit.get("gate") == "wide" else BASIC)}


def computing_rows(circuit: dict, sel=None) -> list:
    """row x computes when its output coefficient is non-zero: every row of the basic gate, qO(x) != 0 of the wide one"""
    N = 1 << circuit["mu"]
    if circuit.get("gate") != "wide":
        return [True] * N
    return [q != 0 for q in (sel or selectors(circuit))["qO"]]


def plan(sigma, N: int, computing) -> dict:
    """
    -> {"src": per slot (free, v) -- free: v is the smallest slot of the class, else v is the source ROW (its c slot 2N + v is the smallest c
        slot of a computing row in the class), "level": per row its level (None: not computing), "levels": the rows of every level in
        ascending order}.  ValueError: sigma is not a permutation / "K of N rows depend on their own output" with the smallest such row.
    """
    sigma = [int(s) for s in sigma]
    if len(sigma) != 3 * N or sorted(sigma) != list(range(3 * N)):
        raise ValueError("sigma is not a permutation")
    src, seen = [None] * (3 * N), [False] * (3 * N)
    for s in range(3 * N):
        if seen[s]:
            continue
        cls, t = [], s
        while not seen[t]:
            seen[t] = True
            cls.append(t)
            t = sigma[t]
        cs = [t for t in cls if t >= 2 * N and computing[t - 2 * N]]
        v = (False, min(cs) - 2 * N) if cs else (True, min(cls))
        for t in cls:
            src[t] = v
    deps = lambda x: [v for free, v in (src[x], src[N + x]) if not free]
    # the level by its definition, depth first without recursion; 0 new, 1 being worked on, 2 done.  NONE: the row has no level
    NONE = -1
    level, state = [None] * N, [0] * N
    for x0 in range(N):
        if not computing[x0] or state[x0]:
            continue
        stack = [x0]
        state[x0] = 1
        while stack:
            x = stack[-1]
            todo = [d for d in deps(x) if state[d] == 0]
            if todo:
                state[todo[0]] = 1
                stack.append(todo[0])
                continue
            ds = deps(x)
            if any(state[d] == 1 or level[d] == NONE for d in ds):  # d == x, d further down the stack (a cycle), or d without a level
                level[x] = NONE
            else:
                level[x] = 1 + max(level[d] for d in ds) if ds else 0
            state[x] = 2
            stack.pop()
    bad = [x for x in range(N) if level[x] == NONE]
    if bad:
        raise ValueError(f"{len(bad)} of {N} rows depend on their own output; the first is row {bad[0]}")
    top = max((v for v in level if v is not None), default=-1)
    rows = [[] for _ in range(top + 1)]
    for x in range(N):
        if level[x] is not None:
            rows[level[x]].append(x)
    return {"N": N, "src": src, "level": level, "levels": rows}


def launches(p: dict, block: int = 256) -> list:
    """the launch schedule: (first level, one past the last) -- a level of more than `block` rows alone, a run of consecutive levels of at
    most `block` rows each together"""
    out, sizes, v = [], [len(r) for r in p["levels"]], 0
    while v < len(sizes):
        e = v + 1
        if sizes[v] <= block:
            while e < len(sizes) and sizes[e] <= block:
                e += 1
        out.append((v, e))
        v = e
    return out


def info(p: dict) -> dict:
    """what zk_witness_plan_info reports"""
    return {"levels": len(p["levels"]), "max_level_rows": max((len(r) for r in p["levels"]), default=0), "launches": len(launches(p))}


def _in(circuit, public_inputs):
    N = 1 << circuit["mu"]
    pi = ints(public_inputs) if len(public_inputs) else []
    return pi + [0] * (N - len(pi))


def out_value(sel: dict, wide: bool, x: int, a: int, b: int, inp: int) -> int:
    """the c that satisfies a computing row"""
    if not wide:
        return (sel["q1"][x] * (a + b) + sel["q2"][x] * a * b + inp) % R
    t = sel["qL"][x] * a + sel["qR"][x] * b + sel["qM"][x] * a * b + sel["qH"][x] * pow(a, 5, R) + sel["qC"][x] + inp
    return t * pow(sel["qO"][x], -1, R) % R


def gate_value(sel: dict, wide: bool, x: int, a: int, b: int, c: int, inp: int) -> int:
    """the gate identity of row x (0: it holds)"""
    if not wide:
        return (sel["q1"][x] * (a + b) + sel["q2"][x] * a * b - c + inp) % R
    return (sel["qL"][x] * a + sel["qR"][x] * b + sel["qM"][x] * a * b + sel["qH"][x] * pow(a, 5, R) - sel["qO"][x] * c + sel["qC"][x] + inp) % R


def generate(circuit: dict, p: dict, public_inputs, free=None):
    """-> (a, b, c) canonical ints.  free: 3N canonical ints (or None: zeros), read at the smallest slot of every free class"""
    N, wide, sel, inp = p["N"], circuit.get("gate") == "wide", selectors(circuit), _in(circuit, public_inputs)
    w = [[0] * N for _ in range(3)]
    value = lambda s: (free[s[1]] % R if free is not None else 0) if s[0] else w[2][s[1]]
    for rows in p["levels"]:
        for x in rows:
            w[0][x], w[1][x] = value(p["src"][x]), value(p["src"][N + x])
            w[2][x] = out_value(sel, wide, x, w[0][x], w[1][x], inp[x])
    for x in range(N):
        if p["level"][x] is None:
            for j in range(3):
                w[j][x] = value(p["src"][j * N + x])
    return w[0], w[1], w[2]


def check(circuit: dict, p: dict, a, b, c, public_inputs) -> dict:
    """any a, b, c (canonical ints) against the gates and the classes -> the dict of zkhip.plonk.check_witness"""
    N, wide, sel, inp = p["N"], circuit.get("gate") == "wide", selectors(circuit), _in(circuit, public_inputs)
    w = a + b + c
    rows = [x for x in range(N) if gate_value(sel, wide, x, a[x], b[x], c[x], inp[x])]
    rep = lambda s: s[1] if s[0] else 2 * N + s[1]  # the slot that holds the class's value
    slots = [s for s in range(3 * N) if w[s] != w[rep(p["src"][s])]]
    return {"bad_rows": len(rows), "first_bad_row": rows[0] if rows else None, "bad_copies": len(slots), "first_bad_copy": slots[0] if slots else None}


def free_of_lookup(circuit: dict) -> list:
    """the free values of a sample_circuit_lookup circuit: the a and b slots of its lookup rows are fixed points of sigma (free classes of
    one slot) and hold the table's u, v -- what a witness generator looks up itself.  Taken from the sampled wires at those slots only."""
    N = 1 << circuit["mu"]
    a, b = ints(circuit["a"]), ints(circuit["b"])
    qk = ints(circuit["lookup"]["qk"])
    free = [0] * (3 * N)
    for x in range(N):
        if qk[x]:
            free[x], free[N + x] = a[x], b[x]
    return free


# ---- hand-built circuits ----
def sigma_of(N: int, classes) -> np.ndarray:
    """one cycle per class (a list of slots, walked in ascending order); every other slot is a fixed point"""
    sigma = np.arange(3 * N, dtype=np.uint64)
    for cls in classes:
        cls = sorted(cls)
        for s, t in zip(cls, cls[1:] + cls[:1]):
            sigma[s] = t
    return sigma


def _users(N: int, l: int, ia, ib) -> list:
    """the classes of a circuit whose row x >= l takes a = c[ia(x)], b = c[ib(x)]"""
    cls = {}
    for x in range(l, N):
        cls.setdefault(ia(x), []).append(x)
        cls.setdefault(ib(x), []).append(N + x)
    return [[2 * N + y] + slots for y, slots in cls.items()]


def _basic(mu: int, l: int, ia, ib, seed: int) -> dict:
    N = 1 << mu
    rnd = lambda k: [(seed * 1000003 + 7919 * k + 31 * x * x + x) % 65521 + 1 for x in range(N)]
    q1, q2 = rnd(1), rnd(2)
    for x in range(l):
        q1[x] = q2[x] = 0
    return {"mu": mu, "l": l, "q1": limbs(q1), "q2": limbs(q2), "sigma": sigma_of(N, _users(N, l, ia, ib)), "public_inputs": limbs([seed + 11 * x + 2 for x in range(l)])}


def chain(mu: int, l: int = 4, seed: int = 5) -> dict:
    """row x >= l takes a = c[x - 1], b = c[x - l]: row x has level x - l + 1, so the deepest level is N - l and every level but the input
    rows' holds one row -- one single-workgroup run of N - l + 1 levels"""
    return _basic(mu, l, lambda x: x - 1, lambda x: x - l, seed)


def flat(mu: int, l: int = 4, seed: int = 6) -> dict:
    """row x >= l takes a = c[x mod l], b = c[(x + 1) mod l]: ONE level of N - l rows above the input rows"""
    return _basic(mu, l, lambda x: x % l, lambda x: (x + 1) % l, seed)


def self_dependent(mu: int, row: int, l: int = 4) -> dict:
    """the flat circuit, but the a slot of `row` sits in the class of its own c slot"""
    N = 1 << mu
    c = flat(mu, l)
    ia = lambda x: x if x == row else x % l
    c["sigma"] = sigma_of(N, _users(N, l, ia, lambda x: (x + 1) % l))
    return c


def wide_edge(broken_assert: bool = False, unequal: bool = False) -> dict:
    """
    Eight rows of the wide gate, l = 2:
      0, 1  input rows (qO = 1);
      2     qO = 3 (neither 0 nor 1): c = (a + b) / 3 with a = c[0], b = c[1];
      3     S-box: c = a^5 + 5 with a = c[2]; b is a free class (free[N + 3] = 9);
      4     qO = 0, an ASSERTION a - b = 0 with a = b = c[3] (broken_assert: qC = 1, so a - b + 1 != 0 -- one bad gate row, 4); its c slot is a
            free class (free[2N + 4] = 77);
      5     c = a with a = c[3], and its c slot lies in the class of c[3]: a class with TWO computing c slots, equal (unequal: qC = 1, so
            c[5] = c[3] + 1 -- one bad copy, slot 2N + 5);
      6, 7  rows with every selector 0: three free classes each (free[6] = 123, the others absent).
    -> the circuit plus "free": 3N canonical ints
    """
    N, l = 8, 2
    sel = {k: [0] * N for k in WIDE}
    sel["qO"][0] = sel["qO"][1] = 1
    sel["qL"][2], sel["qR"][2], sel["qO"][2] = 1, 1, 3
    sel["qH"][3], sel["qC"][3], sel["qO"][3] = 1, 5, 1
    sel["qL"][4], sel["qR"][4], sel["qC"][4] = 1, R - 1, int(broken_assert)
    sel["qL"][5], sel["qO"][5], sel["qC"][5] = 1, 1, int(unequal)
    classes = [[2 * N + 0, 2], [2 * N + 1, N + 2], [2 * N + 2, 3], [2 * N + 3, 4, N + 4, 5, 2 * N + 5]]
    free = [0] * (3 * N)
    free[N + 3], free[2 * N + 4], free[6] = 9, 77, 123
    c = {"gate": "wide", "mu": 3, "l": l, "sigma": sigma_of(N, classes), "public_inputs": limbs([6, 15]), "free": free}
    c.update({k: limbs(v) for k, v in sel.items()})
    return c
