"""
An independent pure-integer model of Poseidon zkhip-poseidon-v1 (imports nothing from zkhip/poseidon.py or zkhip/circuit.py): the constants from
their SHA-256 rule, the permutation, hash2, the Merkle tree, and a row-by-row evaluator of a wide-gate circuit dict that applies the witness
rules of the plonk module (classes = cycles of sigma; a class takes the c of its smallest computing c slot, else free[smallest slot]).
Written from the rule in include/zkhip.h, with its own loops: rounds are told apart by position lists, the matrix is applied column-wise.
"""
import hashlib

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
T, ALPHA, R_F, R_P = 3, 5, 8, 57
NAME = b"zkhip-poseidon-v1"


def constants():
    """(rc: 195 ints, M: 3 x 3 ints)"""
    rc = []
    for k in range(T * (R_F + R_P)):
        pre = NAME + bytes([k & 255, (k >> 8) & 255, (k >> 16) & 255, (k >> 24) & 255])
        wide = hashlib.sha256(pre + b"\x00").digest() + hashlib.sha256(pre + b"\x01").digest()
        rc.append(int.from_bytes(wide, "little") % R)
    xs, ys = (0, 1, 2), (3, 4, 5)
    M = [[pow(x + y, R - 2, R) for y in ys] for x in xs]  # Cauchy: 1 / (x_i + y_j) = 1 / (i + j + 3)
    return rc, M


def constants_sha256() -> str:
    """SHA-256 over rc[0..194] then M row-major, each as 32 little-endian bytes of the canonical integer"""
    rc, M = constants()
    h = hashlib.sha256()
    for v in rc + [v for row in M for v in row]:
        h.update(v.to_bytes(32, "little"))
    return h.hexdigest()


def derived_constants(rf: int, rp: int, name: bytes):
    """another instance by the same kind of rule under another name: the constants are data"""
    rc = [int.from_bytes(hashlib.sha256(name + b"/rc/" + str(k).encode()).digest() * 2, "little") % R for k in range(T * (rf + rp))]
    M = [[pow(1 + 2 * i + 7 * j + 11, R - 2, R) for j in range(T)] for i in range(T)]  # Cauchy on x = 1, 3, 5 and y = 11, 18, 25
    return rc, M


def permute(state, rf=R_F, rp=R_P, consts=None):
    rc, M = consts or constants()
    full_rounds = set(range(rf // 2)) | set(range(rf // 2 + rp, rf + rp))
    s = [v % R for v in state]
    for k in range(rf + rp):
        for i in range(T):
            s[i] = (s[i] + rc[T * k + i]) % R
        for i in (range(T) if k in full_rounds else (0,)):
            s[i] = pow(s[i], ALPHA, R)
        out = [0] * T
        for j in range(T):  # column by column
            for i in range(T):
                out[i] = (out[i] + M[i][j] * s[j]) % R
        s = out
    return tuple(s)


def hash2(left, right, **kw):
    return permute((0, left, right), **kw)[0]


def merkle(leaves, **kw):
    """2n - 1 elements: the leaves, n / 2 nodes, .., the root last"""
    level = [v % R for v in leaves]
    assert len(level) >= 1 and len(level) & (len(level) - 1) == 0
    tree = list(level)
    while len(level) > 1:
        level = [hash2(level[2 * i], level[2 * i + 1], **kw) for i in range(len(level) // 2)]
        tree += level
    return tree


def path_of(tree, n, index):
    """(siblings, bits) from the leaf level up"""
    sibs, bits, base = [], [], 0
    while n > 1:
        sibs.append(tree[base + (index ^ 1)])
        bits.append(index & 1)
        base, n, index = base + n, n // 2, index // 2
    return sibs, bits


def root_of_path(leaf, sibs, bits):
    cur = leaf
    for s, b in zip(sibs, bits):
        cur = hash2(s, cur) if b else hash2(cur, s)
    return cur


# ---- the circuit evaluator ----
_RINV = pow(1 << 256, R - 2, R)


def _ints(limbs):
    """[n, 4] u64 Montgomery limbs -> canonical integers"""
    out = []
    for row in limbs:
        v = 0
        for i, w in enumerate(row):
            v |= int(w) << (64 * i)
        out.append(v * _RINV % R)
    return out


def evaluate(circuit, public_inputs, free=None):
    """
    circuit: a wide-gate dict; public_inputs: l canonical ints; free: {slot: canonical int} (absent: 0).
    -> {"a", "b", "c": N ints, "bad_rows": rows whose gate identity fails, "bad_copies": slots whose value differs from their class's,
        "classes": list of slot lists (the cycles of sigma with more than one slot)}
    Rows are generated in ascending order; a row that reads a class whose source row comes later raises (the builder never emits one).
    """
    assert circuit["gate"] == "wide"
    mu, l = int(circuit["mu"]), int(circuit["l"])
    N = 1 << mu
    free = free or {}
    q = {k: _ints(circuit[k]) for k in ("qL", "qR", "qM", "qO", "qC", "qH")}
    sigma = [int(s) for s in circuit["sigma"]]
    assert sorted(sigma) == list(range(3 * N)), "sigma is not a permutation"
    assert len(public_inputs) == l
    cls = [None] * (3 * N)
    classes = []
    for s in range(3 * N):
        if cls[s] is None:
            cyc, t = [], s
            while cls[t] is None:
                cls[t] = len(classes)
                cyc.append(t)
                t = sigma[t]
            classes.append(sorted(cyc))
    source = []  # per class: ("row", x) or ("free", slot)
    for cyc in classes:
        comp = [s - 2 * N for s in cyc if s >= 2 * N and q["qO"][s - 2 * N] != 0]
        source.append(("row", min(comp)) if comp else ("free", cyc[0]))
    inp = [public_inputs[x] % R if x < l else 0 for x in range(N)]
    a, b, c = [None] * N, [None] * N, [None] * N

    def value(slot):
        kind, at = source[cls[slot]]
        if kind == "free":
            return free.get(at, 0) % R
        assert c[at] is not None, f"slot {slot} reads row {at} before it is computed"
        return c[at]

    def lhs(x):
        return (q["qL"][x] * a[x] + q["qR"][x] * b[x] + q["qM"][x] * a[x] * b[x] + q["qH"][x] * pow(a[x], 5, R) + q["qC"][x] + inp[x]) % R

    for x in range(N):
        if q["qO"][x] != 0:
            a[x], b[x] = value(x), value(N + x)
            c[x] = lhs(x) * pow(q["qO"][x], R - 2, R) % R
    for x in range(N):
        if q["qO"][x] == 0:
            a[x], b[x], c[x] = value(x), value(N + x), value(2 * N + x)
    bad_rows = [x for x in range(N) if (lhs(x) - q["qO"][x] * c[x]) % R != 0]
    wires = a + b + c
    bad_copies = [s for s in range(3 * N) if wires[s] != value(s)]
    return {"a": a, "b": b, "c": c, "bad_rows": bad_rows, "bad_copies": bad_copies, "classes": [cy for cy in classes if len(cy) > 1]}
