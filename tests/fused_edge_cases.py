"""
The fused identity sumchecks (csrc/zk_fused.cuh, csrc/zk_fs.hip, csrc/zk_gate.cuh) at extreme STORED values: the cases that
tests/test_gpu_fused_edges.py runs on the device and tests/test_fused_edge_inputs.py proves properties of (a helper, not a test), so
that both files speak of the same inputs.  Everything here is a stored integer -- what a kernel reads -- in [0, r).

Besides the cases: the brackets of zk_gate.cuh restated on stored integers (mul = a b R^-1 mod r), a big-int restatement of the two
engines that keeps the INTEGERS the passes hold (each lane's 17-limb sum, each wave's, the pass total W0 + W1 2^256 + W2 2^512, the
lane's free sums g0, gd) and the closed forms of constant tables.
"""
import lookup_model as lm
import plonk_lookup_model as plm
import plonk_model as pm
import pyoracle as po
import widegate_model as wg
import wiring_model as wm
import zerocheck_model as zm
from helpers import EDGE_TABLES, M_INT, ONE_INT, R_MOD, chal_set, edge_table, fr_ints

r = R_MOD
R = 1 << 256
MASK = R - 1
RINV = pow(R, -1, r)
BLOCK, WAVE = 256, 64


def mul(a, b):
    """fr_mul on stored integers"""
    return a * b * RINV % r


# ---- the brackets of zk_gate.cuh on stored integers, v in the Kind's table order ----
def _gate(g, v):
    return (mul(v[1], (v[3] + v[4]) % r) + mul(mul(v[2], v[3]), v[4]) - v[5] + v[6]) % r


def _wiring(g, v):
    return (v[1] - mul(v[2], v[3]) + mul(g, (mul(v[6], v[4]) - v[5]) % r)) % r


def _perm3(g, v):
    dd = mul(mul(mul(v[8], v[9]), v[10]), v[4])
    nn = mul(mul(v[5], v[6]), v[7])
    return (v[1] - mul(v[2], v[3]) + mul(g, (dd - nn) % r)) % r


def _gatew(g, v):
    a, b = v[7], v[8]
    a2 = mul(a, a)
    a5 = mul(mul(a2, a2), a)
    return (mul(v[1], a) + mul(v[2], b) + mul(mul(v[3], a), b) + mul(v[6], a5) - mul(v[4], v[9]) + v[5] + v[10]) % r


def _lookup(g, v):
    return (mul(v[4], v[1]) - ONE_INT + mul(g, (mul(v[5], v[2]) - v[3]) % r)) % r


def _lookupsel(g, v):
    return (mul(v[4], v[1]) - v[6] + mul(g, (mul(v[5], v[2]) - v[3]) % r)) % r


TREE4, TREE8 = ("eq", "tree", "num", "den"), ("eq", "tree", "n0", "n1", "n2", "d0", "d1", "d2")


class Kind:
    def __init__(self, name, knob, tables, uploaded, evals, local_max, per_cu, pass_wg, gamma, free, inner, model):
        self.name, self.knob, self.tables, self.uploaded, self.evals, self.local_max = name, knob, tables, uploaded, evals, local_max
        self.per_cu, self.pass_wg, self.gamma, self.free, self.inner, self.model = per_cu, pass_wg, gamma, free, inner, model
        self.tree = "tree" in uploaded


# per Kind: its hand-over knob, the tables of the identity, what is uploaded, evaluations per round, the default hand-over length,
# workgroups per CU of its passes, the knob that overrides them (gate and wiring only), has gamma, has the free term hf - ht,
# the bracket, the big-int model(tabs, gamma, chal) on FIELD values
KINDS = {k.name: k for k in (
    Kind("gate", "gate_local_e", zm.TABLES, zm.TABLES, 5, 512, 2, "gate_pass_wg", False, False, _gate, lambda t, g, ch: zm.sumcheck_gate(t, ch)),
    Kind("wiring", "wiring_local_e", wm.TABLES, TREE4, 4, 512, 2, "wiring_pass_wg", True, False, _wiring, wm.sumcheck_wiring),
    Kind("perm3", "perm3_local_e", pm.TABLES, TREE8, 6, 256, 1, None, True, False, _perm3, pm.sumcheck_perm3),
    Kind("gate_wide", "gatew_local_e", wg.TABLES, wg.TABLES, 8, 256, 1, None, False, False, _gatew, lambda t, g, ch: wg.sumcheck_gate_wide(t, ch)),
    Kind("lookup", "lookup_local_e", lm.TABLES, lm.TABLES, 4, 512, 2, None, True, True, _lookup, lm.sumcheck_lookup),
    Kind("lookup_sel", "lookupsel_local_e", plm.TABLES, plm.TABLES, 4, 512, 1, None, True, True, _lookupsel, plm.sumcheck_lookup_sel),
)}
# the order of the tables is the order of the calls' arguments and of their last values
assert zm.TABLES == ("eq", "q1", "q2", "a", "b", "c", "in") and wm.TABLES == ("eq", "v1x", "vx0", "vx1", "h", "num", "den")
assert pm.TABLES == ("eq", "v1x", "vx0", "vx1", "h", "n0", "n1", "n2", "d0", "d1", "d2")
assert wg.TABLES == ("eq", "qL", "qR", "qM", "qO", "qC", "qH", "a", "b", "c", "in")
assert lm.TABLES == ("E", "df", "dt", "m", "hf", "ht") and plm.TABLES == lm.TABLES + ("qk",)

PATTERNS = ("allM", "allNearM", "allZero", "macM", "lo0_hiM", "loM_hi0", "bit0_M", "bitmid_M") + tuple("rot%d" % s for s in range(6)) + ("rand", "lateW1")
NAMES = ("rand", "M", "zero", "one")  # of the gammas and of the preset challenge sets
# (mu, value of the Kind's *_local_e knob or None for its default): three HBM passes of 8, 4, 2 pairs | passes to the last element and
# a local stage of zero rounds | the local stage alone | one or two passes of several workgroups, then a local stage
SHAPES = [(4, 2), (4, 1), (6, None), (10, None)]

# macM: constant tables with eq (E) = M and the bracket's stored value = M, so both operands of fp_mac_wide are M at every pair and t
# (d = 0: the t-stepping leaves the constants).  One additive table of each Kind solved backwards, the others 0:
#   gate, wide gate   in = M | qC = M                                        [0 + 0 - 0 + M]
#   wiring            gamma = ONE (the field's 1), num = 1:                  0 - 0 + 1 (0 - 1) = r - 1
#   perm3             gamma = ONE, n0 = 1, n1 = n2 = ONE: n0 n1 n2 = 1       0 - 0 + 1 (0 - 1) = r - 1
#   lookup            gamma = ONE, m = 1 - ONE: -ONE + 1 (0 - m)             = -ONE - 1 + ONE = r - 1;  hf = M, ht = 0 (df = dt = 0 hides them)
#   lookup_sel        qk = 1: 0 - 1 + gamma (0 - 0) = r - 1 for ANY gamma;   hf = M, ht = 0
MAC_M = {
    "gate": ({"eq": M_INT, "in": M_INT}, None),
    "wiring": ({"eq": M_INT, "num": 1}, ONE_INT),
    "perm3": ({"eq": M_INT, "n0": 1, "n1": ONE_INT, "n2": ONE_INT}, ONE_INT),
    "gate_wide": ({"eq": M_INT, "qC": M_INT}, None),
    "lookup": ({"E": M_INT, "m": (1 - ONE_INT) % r, "hf": M_INT}, ONE_INT),
    "lookup_sel": ({"E": M_INT, "qk": 1, "hf": M_INT}, None),
}

# lateW1: the macM constants with another eq (E) and no free term (hf = 0), so the first pass of 2^9 pairs totals W = 512 E M for every
# Kind.  E is draw 1724 of SplitMix64(9100), the first whose total has W1 >= 2r AND W0 R^-1 + (W1 - 2r) + W2 R >= 2r (each term
# reduced): there a reduction that subtracts r from W1 only once leaves a sum that the two fr_add of gate_reduce_value cannot bring below
# r.  It needs W2 R mod r large, hence many products: with W2 <= 1 that term is at most R mod r = 0.208 r and the sum stays below 2r.
LATE_E = 0x360bd88c1bf71a64cf1214a237ab90c1636bfa0fcc4ecaafa1d40a31a193d6eb
LATE_W1 = {k: ({**{n: v for n, v in c.items() if n != "hf"}, ("E" if "E" in c else "eq"): LATE_E}, g) for k, (c, g) in MAC_M.items()}
CONST = {"macM": MAC_M, "lateW1": LATE_W1}

_INS = {}


def inputs(kind, pattern, mu):
    """-> (what is uploaded: name -> list of stored integers (the tree: 2N of them), gamma the pattern fixes or None)"""
    key = (kind, pattern, mu)
    if key not in _INS:
        K = KINDS[kind]
        size = lambda k: mu + 1 if k == "tree" else mu
        fixed = None
        if pattern in CONST:
            const, fixed = CONST[pattern][kind]
            ins = {k: [const.get(k, 0)] * (1 << size(k)) for k in K.uploaded}
        else:
            if pattern.startswith("rot"):
                names = [EDGE_TABLES[(i + int(pattern[3:])) % 6] for i in range(len(K.uploaded))]
            else:
                names = [{"allM": "M", "allNearM": "nearM", "allZero": "zero"}.get(pattern, pattern)] * len(K.uploaded)
            ins = {k: fr_ints(edge_table(nm, size(k), seed=3 * i + sorted(KINDS).index(kind))) for i, (k, nm) in enumerate(zip(K.uploaded, names))}
        assert all(0 <= x < r for v in ins.values() for x in v)
        _INS[key] = (ins, fixed)
    return _INS[key]


def scalar(name, seed=0):
    """a gamma by name (stored)"""
    return fr_ints(chal_set(name, 1, seed=40 + seed))[0]


def gamma_of(kind, pattern, gname, mu):
    fixed = inputs(kind, pattern, mu)[1]
    if not KINDS[kind].gamma:
        return 0
    return fixed if fixed is not None else scalar(gname)


def gammas_of(kind, pattern):
    """the gamma names a pattern is crossed with"""
    if not KINDS[kind].gamma:
        return ("none",)
    return ("fixed",) if pattern in CONST and CONST[pattern][kind][1] is not None else NAMES


def challenges(cname, mu):
    return fr_ints(chal_set(cname, mu, seed=7))[:mu]


def combos(kind, mu):
    """preset-challenge cases (pattern, gamma name, challenge set): the full cross product at the small sizes; above, every pattern on
    random challenges (the gammas taking turns) and allM / macM on every challenge set -- the rule of test_gpu_sumcheck_edges.combos"""
    if mu <= 6:
        return [(p, g, c) for p in PATTERNS for g in gammas_of(kind, p) for c in NAMES]
    turn = lambda p: gammas_of(kind, p)[PATTERNS.index(p) % len(gammas_of(kind, p))]
    return [(p, turn(p), "rand") for p in PATTERNS] + [(p, turn(p), c) for p in ("allM", "macM") for c in NAMES[1:]]


def fs_combos(kind, mu):
    """transcript-driven cases (pattern, gamma name): the challenges are the call's own"""
    if mu <= 6:
        return [(p, g) for p in PATTERNS for g in gammas_of(kind, p)]
    return [(p, gammas_of(kind, p)[PATTERNS.index(p) % len(gammas_of(kind, p))]) for p in PATTERNS]


def tables_of(kind, ins):
    """what is uploaded -> the identity's tables in the Kind's order (the four views of the tree as wiring_model states them)"""
    K = KINDS[kind]
    t = dict(ins)
    if K.tree:
        t.update(wm.views(ins["tree"]))
    return [t[k] for k in K.tables]


# ---- the identity models, which take field values: x R^-1 in, x R out ----
def to_field(xs):
    return [x * RINV % r for x in xs]


def to_stored(xs):
    return [x * R % r for x in xs]


def model_preset(kind, ins, gamma, chal, check_mont=False):
    """the identity's big-int model on the stored tables -> (rounds, last) as stored integers"""
    K = KINDS[kind]
    tabs = dict(zip(K.tables, (to_field(t) for t in tables_of(kind, ins))))
    if check_mont:  # the models' own conversion gives back exactly what the kernel reads
        for k, t in zip(K.tables, tables_of(kind, ins)):
            assert fr_ints(zm.mont(tabs[k])) == t, k
    rounds, last = K.model(tabs, gamma * RINV % r, to_field(chal))
    return [to_stored(p) for p in rounds], to_stored(last)


SEED = b"fused-edges"


def model_fs(kind, ins, gamma):
    """the model driven by the hashlib transcript (fs_model) -> (rounds, last, chal) as stored integers"""
    import fs_model as fm

    K = KINDS[kind]
    tabs = dict(zip(K.tables, (to_field(t) for t in tables_of(kind, ins))))
    tr = fm.Model(b"diff").absorb(SEED)
    rounds, last, chal = fm._stepwise(tr, tabs, lambda cur, ch: K.model(cur, gamma * RINV % r, ch)[0])
    return [to_stored(p) for p in rounds], to_stored([last[k] for k in K.tables]), to_stored(chal)


# ---- the engines on integers ----
def blocks_of(half, cu, per_cu):
    return min(-(-half // BLOCK), cu * per_cu)


def engine(kind, ins, gamma, chal=None, local_e=None, cu=256, per_cu=None):
    """
    run_preset (chal: one stored challenge per round) or run_fs (chal None: drawn from a hashlib transcript after each round) restated:
    passes while the tables are longer than the hand-over length, grid-stride lanes of `blocks` workgroups of 256, waves of 64.
    -> dict rounds, last, chal (stored), passes: per pass and evaluation a dict of the integers, flags: the C5 events seen
    (step_r: an unreduced v + d of exactly r in the t-stepping, fold_r: an unreduced lo + r (hi - lo) of exactly r, d_M: a difference M)
    """
    import hashlib

    K = KINDS[kind]
    cur = [list(t) for t in tables_of(kind, ins)]
    N = len(cur[0])
    mu = N.bit_length() - 1
    emax = local_e or K.local_max
    per_cu = per_cu or K.per_cu
    state = hashlib.sha256(hashlib.sha256(b"zkhip-fs-v1" + b"diff").digest() + bytes([0]) + SEED).digest()
    out = {"rounds": [], "chal": [], "passes": [], "flags": set()}
    nt = len(cur)
    for i in range(mu):
        half = len(cur[0]) // 2
        prods = [[0] * half for _ in range(K.evals)]  # the raw 512-bit products
        frees = [(0, 0)] * half
        all_M = True
        for j in range(half):
            v = [t[j] for t in cur]
            d = [(t[j + half] - t[j]) % r for t in cur]
            if M_INT in d:
                out["flags"].add("d_M")
            if K.free:
                frees[j] = ((v[4] - v[5]) % r, (d[4] - d[5]) % r)
            for t in range(K.evals):
                b = K.inner(gamma, v)
                all_M = all_M and v[0] == M_INT and b == M_INT
                prods[t][j] = v[0] * b
                if t + 1 < K.evals:
                    if any(x + y == r for x, y in zip(v, d)):
                        out["flags"].add("step_r")
                    v = [(x + y) % r for x, y in zip(v, d)]
        if len(cur[0]) > emax:  # an HBM pass: integers
            nl = blocks_of(half, cu, per_cu) * BLOCK
            g0 = [sum(f[0] for f in frees[L::nl]) % r for L in range(min(nl, half))]
            gd = [sum(f[1] for f in frees[L::nl]) % r for L in range(min(nl, half))]
            evals, per_t = [], []
            for t in range(K.evals):
                lane_p = [sum(prods[t][L::nl]) for L in range(min(nl, half))]
                g = [(a + t * b) % r for a, b in zip(g0, gd)]
                lanes = [p + (x << 256) for p, x in zip(lane_p, g)]
                waves = [lanes[w:w + WAVE] for w in range(0, len(lanes), WAVE)]
                W = sum(lanes)
                assert W < 1 << 544
                w0, w1, w2 = W & MASK, (W >> 256) & MASK, W >> 512
                evals.append((w0 % r * RINV + w1 + w2 * R) % r)
                per_t.append({
                    "W": W, "w0_band": min(w0 // r, 2), "w1_band": min(w1 // r, 2), "w2": w2, "lane_max": max(lanes), "iters": -(-half // nl),
                    "wave_from_shuffle": any(sum(w) >> 512 and not any(x >> 512 for x in w) for w in waves),
                    "hi_carry": any((((p >> 256) & MASK) + x) >> 256 for p, x in zip(lane_p, g)),
                    "mac_M": all_M, "w1_late": w1 >= 2 * r and w0 % r * RINV % r + (w1 - 2 * r) + w2 * R % r >= 2 * r,
                })
            out["passes"].append(per_t)
        else:  # the local stage: reduced sums
            evals = [(sum(mul(1, p) for p in prods[t]) + sum((f[0] + t * f[1]) for f in frees)) % r for t in range(K.evals)]
        out["rounds"].append(evals)
        if chal is not None:
            c = chal[i]
        else:
            state = hashlib.sha256(state + bytes([0]) + b"".join(x.to_bytes(32, "little") for x in evals)).digest()
            state = hashlib.sha256(state + bytes([1])).digest()
            c = (int.from_bytes(state, "little") % (1 << 254)) * R % r
        out["chal"].append(c)
        nxt = []
        for t in cur:
            x = [mul(c, (t[j + half] - t[j]) % r) for j in range(half)]
            if any(t[j] + x[j] == r for j in range(half)):
                out["flags"].add("fold_r")
            nxt.append([(t[j] + x[j]) % r for j in range(half)])
        cur = nxt
    out["last"] = [t[0] for t in cur]
    return out


# ---- constant tables: closed forms and the large cases ----
def const_values(kind, const):
    """the stored constants of the identity's tables (the views of a constant tree are that constant)"""
    K = KINDS[kind]
    return [const.get("tree" if (K.tree and k in ("v1x", "vx0", "vx1", "h")) else k, 0) for k in K.tables]


def closed_form(kind, const, gamma, mu):
    """constant tables: round i over h = N >> (i+1) pairs returns h (E B R^-1 + F) at every t, and the last values are the constants
    (the fold of a constant is that constant whatever the challenge) -> (rounds, last) stored"""
    K = KINDS[kind]
    v = const_values(kind, const)
    F = (v[4] - v[5]) % r if K.free else 0
    term = (mul(v[0], K.inner(gamma, v)) + F) % r
    return [[(1 << (mu - i - 1)) * term % r] * K.evals for i in range(mu)], v


def lane_model(kind, const, gamma, mu, cu, per_cu, t=0):
    """one lane of the FIRST pass over constant tables, `it` grid-stride iterations: -> (the lane's sum of products, its g0) of the
    busiest lane (lane 0)"""
    K = KINDS[kind]
    v = const_values(kind, const)
    half = 1 << (mu - 1)
    it = -(-half // (blocks_of(half, cu, per_cu) * BLOCK))
    F = (v[4] - v[5]) % r if K.free else 0
    return it, it * v[0] * K.inner(gamma, v), it * F % r


def large_case(kind, cu):
    """
    The smallest table at which one lane of the first pass passes 2^512 inside its loop (C3) on the macM constants and, for the lookups,
    the add of its free term carries out of limb 15 (C4): hf is chosen so that the busiest lane's g0 = it * hf is M.
    -> (mu, knobs to set, constants, gamma, it) or None if no size up to 2^22 does
    """
    K = KINDS[kind]
    const, gamma = MAC_M[kind]
    gamma = (gamma if gamma is not None else ONE_INT) if K.gamma else 0
    per_cu, knobs = (1, {K.pass_wg: 1}) if K.pass_wg else (K.per_cu, {})
    for mu in range(10, 23):
        if (1 << mu) <= K.local_max:
            continue
        c = dict(const)
        it, p, g0 = lane_model(kind, c, gamma, mu, cu, per_cu)
        if K.free:
            c["hf"], c["ht"] = M_INT * pow(it, -1, r) % r, 0
            it, p, g0 = lane_model(kind, c, gamma, mu, cu, per_cu)
            assert g0 == M_INT
        if p >> 512 and (not K.free or (((p >> 256) & MASK) + g0) >> 256):
            return mu, knobs, c, gamma, it
    return None
