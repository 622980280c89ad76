"""
Plain-integer model of the MSM's XYZZ group arithmetic (csrc/curve30.cuh for G1, csrc/curve30_g2.cuh for G2), for
tests/test_gpu_xyzz.py (test hooks zk_dbg_xyzz_op / zk_dbg_xyzz2_op) and tests/test_xyzz_model.py.

The reference of every operation is the AFFINE chord / tangent map, not the EFD XYZZ formulas the device runs:
    chord   lambda = (y2 - y1) / (x2 - x1)        tangent (a = 0)   lambda = 3 x^2 / 2 y
    x3 = lambda^2 - x1 - x2                         y3 = lambda (x1 - x3) - y1
with infinity, equal points and opposite points by the group law.  A device result (X, Y, ZZ, ZZZ) is decoded as x = X / ZZ,
y = Y / ZZZ, which does not depend on how the device scales its coordinates.  The formulas for a = 0 never read the curve constant, so
operands need not lie on the curve; they must be consistent XYZZ points (ZZ = z^2, ZZZ = z^3 for some z).

Field elements are tuples of integers below q: 1 component for Fq, 2 for Fq2 = Fq[u] / (u^2 + 1).  Coordinates on the device are in the
internal Montgomery form of radix 2^390: the stored residue of a value v is v * 2^390 mod q.  An operand is 4 stored coordinates
(X, Y, ZZ, ZZZ) and a lift of the same shape: the device works on the exact integer residue + lift * q.
"""
from collections import namedtuple
from functools import lru_cache
from typing import List, Optional, Sequence, Tuple

import pyoracle as po
from pairing_tower_model import Q, RADIX, RADIX_INV, limbs_to_int, rand_fq

LIFT_MAX = (7, 3, 1, 1)  # X < 8q, Y < 4q, ZZ < 2q, ZZZ < 2q
BOUND = (8, 4, 2, 2)
MODES = ("madd", "madd_neg", "add", "dbl", "dbl_affine", "add_quad", "acc_quad")
UNARY = ("dbl", "dbl_affine")
VARIANTS = ("zero", "max", "mixed")
R390 = RADIX % Q
R384 = (1 << 384) % Q
# residues at the edges: 0, 1, q-1, q-2, 2^360 - 1 (twelve all-ones 30-bit limbs, top limb zero), 2^380 - 1 (all-ones limbs as far as
# q allows: q has 381 bits), the residues of 2^390 (the Montgomery one) and of 2^384
EXTREMES = (0, 1, Q - 1, Q - 2, (1 << 360) - 1, (1 << 380) - 1, R390, R384)


class Curve:
    """field arithmetic for one of the two groups; elements are tuples of `deg` integers below q"""

    def __init__(self, name: str, deg: int):
        self.name, self.deg = name, deg
        self.zero = (0,) * deg
        self.one = (1,) + (0,) * (deg - 1)

    def add(self, a, b):
        return tuple((x + y) % Q for x, y in zip(a, b))

    def sub(self, a, b):
        return tuple((x - y) % Q for x, y in zip(a, b))

    def neg(self, a):
        return tuple(-x % Q for x in a)

    def smul(self, a, k: int):
        return tuple(x * k % Q for x in a)

    def mul(self, a, b):
        if self.deg == 1:
            return (a[0] * b[0] % Q,)
        return ((a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q)  # u^2 = -1

    def inv(self, a):
        if self.deg == 1:
            return (pow(a[0], -1, Q),)
        n = pow(a[0] * a[0] + a[1] * a[1], -1, Q)
        return (a[0] * n % Q, -a[1] * n % Q)

    def div(self, a, b):
        return self.mul(a, self.inv(b))

    def elem(self, *v):
        """a field element from integers (missing components repeat the last one)"""
        return tuple(v[min(i, len(v) - 1)] % Q for i in range(self.deg))

    def rand(self, rng):
        return tuple(rand_fq(rng) for _ in range(self.deg))

    def rand_nonzero(self, rng):
        while True:
            v = self.rand(rng)
            if v != self.zero:
                return v


G1 = Curve("g1", 1)
G2 = Curve("g2", 2)
CURVES = {"g1": G1, "g2": G2}


# ---- the group law on affine pairs (None = infinity) ---------------------------------------------------------------------------------
def law_add(cv: Curve, P, S):
    if P is None:
        return S
    if S is None:
        return P
    (x1, y1), (x2, y2) = P, S
    if x1 == x2:
        if y1 != y2 or y1 == cv.zero:
            return None
        lam = cv.div(cv.smul(cv.mul(x1, x1), 3), cv.smul(y1, 2))
    else:
        lam = cv.div(cv.sub(y2, y1), cv.sub(x2, x1))
    x3 = cv.sub(cv.sub(cv.mul(lam, lam), x1), x2)
    return (x3, cv.sub(cv.mul(lam, cv.sub(x1, x3)), y1))


def law_neg(cv: Curve, P):
    return None if P is None else (P[0], cv.neg(P[1]))


# ---- operands ---------------------------------------------------------------------------------------------------------------------------
def inf_op(cv: Curve):
    return (cv.zero,) * 4


def raw(cv: Curve, X, Y, z):
    """the operand with STORED coordinates X, Y and ZZ, ZZZ from z: it stands for the pair (X / z^2, Y / z^3) / 2^390"""
    z2 = cv.mul(z, z)
    return (X, Y, cv.smul(z2, RADIX), cv.smul(cv.mul(z2, z), RADIX))


def scale(cv: Curve, P, z):
    """the true affine pair P as an XYZZ operand with the given z (P = None: infinity)"""
    if P is None:
        return inf_op(cv)
    z2 = cv.mul(z, z)
    return raw(cv, cv.smul(cv.mul(P[0], z2), RADIX), cv.smul(cv.mul(P[1], cv.mul(z2, z)), RADIX), z)


def is_inf(cv: Curve, op) -> bool:
    return op[2] == cv.zero


def point(cv: Curve, op):
    """the affine pair an XYZZ operand (residues) stands for; the Montgomery radix cancels in X / ZZ and Y / ZZZ"""
    if is_inf(cv, op):
        return None
    return (cv.div(op[0], op[2]), cv.div(op[1], op[3]))


def affine_point(cv: Curve, op):
    """the pair the AFFINE operand (op.X, op.Y) stands for (x = y = 0: infinity)"""
    if op[0] == cv.zero and op[1] == cv.zero:
        return None
    return (cv.smul(op[0], RADIX_INV), cv.smul(op[1], RADIX_INV))


def consistent(cv: Curve, op) -> bool:
    """ZZ^3 == ZZZ^2 on the values the stored coordinates stand for"""
    zz, zzz = cv.smul(op[2], RADIX_INV), cv.smul(op[3], RADIX_INV)
    return cv.mul(cv.mul(zz, zz), zz) == cv.mul(zzz, zzz)


# named intermediates of the device's mixed addition (residues): what the engineered cases are solved for
def madd_u2(cv, a, b):
    return cv.smul(cv.mul(b[0], a[2]), RADIX_INV)


def madd_s2(cv, a, b):
    return cv.smul(cv.mul(b[1], a[3]), RADIX_INV)


def madd_q(cv, a, b):
    p = cv.sub(madd_u2(cv, a, b), a[0])
    pp = cv.smul(cv.mul(p, p), RADIX_INV)
    return cv.smul(cv.mul(a[0], pp), RADIX_INV)


Case = namedtuple("Case", "tag kind a la b lb rep")  # kind: ord | inf | same;  b, lb = None for the unary modes;  la, lb: 4 x deg lifts


def expected(cv: Curve, mode: str, c: Case):
    if mode == "madd":
        return law_add(cv, point(cv, c.a), affine_point(cv, c.b))
    if mode == "madd_neg":
        return law_add(cv, point(cv, c.a), law_neg(cv, affine_point(cv, c.b)))
    if mode in ("add", "add_quad"):
        return law_add(cv, point(cv, c.a), point(cv, c.b))
    if mode == "dbl":
        P = point(cv, c.a)
        return law_add(cv, P, P)
    if mode == "dbl_affine":
        P = affine_point(cv, c.a)
        return law_add(cv, P, P)
    assert mode == "acc_quad"
    acc, B = point(cv, c.a), point(cv, c.b)
    for _ in range(c.rep):
        acc = law_add(cv, acc, B)
    return acc


def values(cv: Curve, op, lift) -> List[int]:
    """the exact integers the device works on, 4 * deg of them"""
    return [r + k * Q for co, lf in zip(op, lift) for r, k in zip(co, lf)]


def check_result(cv: Curve, limbs, want) -> Optional[str]:
    """limbs: [4 * deg][13] raw limbs of a device result; want: the reference pair or None.  Returns None or what is wrong."""
    ints = [limbs_to_int(l) for l in limbs]
    for k, l in enumerate(limbs):
        if any(int(x) >> 30 for x in l[:12]):
            return f"component {k}: a limb of 0..11 is not below 2^30"
    if want is None:
        return None if not any(ints) else "infinity expected: every limb of the four coordinates must be zero"
    for k, v in enumerate(ints):
        if v >= BOUND[k // cv.deg] * Q:
            return f"component {k} = {v / Q:.3f} q is outside its bound {BOUND[k // cv.deg]} q"
    op = tuple(tuple(v % Q for v in ints[cv.deg * c : cv.deg * (c + 1)]) for c in range(4))
    if is_inf(cv, op):
        return "ZZ = 0 (mod q) on a finite result"
    if not consistent(cv, op):
        return "ZZ^3 != ZZZ^2"
    if point(cv, op) != want:
        return "decodes to another point"
    return None


def split(cv: Curve, limbs):
    """a raw device result as (operand of residues, lifts): v = (v mod q) + (v // q) q, to feed it back in"""
    ints = [limbs_to_int(l) for l in limbs]
    op = tuple(tuple(v % Q for v in ints[cv.deg * c : cv.deg * (c + 1)]) for c in range(4))
    lf = tuple(tuple(v // Q for v in ints[cv.deg * c : cv.deg * (c + 1)]) for c in range(4))
    return op, lf


# ---- lifts ------------------------------------------------------------------------------------------------------------------------------
def lifts(cv: Curve, op, variant: str, rng):
    """4 x deg lifts; an infinite operand keeps lift 0 everywhere (ZZ = 0 with lift 0 is the encoding, and infinity is all-zero limbs)"""
    if is_inf(cv, op) or variant == "zero":
        return ((0,) * cv.deg,) * 4
    if variant == "max":
        return tuple((m,) * cv.deg for m in LIFT_MAX)
    return tuple(tuple(rng.next() % (m + 1) for _ in range(cv.deg)) for m in LIFT_MAX)


ZERO_LIFT = {1: ((0,),) * 4, 2: ((0, 0),) * 4}


# ---- points -----------------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def curve_points(name: str, n: int) -> tuple:
    """true affine points ON the curve: G1 from helpers.synthetic_bases, G2 multiples of the generator as tests/test_gpu_g2.py builds them"""
    if name == "g1":
        from helpers import pt_ints, synthetic_bases

        bases, _ = synthetic_bases(n, 77)
        return tuple(((p[0],), (p[1],)) for p in (pt_ints(b) for b in bases))
    rng = po.SplitMix64(78)
    cur, step = po.g2_mul(po.G2_GEN, rng.fr()), po.g2_mul(po.G2_GEN, rng.fr())
    out = []
    for _ in range(n):
        out.append(cur)
        cur = po.g2_add(cur, step)
    return tuple(out)


def _extreme_elems(cv: Curve, nonzero: bool = False):
    """field elements whose components are the edge residues (G2: every edge in c0 against a rotating edge in c1)"""
    E = [e for e in EXTREMES if not (nonzero and e == 0)]
    if cv.deg == 1:
        return [(e,) for e in E]
    return [(e, E[(i * 3 + 1) % len(E)]) for i, e in enumerate(E)] + [(0, e) for e in E[1:4]] + ([] if nonzero else [(0, 0)])


# ---- base cases: (tag, kind, a, b) -----------------------------------------------------------------------------------------------------
def _binary_bases(cv: Curve, affine_b: bool):
    """pairs for madd / add / the quad forms.  affine_b: b is used as the affine operand (b.X, b.Y), so its z is 1."""
    rng = po.SplitMix64(1000 + cv.deg + (10 if affine_b else 0))
    zb = (lambda: cv.one) if affine_b else (lambda: cv.rand_nonzero(rng))
    out = []
    # 1. curve points, scaled by random z
    pts = curve_points(cv.name, 24)
    for i in range(0, 24, 2):
        out.append((f"curve{i}", "ord", scale(cv, pts[i], cv.rand_nonzero(rng)), scale(cv, pts[i + 1], zb())))
    # 2. off-curve pairs with extreme stored residues
    E = _extreme_elems(cv)
    for i in range(len(E)):
        for j in range(0, len(E), 3):
            X1, Y1, X2, Y2 = E[i], E[(i + j) % len(E)], E[(i + 2 * j + 1) % len(E)], E[(2 * i + j + 3) % len(E)]
            if affine_b and X2 == cv.zero and Y2 == cv.zero:
                Y2 = cv.one  # (0, 0) is the affine encoding of infinity: that is class 4
            out.append((f"extreme{i}.{j}", "ord", raw(cv, X1, Y1, cv.rand_nonzero(rng)), raw(cv, X2, Y2, zb())))
    # 3. engineered intermediates of the mixed addition, solved backwards through the Montgomery radix.  b has z = 1, so the full
    #    addition sees the same U2, S2, Q (its U1 is X1).  The "max" lift variant puts X1 = x + 7q, Y1 = y + 3q at the top of their bands.
    for tag, a, b, _ in engineered(cv):
        out.append((tag, "ord", a, b))
    # 4. degenerate pairs
    offc = [(cv.elem(Q - 1, 5), cv.elem(Q - 2, 1)), (cv.elem(1, R390), cv.elem(Q - 1, Q - 1)), (cv.rand(rng), cv.rand_nonzero(rng))]
    for i, P in enumerate(list(pts[:5]) + offc):
        za = cv.rand_nonzero(rng)
        A = scale(cv, P, za)
        out.append((f"double{i}", "same", A, scale(cv, P, zb())))  # the same point, another z: doubling (madd_neg: cancellation)
        out.append((f"cancel{i}", "same", A, scale(cv, law_neg(cv, P), zb())))  # opposite points, another z
        if not affine_b:
            out.append((f"cancel_band{i}", "same", A, (A[0], cv.neg(A[1]), A[2], A[3])))  # Y negated in place: k q - Y inside the band
        out.append((f"a_inf{i}", "inf", inf_op(cv), scale(cv, P, zb())))
        out.append((f"b_inf{i}", "inf", A, inf_op(cv)))
    out.append(("both_inf", "inf", inf_op(cv), inf_op(cv)))
    return out


def engineered(cv: Curve):
    """(tag, a, b, claim): claim = (name of the intermediate, its residue).  b always has z = 1."""
    rng = po.SplitMix64(2000 + cv.deg)
    out = []
    small = [cv.elem(5, 7), cv.elem((1 << 300) + 3, 2), cv.elem(1, 0), cv.elem(0, 9) if cv.deg == 2 else cv.elem(2)]
    top = [cv.elem(Q - 1), cv.elem(Q - 1, 3)] if cv.deg == 2 else [cv.elem(Q - 1)]
    y_top = [cv.elem(Q - 1), cv.elem(Q - (1 << 30)), cv.elem(Q - 1, Q - (1 << 30))][: 2 + (cv.deg - 1)]
    x_top = [cv.elem(Q - 1), cv.elem(Q - 2, Q - 1)][: cv.deg]
    for yi, Y1 in enumerate(y_top):
        for si, s in enumerate(small + top + [cv.zero]):  # S2 = s; s = 0 is b.Y = 0, where the device's S2 is zero in every limb
            a = raw(cv, x_top[(yi + si) % len(x_top)], Y1, cv.rand_nonzero(rng))
            bY = cv.div(cv.smul(s, RADIX), a[3])
            out.append((f"S2.{yi}.{si}", a, raw(cv, cv.rand_nonzero(rng), bY, cv.one), ("S2", s)))
    for xi, X1 in enumerate(x_top):
        for ui, u in enumerate(small + [cv.zero]):  # U2 = u small against X1 at the top
            a = raw(cv, X1, y_top[(xi + ui) % len(y_top)], cv.rand_nonzero(rng))
            bX = cv.div(cv.smul(u, RADIX), a[2])
            out.append((f"U2.{xi}.{ui}", a, raw(cv, bX, cv.rand_nonzero(rng), cv.one), ("U2", u)))
    for ti, t in enumerate(small + top):  # Q = t: X1 = t 2^780 / P^2 for a chosen P = U2 - X1, against whatever X3 comes out (large for small Q)
        for Y1 in y_top[:2]:
            p = cv.rand_nonzero(rng)
            X1 = cv.div(cv.smul(t, RADIX * RADIX), cv.mul(p, p))
            a = raw(cv, X1, Y1, cv.rand_nonzero(rng))
            bX = cv.div(cv.smul(cv.add(X1, p), RADIX), a[2])
            out.append((f"Q.{ti}", a, raw(cv, bX, cv.rand_nonzero(rng), cv.one), ("Q", t)))
    return out


def _unary_bases(cv: Curve, affine: bool):
    """operands for dbl (XYZZ, infinity included) and dbl_affine (X, Y only: z = 1, no infinity).  Y = 0 (mod q) is left out: such a
    point has order 2, neither group has one, and the doubling formulas do not claim to detect it."""
    rng = po.SplitMix64(3000 + cv.deg + (10 if affine else 0))
    z = (lambda: cv.one) if affine else (lambda: cv.rand_nonzero(rng))
    out = [(f"curve{i}", "same", scale(cv, P, z()), None) for i, P in enumerate(curve_points(cv.name, 24)[:12])]
    E, EY = _extreme_elems(cv), _extreme_elems(cv, nonzero=True)
    for i in range(len(E)):
        for j in range(0, len(EY), 2):
            Y = EY[(i + j) % len(EY)]
            if Y != cv.zero:
                out.append((f"extreme{i}.{j}", "same", raw(cv, E[i], Y, z()), None))
    if not affine:
        out.append(("inf", "inf", inf_op(cv), None))
    return out


def _with_lifts(cv: Curve, bases, affine_b: bool, seed: int) -> List[Case]:
    """every base case under all-zero, all-maximal and mixed lifts (the affine operand of madd keeps lift 0)"""
    rng = po.SplitMix64(seed)
    out = []
    for variant in VARIANTS:
        for tag, kind, a, b in bases:
            lb = None if b is None else (ZERO_LIFT[cv.deg] if affine_b else lifts(cv, b, variant, rng))
            out.append(Case(f"{tag}/{variant}", kind, a, lifts(cv, a, variant, rng), b, lb, 1))
    return out


def _quad_order(cases: Sequence[Case]) -> List[Case]:
    """neighbouring elements (= neighbouring quads of one wave) alternate between ordinary, infinite-operand and same-x cases; the
    shorter pools repeat until every case of the longest has run.  rep cycles 1, 2, 3 out of step with the kinds."""
    pools = [[c for c in cases if c.kind == k] for k in ("ord", "inf", "same")]
    assert all(pools)
    out = []
    for i in range(3 * max(len(p) for p in pools)):
        p = pools[i % 3]
        out.append(p[(i // 3) % len(p)]._replace(rep=1 + (i + i // 3) % 3))
    if len(out) % 64 == 0:
        out.append(out[0])
    return out


@lru_cache(maxsize=None)
def cases(name: str, mode: str) -> Tuple[Case, ...]:
    """the full list of one curve and mode; the GPU test runs all of it"""
    cv = CURVES[name]
    if mode in UNARY:
        return tuple(_with_lifts(cv, _unary_bases(cv, mode == "dbl_affine"), False, 41))
    affine_b = mode in ("madd", "madd_neg")
    cs = _with_lifts(cv, _binary_bases(cv, affine_b), affine_b, 42)
    return tuple(_quad_order(cs) if mode in ("add_quad", "acc_quad") else cs)


# ---- packing for the hooks ------------------------------------------------------------------------------------------------------------
def pack_ops(cv: Curve, ops):
    """operands -> [n, 4 * deg * 6] u64 (48-byte little-endian integers)"""
    import numpy as np

    flat = [(v >> (64 * k)) & po.MASK64 for op in ops for co in op for v in co for k in range(6)]
    return np.array(flat, dtype=np.uint64).reshape(len(ops), 24 * cv.deg)


def pack_lifts(cv: Curve, lfs):
    """lifts -> [n] u32, one nibble per coordinate (per component) from bit 0 up"""
    import numpy as np

    return np.array([sum(k << (4 * i) for i, k in enumerate(k for co in lf for k in co)) for lf in lfs], dtype=np.uint32)
