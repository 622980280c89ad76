"""
The field tower under the device pairing, one operation at a time (test hooks zk_dbg_fq30_op / zk_dbg_fq12_op of
include/zkhip_test.h) against tests/pairing_tower_model.py.  Everything is bit-exact.

  * Fq30 (csrc/fq30.cuh): the conditional subtractions and reductions at every threshold k q - 1, k q, k q + 1 their contracts
    allow, the subtractions a + K q - b with b at K q - 1 and at 0, the additions, and the three Montgomery multipliers and the
    inversion with operands at the top of their contracts (a = x + 15 q).  The reductions, subtractions and additions are compared
    as INTEGERS (rebuilt from the 13 raw limbs); the products by residue, result < 2q and normalised limbs.
  * Fq2 / Fq6 / Fq12 (curve30_g2.cuh, fq12.cuh) and f12_exp_by_x / final_exp of zk_pairing.hip against zkhip.pairing.Fq12 (another
    representation: Fq[w] / (w^12 - 2 w^6 + 2)), each at three lift patterns: inputs as converted (< q), every component + q (the
    largest representative the tower's bound rule allows, < 2q), and a random mask per element.  On EVERY output both flags must be
    set: limbs normalised, and every component of the value the function returned below 2q -- the bound rule itself, which a
    too-weak reduction breaks long before a value goes wrong.
"""
import functools

import numpy as np
import pytest

import pairing_tower_model as tm
import pyoracle as po
from zkhip import pairing as pr

pytestmark = pytest.mark.gpu

Q = tm.Q
LIFT_ALL = 0xFFFFFF
ONE_WORDS = tm.to_words(pr.Fq12.one())


# ---- plumbing ------------------------------------------------------------------------------------------------------------------------
def _fq_bytes(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(48, "little") for v in vals), dtype=np.uint8).reshape(-1, 48)


def run30(ctx, mode, a, b=None):
    """a, b: lists of (x < q, k <= 15) standing for x + k q -> (the result integers, flags)"""
    n = len(a)
    dx, dkx = ctx.to_device(_fq_bytes([x for x, _ in a])), ctx.to_device(np.array([k for _, k in a], dtype=np.uint32))
    dy = dky = None
    if b is not None:
        assert len(b) == n
        dy, dky = ctx.to_device(_fq_bytes([y for y, _ in b])), ctx.to_device(np.array([k for _, k in b], dtype=np.uint32))
    limbs, flags = ctx.dbg_fq30(mode, dx, dkx, dy, dky, n)
    return [tm.limbs_to_int(row) for row in limbs], flags


def words_of(comps_list):
    return np.array([tm.comps_to_words(c) for c in comps_list], dtype=np.uint64).reshape(-1, 72)


def model_words(fs):
    return np.array([tm.to_words(f) for f in fs], dtype=np.uint64).reshape(-1, 72)


def run12(ctx, mode, A, B, lift):
    """A, B: [n, 72] u64 ark words (B None for unary modes); lift: [n] u32 -> (out [n, 72], flags [n])"""
    n = len(A)
    return ctx.dbg_fq12(mode, ctx.to_device(A), None if B is None else ctx.to_device(B), ctx.to_device(np.asarray(lift, dtype=np.uint32)), n)


def lift_patterns(n, seed):
    rng = po.SplitMix64(seed)
    return {
        "none": np.zeros(n, dtype=np.uint32),
        "all": np.full(n, LIFT_ALL, dtype=np.uint32),
        "random": np.array([rng.next() & LIFT_ALL for _ in range(n)], dtype=np.uint32),
    }


def check12(ctx, mode, A, B, want, seed, what=""):
    """the device at the three lift patterns == want, with both flags set on every output"""
    for name, lift in lift_patterns(len(A), seed).items():
        got, flags = run12(ctx, mode, A, B, lift)
        bad = np.nonzero(flags != 3)[0]
        assert len(bad) == 0, f"{mode}{what} lift={name}: flags {flags[bad[0]]} at element {bad[0]} ({len(bad)} elements): " \
                              "bit 0 = limbs normalised, bit 1 = every component < 2q"
        diff = np.nonzero((got != want).any(axis=1))[0]
        assert len(diff) == 0, f"{mode}{what} lift={name}: value differs at element {diff[0]} ({len(diff)} elements)"


# ---- inputs, built once ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def fq_edge_values():
    """x < q: the edges (with k they give k q - 1, k q, k q + 1 and limbs of all ones / all zeros) and 200 random"""
    rng = po.SplitMix64(0xF930)
    return [0, 1, (1 << 30) - 1, 1 << 30, Q - (1 << 30), Q - 1, (1 << 360) - 1, (1 << 380) - 1] + [tm.rand_fq(rng) for _ in range(200)]


@functools.lru_cache(None)
def tower_set():
    """252 elements (no multiple of the workgroup's 64 lanes) as comps: 200 random, 0, 1, -1, the 12 unit vectors of the tower basis,
    the 12 monomials w^e of the model's basis, all components q - 1, and one non-zero component (random, and q - 1) at each place"""
    rng = po.SplitMix64(0x70E7)
    s = [[tm.rand_fq(rng) for _ in range(12)] for _ in range(200)]
    s += [[0] * 12, [1] + [0] * 11, [Q - 1] + [0] * 11]
    s += [[1 if k == j else 0 for k in range(12)] for j in range(12)]
    s += [tm.to_comps(pr.W**e) for e in range(12)]
    s += [[Q - 1] * 12]
    s += [[tm.rand_fq(rng) if k == j else 0 for k in range(12)] for j in range(12)]
    s += [[Q - 1 if k == j else 0 for k in range(12)] for j in range(12)]
    return s


@functools.lru_cache(None)
def tower_inputs():
    """(comps, words A, model elements, the partner list B = A reversed: specials meet randoms, the middle meets itself)"""
    comps = tower_set()
    A = words_of(comps)
    fa = [tm.from_comps(c) for c in comps]
    return comps, A, fa, A[::-1].copy(), fa[::-1]


@functools.lru_cache(None)
def cyclotomic():
    rng = po.SplitMix64(0xC7C1)
    seeds = [pr.Fq12([tm.rand_fq(rng) for _ in range(12)]) for _ in range(2)]
    return tm.cyclotomic_elements(seeds)


# ---- Fq30: reductions at every threshold -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", list(tm.REDUCTIONS))
def test_fq30_reductions_at_every_threshold(ctx, mode):
    fn, kmax = tm.REDUCTIONS[mode]
    a = [(x, k) for k in range(kmax + 1) for x in fq_edge_values()]
    got, flags = run30(ctx, mode, a)
    assert (flags & 1).all(), mode
    for (x, k), g in zip(a, got):
        assert g == fn(x + k * Q), (mode, hex(x), k)


@pytest.mark.parametrize("K", [2, 4, 6, 8, 12])
def test_fq30_subtractions(ctx, K):
    """a + K q - b as an integer: b at K q - 1 and at 0 with a at 0 and at its largest (the result stays below 16q), b over the edge
    values at every k below K, random pairs"""
    rng = po.SplitMix64(0x5B00 + K)
    top = (Q - 1, 15 - K)
    a, b = [], []
    for bb in ((Q - 1, K - 1), (0, 0)):
        for aa in ((0, 0), top, (tm.rand_fq(rng), 0)):
            a.append(aa)
            b.append(bb)
    for ky in range(K):
        for y in fq_edge_values():
            a.append((tm.rand_fq(rng), rng.next() % (16 - K)))
            b.append((y, ky))
    for x in fq_edge_values():
        a.append((x, rng.next() % (16 - K)))
        b.append((tm.rand_fq(rng), rng.next() % K))
    got, flags = run30(ctx, f"sub{K}", a, b)
    assert (flags & 1).all()
    for (x, kx), (y, ky), g in zip(a, b, got):
        assert g == tm.sub_k(K, x + kx * Q, y + ky * Q), (K, hex(x), kx, hex(y), ky)


def test_fq30_additions(ctx):
    rng = po.SplitMix64(0xADD)
    ev = fq_edge_values()
    # add: a + b below 16q
    a = [(Q - 1, 7), (Q - 1, 14), (Q - 1, 0), (0, 0), (0, 15)]
    b = [(Q - 1, 7), (Q - 1, 0), (Q - 1, 14), (0, 0), (0, 0)]
    for x in ev:
        kx = rng.next() % 15
        a.append((x, kx))
        b.append((ev[rng.next() % len(ev)], rng.next() % (15 - kx)))
    got, flags = run30(ctx, "add", a, b)
    assert (flags & 1).all()
    for (x, kx), (y, ky), g in zip(a, b, got):
        assert g == x + kx * Q + y + ky * Q, ("add", hex(x), kx, hex(y), ky)
    # add2x: a + 2 b below 16q
    a = [(Q - 1, 13), (Q - 1, 1), (Q - 1, 3), (0, 0), ((1 << 30) - 1, 0)]
    b = [(Q - 1, 0), (Q - 1, 6), (Q - 1, 5), (0, 0), ((1 << 360) - 1, 6)]
    for x in ev:
        ky = rng.next() % 7
        a.append((x, rng.next() % (14 - 2 * ky)))
        b.append((ev[rng.next() % len(ev)], ky))
    got, flags = run30(ctx, "add2x", a, b)
    assert (flags & 1).all()
    for (x, kx), (y, ky), g in zip(a, b, got):
        assert g == x + kx * Q + 2 * (y + ky * Q), ("add2x", hex(x), kx, hex(y), ky)


def test_fq30_products_at_the_top_of_their_contracts(ctx):
    """mul / sqr with both operands x + 15 q (16 * 16 = 256), mul2add with bounds 8 and 16 in each product (128 + 128): the residue,
    result < 2q, limbs normalised"""
    rng = po.SplitMix64(0x3017)
    ev = fq_edge_values()
    tops = [Q - 1, Q - (1 << 30)] + [tm.rand_fq(rng) for _ in range(6)]
    pairs = [(x, y) for x in tops for y in tops] + [(x, ev[(i * 7 + 3) % len(ev)]) for i, x in enumerate(ev)]
    for mode, kx, ky in (("mul", 15, 15), ("mul", 0, 0), ("mul", 15, 0), ("sqr", 15, None), ("sqr", 0, None), ("mul2add", 7, 15),
                         ("mul2add", 15, 7), ("mul2add", 0, 0)):
        a = [(x, kx) for x, _ in pairs]
        b = None if ky is None else [(y, ky) for _, y in pairs]
        got, flags = run30(ctx, mode, a, b)
        assert (flags & 1).all(), mode
        for i, ((x, y), g) in enumerate(zip(pairs, got)):
            av = x + kx * Q
            want = tm.mont_mul_residue(av, av) if mode == "sqr" else tm.mont_mul_residue(av, y + ky * Q) * (2 if mode == "mul2add" else 1) % Q
            assert g % Q == want and g < 2 * Q, (mode, kx, ky, i, g // Q)


def test_fq30_inversion(ctx):
    """0 -> 0, 1, q - 1, random values, every representative x + k q up to 15 q"""
    rng = po.SplitMix64(0x1F7)
    xs = [0, 1, Q - 1, 2, (1 << 30) - 1] + [tm.rand_fq(rng) for _ in range(36)]
    a = [(x, k) for k in range(16) for x in xs]
    got, flags = run30(ctx, "inv", a)
    assert (flags & 1).all()
    for (x, k), g in zip(a, got):
        assert g % Q == tm.mont_inv_residue(x) and g < 2 * Q, (hex(x), k)
        if x == 0 and k == 0:
            assert g == 0


# ---- the tower: every operation at three lift patterns -----------------------------------------------------------------------------------
def _f6(c):
    return tm.embed_fq6(c[:6])


def _f2(c):
    return tm.embed_fq2(c[0], c[1])


TOWER_OPS = {
    # mode: (binary, model on (comps a, element a, comps b, element b))
    "mul": (True, lambda ca, fa, cb, fb: fa * fb),
    "sqr": (False, lambda ca, fa, cb, fb: fa * fa),
    "conj": (False, lambda ca, fa, cb, fb: tm.conj(fa)),
    "inv": (False, lambda ca, fa, cb, fb: tm.inv0(fa)),
    "frob1": (False, lambda ca, fa, cb, fb: tm.frob(fa, 1)),
    "frob2": (False, lambda ca, fa, cb, fb: tm.frob(fa, 2)),
    "frob3": (False, lambda ca, fa, cb, fb: tm.frob(fa, 3)),
    "f6_mul": (True, lambda ca, fa, cb, fb: _f6(ca) * _f6(cb)),
    "f6_inv": (False, lambda ca, fa, cb, fb: tm.inv0(_f6(ca))),
    "f2_mul": (True, lambda ca, fa, cb, fb: _f2(ca) * _f2(cb)),
    "f2_sqr": (False, lambda ca, fa, cb, fb: _f2(ca) * _f2(ca)),
    "f2_inv": (False, lambda ca, fa, cb, fb: tm.inv0(_f2(ca))),
}


@pytest.mark.parametrize("mode", list(TOWER_OPS))
def test_tower_operation(ctx, mode):
    """the whole input set (the model's Euclidean inverse included: 252 inversions take about 0.3 s)"""
    comps, A, fa, B, fb = tower_inputs()
    binary, model = TOWER_OPS[mode]
    want = model_words([model(ca, a, cb, b) for ca, a, cb, b in zip(comps, fa, comps[::-1], fb)])
    check12(ctx, mode, A, B if binary else None, want, seed=0x11F7 + len(mode))
    if mode in ("inv", "f6_inv", "f2_inv"):  # 0 -> 0 (element 200 is zero)
        assert not any(comps[200]) and not want[200].any()


def test_tower_tail_sizes(ctx):
    """1 and 65 lanes: the first and the second workgroup's tails"""
    comps, A, fa, B, fb = tower_inputs()
    want = model_words([a * b for a, b in zip(fa[:65], fb[:65])])
    for n in (1, 65):
        check12(ctx, "mul", A[:n].copy(), B[:n].copy(), want[:n], seed=n, what=f" n={n}")


def test_frobenius_orbits(ctx):
    """frobK applied 12 / gcd(12, K) times is the identity (a second route, without the model); flags at every step"""
    _, A, _, _, _ = tower_inputs()
    X = np.concatenate([A[:41], A[200:224]])  # 65 elements
    for K, steps in ((1, 12), (2, 6), (3, 4)):
        lifts = lift_patterns(len(X), 0xF0B + K)
        cur = X
        for s in range(steps):
            cur, flags = run12(ctx, f"frob{K}", cur, None, lifts[("none", "all", "random")[s % 3]])
            assert (flags == 3).all(), (K, s)
            if s + 1 < steps:
                assert (cur != X).any(axis=1)[:41].all(), (K, s)  # the random elements have the full orbit
        assert (cur == X).all(), K


# ---- cyclotomic squaring, x-power, final exponentiation ---------------------------------------------------------------------------------
def test_cyclotomic_squaring(ctx):
    """cyc_sqr == sqr == the model's square on cyclotomic elements (1, two easy-part values, their conjugates, squares and products),
    and != sqr outside the subgroup: on -1 and -c (unitary, but of even order) and on a random element"""
    cyc = cyclotomic()
    A = model_words(cyc)
    want = model_words([c * c for c in cyc])
    check12(ctx, "cyc_sqr", A, None, want, seed=0xC5)
    check12(ctx, "sqr", A, None, want, seed=0xC6)
    outside = tm.unitary_outside(cyc) + [tm.from_comps(tower_set()[0])]
    O = model_words(outside)
    zero = np.zeros(len(O), dtype=np.uint32)
    gs, _ = run12(ctx, "cyc_sqr", O, None, zero)
    sq, flags = run12(ctx, "sqr", O, None, zero)
    assert (flags == 3).all() and (sq == model_words([o * o for o in outside])).all()
    assert (gs != sq).any(axis=1).all(), "cyc_sqr agrees with sqr outside the cyclotomic subgroup: it is not the Granger-Scott squaring"


def test_exp_by_x(ctx):
    cyc = cyclotomic()
    check12(ctx, "exp_by_x", model_words(cyc), None, model_words([tm.exp_by_x(c) for c in cyc]), seed=0xE8)


def test_final_exp(ctx):
    """0 -> 0, 1 -> 1, Fq6 and Fq2 elements -> 1 (killed by q^6 - 1), and two random elements against the model's single power
    (about half a second each)"""
    comps = tower_set()
    f6 = comps[3][:6] + [0] * 6
    f2 = comps[4][:2] + [0] * 10
    A = words_of([[0] * 12, [1] + [0] * 11, f6, f2, comps[0], comps[1]])
    want = np.array([[0] * 72, ONE_WORDS, ONE_WORDS, ONE_WORDS] + [tm.to_words(tm.final_exp(tm.from_comps(c))) for c in comps[:2]], dtype=np.uint64)
    assert not (want[4] == want[0]).all() and not (want[4] == want[1]).all()
    check12(ctx, "final_exp", A, None, want, seed=0xFE)


# ---- the sparse line product --------------------------------------------------------------------------------------------------------------
def test_mul_by_014(ctx):
    """== the dense product by the embedded line == the model; lines with c0 = 0, c1 = 0, c4 = 0, two of the three zero, all zero, all
    components q - 1 (lifted to 2q - 1 by the 'all' pattern), and random ones"""
    comps, A, fa, _, _ = tower_inputs()
    rng = po.SplitMix64(0x014)
    r2 = lambda: (tm.rand_fq(rng), tm.rand_fq(rng))
    z, m = (0, 0), (Q - 1, Q - 1)
    lines = []
    for i in range(len(comps)):
        special = [(z, r2(), r2()), (r2(), z, r2()), (r2(), r2(), z), (z, z, r2()), (z, r2(), z), (r2(), z, z), (z, z, z), (m, m, m),
                   ((1, 0), z, z), ((0, Q - 1), (Q - 1, 0), (0, 1))]
        lines.append(special[i % 16] if i % 16 < len(special) else (r2(), r2(), r2()))
    lc = [tm.line_comps(*l) for l in lines]
    B = words_of(lc)
    want = model_words([a * tm.from_comps(c) for a, c in zip(fa, lc)])
    check12(ctx, "mul_by_014", A, B, want, seed=0x140)
    check12(ctx, "mul", A, B, want, seed=0x141, what=" (dense, by the line)")
    # the slots outside c0.c0, c0.c1, c1.c1 of the line operand are not read
    noisy = B.copy().reshape(-1, 12, 6)
    noisy[:, [4, 5, 6, 7, 10, 11]] = A.reshape(-1, 12, 6)[:, [4, 5, 6, 7, 10, 11]]
    check12(ctx, "mul_by_014", A, noisy.reshape(-1, 72), want, seed=0x142, what=" (other slots filled)")


# ---- chains ----------------------------------------------------------------------------------------------------------------------------------
def test_chain_of_50_operations(ctx):
    """mul / sqr / frob1 / conj in turn, 50 steps, every output fed back in, a fresh random lift at every step: the flags at every step
    (a representative that creeps upward shows there), the value against the model at the end"""
    comps, A, fa, B, fb = tower_inputs()
    idx = list(range(41)) + list(range(200, 224))  # 65 elements
    cur, Bk = A[idx].copy(), B[idx].copy()
    want, fbk = [fa[i] for i in idx], [fb[i] for i in idx]
    rng = po.SplitMix64(0xC4A1)
    for s in range(50):
        mode = ("mul", "sqr", "frob1", "conj")[s % 4]
        lift = np.array([rng.next() & LIFT_ALL for _ in idx], dtype=np.uint32) if s % 5 else np.full(len(idx), LIFT_ALL, dtype=np.uint32)
        cur, flags = run12(ctx, mode, cur, Bk if mode == "mul" else None, lift)
        assert (flags == 3).all(), (s, mode, flags[np.nonzero(flags != 3)[0][0]])
        want = [{"mul": lambda w, b: w * b, "sqr": lambda w, b: w * w, "frob1": lambda w, b: tm.frob(w, 1), "conj": lambda w, b: tm.conj(w)}[mode](w, b)
                for w, b in zip(want, fbk)]
    assert (cur == model_words(want)).all()
