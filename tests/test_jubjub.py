"""
Jubjub and "zkhip-schnorr-v1" without a GPU: the constants (G by the rule, [l] G = O, l prime, d a non-square), zkhip.jubjub's host rules
against the independent model (jubjub_model.py) on the edge points and edge scalars, signatures and each corruption's status, the gadgets on
the wires of the witness model (advice_model.py), Builder.to_bits_strict refusing the bits of x + r, and the Schnorr circuit.
"""
import random

import pytest

import advice_model as am
import jubjub_model as jm
from zkhip import jubjub as jj
from zkhip.circuit import Builder, circuit_digest

R, L = jm.R, jm.L


def is_prime(n: int) -> bool:
    """Miller-Rabin on 24 fixed bases (deterministic for this test's two inputs in the sense that a composite would have to fool all)"""
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83, 89):
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


# ---- constants ----
def test_constants():
    assert jj.D == jm.D == (-10240 * pow(10241, -1, R)) % R and jj.L == L
    assert pow(jj.D, (R - 1) // 2, R) == R - 1, "d is a non-square"
    assert is_prime(L) and L.bit_length() == 252
    y, G = jj.generator_by_rule()
    assert y == 3 and G == jj.G == jm.G
    assert jm.mul(L, jj.G) == (0, 1) and jj.mul_host(L, jj.G) == (0, 1)


def test_device_constants_are_the_montgomery_forms():
    """the limbs csrc/zk_jubjub.hip holds for 2d, G.x, G.y, G.x G.y and l, re-derived from the integers"""
    import os
    import re

    text = open(os.path.join(os.path.dirname(os.path.abspath(jj.__file__)), "..", "csrc", "zk_jubjub.hip")).read()
    mont = lambda v: (v << 256) % R
    want = {"D2": mont(2 * jm.D % R), "GX": mont(jm.G[0]), "GY": mont(jm.G[1]), "GT": mont(jm.G[0] * jm.G[1] % R), "L": L}
    for name, v in want.items():
        m = re.search(r"constexpr u32 %s\(int i\) \{[^\n]*\n\s*constexpr u32 t\[8\] = \{([^}]*)\}" % name, text)
        limbs = [int(w.strip().rstrip("u"), 16) for w in m.group(1).split(",")]
        assert sum(l << (32 * i) for i, l in enumerate(limbs)) == v, name


# ---- host rules against the model ----
def test_host_rules_equal_the_model():
    pts = jm.case_points()
    for P in pts:
        assert jj.on_curve_host(P) and jm.on_curve(P)
        assert jj.in_subgroup_host(P) == jm.in_subgroup(P)
        assert jj.neg_host(P) == jm.neg(P)
        for Q in pts:
            assert jj.add_host(P, Q) == jm.add(P, Q)
    for i, P in enumerate(pts):
        for k in jm.SCALARS[i % 3::3] + [L]:
            assert jj.mul_host(k, P) == jm.cached_mul(k, P)
    for k in jm.SCALARS:
        assert jj.mul_host(k, jm.G) == jm.cached_mul(k, jm.G)
    off = jm.off_curve_point(random.Random(3))
    assert not jj.on_curve_host(off) and not jj.in_subgroup_host(off) and not jj.on_curve_host((R, 1))
    assert [jm.in_subgroup(P) for P in pts] == [True, False, False, False, True, True, True, True, False, False, False]


def test_sign_verify_and_corruptions():
    for sk, PK, m, sig in jm.signed_cases():
        assert jj.keygen_host(sk) == PK and jj.sign_host(sk, m) == sig
        assert jj.verify_host(PK, m, sig) == jm.cached_verify(PK, m, sig) == 0
        assert jj.challenge_host(sig[0], PK, m) == jm.challenge(sig[0], PK, m)
    sk, PK, m, sig = jm.signed_cases()[0]
    seen = set()
    for kind in jm.CORRUPTIONS:
        (pk2, m2, sig2), st = jm.corrupt(kind, PK, m, sig)
        assert jj.verify_host(pk2, m2, sig2) == jm.cached_verify(pk2, m2, sig2) == st != 0, kind
        seen.add(st)
    assert seen == {1, 2, 3, 4}
    with pytest.raises(ValueError):
        jj.keygen_host(0)
    with pytest.raises(ValueError):
        jj.keygen_host(L)


# ---- gadgets on the model's wires ----
def evaluate(b: Builder, publics=(), free=None):
    """build, generate with the model -> (circuit, layout, plan, (a, b, c), check)"""
    circuit, layout = b.build()
    p = am.plan(circuit)
    pi = am.wm.limbs(list(publics) + [0] * (layout.l - len(publics)))
    w = am.generate(circuit, p, pi, am.wm.ints(layout.free(free or {})))
    return circuit, layout, p, w, am.check(circuit, p, *w, pi)


CLEAN = {"bad_rows": 0, "first_bad_row": None, "bad_copies": 0, "first_bad_copy": None}


def point_of(layout, w, P):
    return (w[2][layout.row(P[0])], w[2][layout.row(P[1])])


def test_add_double_select_on_curve():
    pts = jm.case_points()
    pairs = [(pts[4], pts[6]), (pts[4], pts[4]), (pts[4], pts[5]), (pts[0], pts[0]), (pts[3], pts[8]), (pts[2], pts[2])]  # G + (-G): a completeness case
    b = Builder()
    ins = [((b.private(), b.private()), (b.private(), b.private())) for _ in pairs]
    bit1, bit0 = b.private(), b.private()
    rows0 = len(b._rows)
    sums = [jj.ed_add(b, P, Q) for P, Q in ins]
    assert len(b._rows) - rows0 == 14 * len(pairs)
    dbls = [jj.ed_double(b, P) for P, _ in ins]
    assert len(b._rows) - rows0 == (14 + 13) * len(pairs)
    sel1, sel0 = jj.ed_select(b, bit1, *ins[0]), jj.ed_select(b, bit0, *ins[0])
    for P, Q in ins:
        jj.assert_on_curve(b, P)
    assert len(b._rows) - rows0 == (14 + 13 + 5) * len(pairs) + 12
    free = {bit1: 1, bit0: 0}
    for (vp, vq), (P, Q) in zip(ins, pairs):
        free.update({vp[0]: P[0], vp[1]: P[1], vq[0]: Q[0], vq[1]: Q[1]})
    _, layout, _, w, chk = evaluate(b, free=free)
    assert chk == CLEAN
    for s, d, (P, Q) in zip(sums, dbls, pairs):
        assert point_of(layout, w, s) == jm.add(P, Q) and point_of(layout, w, d) == jm.add(P, P)
    assert point_of(layout, w, sel1) == pairs[0][0] and point_of(layout, w, sel0) == pairs[0][1]


def test_assert_on_curve_refuses():
    b = Builder()
    P = (b.private(), b.private())
    jj.assert_on_curve(b, P)
    off = jm.off_curve_point(random.Random(9))
    _, _, _, _, chk = evaluate(b, free={P[0]: off[0], P[1]: off[1]})
    assert chk["bad_rows"] == 1 and chk["bad_copies"] == 0


@pytest.mark.parametrize("nbits,scalars", [(4, [0, 1, 6, 15]), (255, [0, L, R - 1, (1 << 255) - 1])])
def test_scalar_multiplication_gadgets(nbits, scalars):
    """ed_mul_fixed on G and ed_mul on an order-8-tainted point and on G, bits least significant first; bits = 0 .. 0 among them"""
    base = jm.case_points()[10]
    for k in scalars:
        b = Builder()
        bits = [b.private() for _ in range(nbits)]
        P = (b.private(), b.private())
        rows0 = len(b._rows)
        fixed = jj.ed_mul_fixed(b, bits)
        assert len(b._rows) - rows0 == 16 * nbits - 14
        var = jj.ed_mul(b, bits, P)
        assert len(b._rows) - rows0 == 16 * nbits - 14 + 30 * nbits - 27
        free = {v: (k >> i) & 1 for i, v in enumerate(bits)}
        free.update({P[0]: base[0], P[1]: base[1]})
        _, layout, _, w, chk = evaluate(b, free=free)
        assert chk == CLEAN
        assert point_of(layout, w, fixed) == jm.cached_mul(k, jm.G)
        assert point_of(layout, w, var) == jm.cached_mul(k, base)


# ---- to_bits_strict ----
def strict_circuit():
    b = Builder()
    x = b.private()
    y = b.lin(1, x, 0, None, 0)
    rows0 = len(b._rows)
    bits = b.to_bits_strict(y)
    assert len(bits) == 255 and len(b._rows) - rows0 == 1018
    return b, x, bits


@pytest.mark.parametrize("x", [0, 1, 5, R - 1, (1 << 255) - R - 1])
def test_to_bits_strict_honest(x):
    b, vx, bits = strict_circuit()
    _, layout, _, w, chk = evaluate(b, free={vx: x})
    assert chk == CLEAN
    assert [w[2][layout.row(v)] for v in bits] == [(x >> i) & 1 for i in range(255)]


@pytest.mark.parametrize("x", [5, (1 << 255) - R - 1])
def test_to_bits_strict_refuses_the_bits_of_x_plus_r(x, monkeypatch):
    """a prover who fills the advice rows with the bits of x + r (which also recompose to x mod r) and derives every other wire honestly:
    all copies hold -- the sum IS x -- and what fails is a gate row, an assertion e b_k = 0 of the comparison with r - 1"""
    honest = am.value
    monkeypatch.setattr(am, "value", lambda code, a: honest(code, a + R) if code != am.INV0 else honest(code, a))
    b, vx, bits = strict_circuit()
    _, layout, _, w, chk = evaluate(b, free={vx: x})
    assert [w[2][layout.row(v)] for v in bits] == [((x + R) >> i) & 1 for i in range(255)]
    assert chk["bad_copies"] == 0 and chk["bad_rows"] >= 1


# ---- the Schnorr circuit ----
@pytest.fixture(scope="module")
def schnorr():
    circuit, layout, v = jj.schnorr_circuit()
    return circuit, layout, v, am.plan(circuit)


def schnorr_check(schnorr, PK, m, sig):
    circuit, layout, v, p = schnorr
    pi = am.wm.limbs([PK[0], PK[1], m % R, 0])
    w = am.generate(circuit, p, pi, am.wm.ints(jj.schnorr_inputs(layout, v, sig)))
    return am.check(circuit, p, *w, pi)


def test_schnorr_circuit_size_and_digest(schnorr):
    circuit, layout, v, _ = schnorr
    assert (layout.rows, layout.mu, layout.l) == jj.SCHNORR_ROWS
    assert circuit_digest(circuit) == circuit_digest(jj.schnorr_circuit()[0])


def test_schnorr_circuit_accepts_and_refuses(schnorr):
    sk, PK, m, sig = jm.signed_cases()[0]
    assert schnorr_check(schnorr, PK, m, sig) == CLEAN
    for kind in ("r_off_curve", "pk_plus_t8", "pk_identity", "m_bit", "r_negated", "s_bit"):
        (pk2, m2, sig2), _ = jm.corrupt(kind, PK, m, sig)
        chk = schnorr_check(schnorr, pk2, m2, sig2)
        assert chk["bad_rows"] + chk["bad_copies"] >= 1, kind
    # s + l: the gadget compares the bits of s with l - 1.  A signature whose s + l still fits 252 bits (about one in ten) shows it: the point
    # equation holds for s + l, and what refuses it is a gate row of the comparison; a 253-bit value cannot be given at all
    for m2 in range(200):
        Rp, s = jm.sign(sk, m2)
        if s + L < 1 << 252:
            break
    assert s + L < 1 << 252 and schnorr_check(schnorr, PK, m2, (Rp, s)) == CLEAN
    chk = schnorr_check(schnorr, PK, m2, (Rp, s + L))
    assert chk["bad_rows"] >= 1 and chk["bad_copies"] == 0
    big = next(c for c in jm.signed_cases() if c[3][1] + L >= 1 << 252)
    with pytest.raises(ValueError):
        jj.schnorr_inputs(schnorr[1], schnorr[2], (big[3][0], big[3][1] + L))


def test_assert_bits_at_most():
    for c, good, bad in ((0b1011, [0, 7, 8, 11], [12, 13, 15]), (0b1000, [0, 8], [9, 15])):
        for x in good + bad:
            b = Builder()
            bits = [b.private() for _ in range(4)]
            for v in bits:
                b.assert_bool(v)
            b.assert_bits_at_most(bits, c)
            chk = evaluate(b, free={v: (x >> i) & 1 for i, v in enumerate(bits)})[4]
            assert (chk == CLEAN) == (x in good), (c, x)
    with pytest.raises(ValueError):
        Builder().assert_bits_at_most([0, 1, 2], 3)


# ---- the signed transfer ----
@pytest.fixture(scope="module")
def signed():
    circuit, layout, v = jj.merkle_signed_transfer_circuit(2, 8)
    return circuit, layout, v, am.plan(circuit)


def signed_check(signed, name):
    import signed_transfer_cases as sc

    circuit, layout, v, p = signed
    c = sc.case(name)
    pi = am.wm.limbs(c["pi"])
    w = am.generate(circuit, p, pi, am.wm.ints(sc.free_of(layout, v, c)))
    return am.check(circuit, p, *w, pi), w


def test_signed_transfer_circuit(signed):
    import signed_transfer_cases as sc

    circuit, layout, v, _ = signed
    assert (layout.rows, layout.mu, layout.l) == (22323, 15, 2)
    assert circuit_digest(circuit) == circuit_digest(jj.merkle_signed_transfer_circuit(2, 8)[0])
    chk, w = signed_check(signed, "good")
    assert chk == CLEAN
    assert w[2][layout.row(v["m"])] == sc.message(sc.AMOUNT) == jj.signed_transfer_message(sc.case("good")["receiver_key"], sc.AMOUNT, sc.case("good")["pi"][0])
    for name in ("receiver_signed", "other_amount"):
        chk, _ = signed_check(signed, name)
        assert chk["bad_copies"] >= 1 and chk["bad_rows"] == 0, name  # the two sides of the point equation differ: copies, not gates
