"""The integer / big-field model of the pairing tower (tests/pairing_tower_model.py) against itself, where two routes exist."""
import math

import pyoracle as po
import pairing_tower_model as tm
from zkhip import pairing as pr

Q = tm.Q


_fq = tm.rand_fq


def _rand_f12(rng):
    return pr.Fq12([_fq(rng) for _ in range(12)])


def test_linear_frobenius_equals_the_power():
    rng = po.SplitMix64(1201)
    for _ in range(2):
        a = _rand_f12(rng)
        f1 = tm.frob(a, 1)
        assert f1 == a**Q
        assert tm.frob(a, 2) == f1**Q
        assert tm.frob(a, 3) == tm.frob(f1, 2)
    # q^6 is the conjugation of the tower, q^12 the identity
    a = _rand_f12(rng)
    assert tm.frob(tm.frob(a, 3), 3) == tm.conj(a)
    assert tm.frob(tm.conj(tm.frob(a, 3)), 3) == a


def test_cyclotomic_elements_are_unitary_and_of_odd_order():
    rng = po.SplitMix64(1202)
    cyc = tm.cyclotomic_elements([_rand_f12(rng), _rand_f12(rng)])
    one = pr.Fq12.one()
    assert len(cyc) >= 8 and len({tuple(c.c) for c in cyc}) == len(cyc)
    for c in cyc:
        assert c * tm.conj(c) == one
    for g in cyc[1:3]:  # the two generators; the rest are their products and conjugates
        assert g**tm.PHI12 == one
    # -1 and -c are unitary but not in the subgroup: its order is odd
    assert tm.PHI12 % 2 == 1
    for c in tm.unitary_outside(cyc):
        assert c * tm.conj(c) == one and not (c**tm.PHI12 == one)
    # no proper subfield meets the subgroup outside 1
    assert math.gcd(tm.PHI12, Q**6 - 1) == 1


def test_final_exp_is_the_cube_of_the_host_final_exponentiation():
    rng = po.SplitMix64(1203)
    f = _rand_f12(rng)
    assert tm.final_exp(f) == pr.final_exponentiation(f) ** 3
    assert tm.final_exp(pr.Fq12.zero()).is_zero() and tm.final_exp(pr.Fq12.one()) == pr.Fq12.one()
    assert tm.final_exp(tm.embed_fq6([_fq(rng) for _ in range(6)])) == pr.Fq12.one()
    c = tm.easy_part(f)
    assert tm.exp_by_x(c) * c**tm.ATE_X == pr.Fq12.one()


def test_integer_reductions_at_the_thresholds():
    for name, (fn, kmax) in tm.REDUCTIONS.items():
        for k in range(1, kmax + 2):
            for v in (k * Q - 1, k * Q, k * Q + 1):
                if v >= (kmax + 1) * Q:
                    continue
                r = fn(v)
                assert r % Q == v % Q and r <= v, (name, k)
                if name.startswith("csub"):
                    c = {"csub_q": 1, "csub_2q": 2, "csub_4q": 4, "csub_8q": 8}[name] * Q
                    assert r == (v - c if v >= c else v) and r < c
                elif name == "canon8":
                    assert r == v % Q
                else:
                    assert r < 2 * Q and r == (v if v < 2 * Q else v % (2 * Q)), (name, k)
    assert tm.red4(2 * Q - 1) == 2 * Q - 1 and tm.red4(2 * Q) == 0 and tm.red8(6 * Q) == 0 and tm.red16(15 * Q + 5) == Q + 5
    assert tm.sub_k(4, 0, 4 * Q - 1) == 1 and tm.sub_k(12, 5, 0) == 12 * Q + 5
    assert tm.limbs_to_int([1, 2] + [0] * 10 + [3]) == 1 + (2 << 30) + (3 << 360)
    assert tm.mont_inv_residue(Q) == 0 and tm.mont_mul_residue(tm.mont_inv_residue(7), 7) == tm.RADIX % Q


def test_layout_and_embeddings():
    rng = po.SplitMix64(1204)
    comps = [_fq(rng) for _ in range(12)]
    f = tm.from_comps(comps)
    assert tm.to_words(f) == tm.comps_to_words(comps)
    assert tm.to_comps(f) == comps and tm.to_comps(pr.Fq12.one()) == [1] + [0] * 11
    a, b = tm.embed_fq2(comps[0], comps[1]), tm.embed_fq2(comps[2], comps[3])
    want = ((comps[0] * comps[2] - comps[1] * comps[3]) % Q, (comps[0] * comps[3] + comps[1] * comps[2]) % Q)
    assert a * b == tm.embed_fq2(*want)
    # the line operand: c0 + c1 v + c4 v w with v = w^2
    c0, c1, c4 = (comps[0], comps[1]), (comps[2], comps[3]), (comps[4], comps[5])
    w = pr.W
    assert tm.from_comps(tm.line_comps(c0, c1, c4)) == pr.Fq12.from_fq2(c0) + pr.Fq12.from_fq2(c1) * w * w + pr.Fq12.from_fq2(c4) * w * w * w
    assert tm.inv0(pr.Fq12.zero()).is_zero() and tm.inv0(f) * f == pr.Fq12.one()
