"""
Plain-integer model of the device pairing's field tower (csrc/fq30.cuh, curve30_g2.cuh, fq12.cuh, final_exp / f12_exp_by_x of
zk_pairing.hip), for tests/test_gpu_pairing_tower.py and tests/test_pairing_tower_model.py.

Two layers:
  * Fq30: the lazily reduced base field as EXACT INTEGERS (not residues): a conditional subtraction either happens or not, a
    subtraction adds a stated multiple of q, an addition is an addition.  Only the Montgomery products leave the representative
    open (any value < 2q of the right residue); for those the model gives the residue.
  * the tower: zkhip.pairing.Fq12, i.e. Fq[w] / (w^12 - 2 w^6 + 2) -- a different representation from the device's 2-3-2 tower --
    with conjugation, Frobenius (by Fq-linearity from powers computed with **, none of the device's constants), the sparse line
    operand, the final exponentiation as one big power, and generators of cyclotomic-subgroup elements.
Elements travel as 12 canonical integers in ark's component order (c0.c0.c0, c0.c0.c1, c0.c1.c0, ..., c1.c2.c1): "comps".
"""
from typing import List, Sequence

from zkhip import pairing as pr
from zkhip.field import Q_MOD, R_MOD

Q = Q_MOD
R = R_MOD
ATE_X = pr.ATE_LOOP
RADIX = 1 << 390  # Montgomery radix of the internal form
RADIX_INV = pow(RADIX, -1, Q)
EXP_MULTIPLE = 3  # ZK_PAIRING_EXP_MULTIPLE
PHI12 = Q**4 - Q**2 + 1  # order of the cyclotomic subgroup (odd)


def rand_fq(rng) -> int:
    """an integer below q from a generator with next() -> 64 bits (pyoracle.SplitMix64)"""
    return sum(rng.next() << (64 * i) for i in range(6)) % Q


# ---- Fq30 layer: exact integers ----------------------------------------------------------------------------------------------------
def limbs_to_int(limbs: Sequence[int]) -> int:
    """13 limbs of 30 bits (the last may be wider) -> the integer they stand for"""
    return sum(int(l) << (30 * i) for i, l in enumerate(limbs))


def csub(v: int, c: int) -> int:
    return v - c if v >= c else v


def red4(v: int) -> int:
    return csub(v, 2 * Q)


def red8(v: int) -> int:
    return csub(csub(v, 4 * Q), 2 * Q)


def red16(v: int) -> int:
    return red8(csub(v, 8 * Q))


def canon8(v: int) -> int:
    return csub(csub(csub(v, 4 * Q), 2 * Q), Q)


# mode name -> (integer function of a, largest k such that every a = x + k q with x < q is inside the function's contract)
REDUCTIONS = {
    "csub_q": (lambda v: csub(v, Q), 1),
    "csub_2q": (lambda v: csub(v, 2 * Q), 3),
    "csub_4q": (lambda v: csub(v, 4 * Q), 7),
    "csub_8q": (lambda v: csub(v, 8 * Q), 15),
    "red4": (red4, 3),
    "red8": (red8, 7),
    "red16": (red16, 15),
    "canon8": (canon8, 7),
}


def sub_k(K: int, a: int, b: int) -> int:
    """f30_subK: a + K q - b for b < K q"""
    return a + K * Q - b


def mont_mul_residue(a: int, b: int) -> int:
    return a * b * RADIX_INV % Q


def mont_inv_residue(a: int) -> int:
    """f30_inv: a^(q-2) by Montgomery products from the Montgomery one, i.e. 2^780 / a; 0 for a = 0 mod q"""
    return 0 if a % Q == 0 else RADIX * RADIX * pow(a, -1, Q) % Q


# ---- ark component order <-> zkhip.pairing.Fq12 ------------------------------------------------------------------------------------
_R384 = (1 << 384) % Q
_MASK64 = (1 << 64) - 1


def comps_to_words(comps: Sequence[int]) -> List[int]:
    """12 canonical integers -> the 72 u64 of ark's layout (each Fq in Montgomery form, radix 2^384)"""
    out: List[int] = []
    for x in comps:
        m = x % Q * _R384 % Q
        out.extend((m >> (64 * k)) & _MASK64 for k in range(6))
    return out


def from_comps(comps: Sequence[int]) -> pr.Fq12:
    return pr.fq12_from_ark(comps_to_words(comps))


def to_words(f: pr.Fq12) -> List[int]:
    return pr.fq12_to_ark(f)


_SLOTS = [(i, j) for i in range(2) for j in range(3)]  # the Fq2 coefficient of w^i v^j, in ark's order; v = w^2, u = w^6 - 1


def to_comps(f: pr.Fq12) -> List[int]:
    """the 12 canonical integers of f in ark's component order"""
    out: List[int] = []
    for i, j in _SLOTS:
        e = i + 2 * j
        out += [(f.c[e] + f.c[e + 6]) % Q, f.c[e + 6]]
    return out


def embed_fq6(comps6: Sequence[int]) -> pr.Fq12:
    """an Fq6 element (6 integers: c0.c0, c0.c1, c1.c0, ...) as the Fq12 element with c1 = 0"""
    return from_comps(list(comps6) + [0] * 6)


def embed_fq2(c0: int, c1: int) -> pr.Fq12:
    return from_comps([c0, c1] + [0] * 10)


# ---- tower operations --------------------------------------------------------------------------------------------------------------
def conj(f: pr.Fq12) -> pr.Fq12:
    """f^(q^6): w^(q^6) = -w, so the odd coefficients change sign"""
    return pr.Fq12([c if e % 2 == 0 else -c for e, c in enumerate(f.c)])


def inv0(f: pr.Fq12) -> pr.Fq12:
    """the device's convention: 0 -> 0"""
    return pr.Fq12.zero() if f.is_zero() else f.inv()


_FROB_BASIS = {}


def frob_basis(K: int) -> List[pr.Fq12]:
    """(w^e)^(q^K) for e = 0..11, by ** alone: w^(q^K) from K successive powers by q, then its e-th powers"""
    if not _FROB_BASIS:
        wq = pr.W
        for k in (1, 2, 3):
            wq = wq**Q
            _FROB_BASIS[k] = [wq**e for e in range(12)]
    return _FROB_BASIS[K]


def frob(f: pr.Fq12, K: int) -> pr.Fq12:
    """f^(q^K) by Fq-linearity: sum_e f_e (w^e)^(q^K)"""
    acc = pr.Fq12.zero()
    for c, b in zip(f.c, frob_basis(K)):
        if c:
            acc = acc + b.scale(c)
    return acc


def line_comps(c0, c1, c4) -> List[int]:
    """the sparse operand of f12_mul_by_014 as a dense element: c0 + c1 v + c4 v w, every other component zero"""
    out = [0] * 12
    out[0], out[1], out[2], out[3], out[8], out[9] = c0[0], c0[1], c1[0], c1[1], c4[0], c4[1]
    return out


def final_exp(f: pr.Fq12) -> pr.Fq12:
    """the device's final exponentiation: f^(3 (q^12 - 1) / r); 0 -> 0"""
    return f ** (EXP_MULTIPLE * ((Q**12 - 1) // R))


def exp_by_x(f: pr.Fq12) -> pr.Fq12:
    """f^x for the negative BLS parameter x and f in the cyclotomic subgroup, where the conjugate is the inverse"""
    return conj(f**ATE_X)


def easy_part(f: pr.Fq12) -> pr.Fq12:
    """f^((q^6 - 1)(q^2 + 1)): lands in the cyclotomic subgroup (order q^4 - q^2 + 1)"""
    g = conj(f) * f.inv()
    return g ** (Q**2 + 1)


def cyclotomic_elements(seeds: Sequence[pr.Fq12]) -> List[pr.Fq12]:
    """
    1, the easy part of every seed (two seeds are what the tests use), and cheap products / conjugates / squares / small powers
    of those (duplicates dropped): the subgroup is closed under all of them.  -1 is NOT in it: the subgroup's order
    q^4 - q^2 + 1 is odd, and the Granger-Scott squaring is wrong on -1 (it gives 5); -1 and -c are `unitary_outside()`.  No
    element other than 1 lies in a proper subfield: gcd(q^4 - q^2 + 1, q^6 - 1) = 1, so Fq6 (and with it Fq2, Fq) meets the
    subgroup in {1}.
    """
    gens = [easy_part(s) for s in seeds]
    out = [pr.Fq12.one()] + gens
    out += [conj(g) for g in gens] + [g * g for g in gens]
    for i in range(len(gens)):
        for j in range(i + 1, len(gens)):
            gi, gj = gens[i], gens[j]
            out += [gi * gj, gi * conj(gj), conj(gi * gi * gj)]
            pi = gi
            for a in range(1, 6):  # gi^a gj^b, a, b = 1..5
                pj = gj
                for b in range(1, 6):
                    out.append(pi * pj)
                    pj = pj * gj
                pi = pi * gi
    seen, uniq = set(), []
    for c in out:
        if tuple(c.c) not in seen:
            seen.add(tuple(c.c))
            uniq.append(c)
    return uniq


def unitary_outside(cyc: Sequence[pr.Fq12]) -> List[pr.Fq12]:
    """-1 and -c: a conj(a) = 1 still holds (order divides q^6 + 1) but the order is even, so they are outside the cyclotomic subgroup"""
    return [-pr.Fq12.one()] + [-c for c in cyc[1:3]]
