"""
The model of zk_g1_decompress_check / zk_g1_check (include/zkhip.h) in Python integers, for tests/test_proof_io.py,
tests/test_gpu_g1check.py and tests/test_gpu_proof_io.py.

Decompression follows the stated rule (flags, x < q, y = (x^3 + 4)^((q+1)/4), the root the sign bit names).  Membership follows the
DEFINITION [r]P = O -- not the endomorphism the kernel and the Python host use -- in homogeneous projective coordinates with the
complete addition law, so the model shares neither a shortcut nor a formula with the code under test.

Seeded generators give every kind of point the issue names; `cases(seed)` is the shared, cached list of (name, encoding).
"""
import functools
import random

import numpy as np

Q = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
X_ABS = 0xD201000000010000
H = (X_ABS + 1) ** 2 // 3  # the cofactor: #E(Fq) = H * R
assert H == 3 * 11**2 * 10177**2 * 859267**2 * 52437899**2 and 3 * H == (X_ABS + 1) ** 2
G = (0x17F1D3A73197D7942695638C4FA9AC0FC3688C4F9774B905A14E3A3F171BAC586C55E83FF97A1AEFFB3AF00ADB22C6BB,
     0x08B3F481E3AAA0F1A09E30ED741D8AE4FCF5E095D5D00AF600DB18CB2C04B3EDD03CC744A2888AE40CAA232946C5E7E1)
OK, BAD_ENCODING, NOT_ON_CURVE, NOT_IN_G1 = 0, 1, 2, 3
B3 = 12  # 3 b


# ---- the group: homogeneous projective (X : Y : Z), complete addition for a = 0 (Renes-Costello-Batina 2016, algorithm 7) ----
def _padd(P, S):
    X1, Y1, Z1 = P
    X2, Y2, Z2 = S
    t0, t1, t2 = X1 * X2 % Q, Y1 * Y2 % Q, Z1 * Z2 % Q
    t3 = ((X1 + Y1) * (X2 + Y2) - t0 - t1) % Q
    t4 = ((Y1 + Z1) * (Y2 + Z2) - t1 - t2) % Q
    y3 = ((X1 + Z1) * (X2 + Z2) - t0 - t2) % Q
    t0 = 3 * t0 % Q
    t2 = B3 * t2 % Q
    z3 = (t1 + t2) % Q
    t1 = (t1 - t2) % Q
    y3 = B3 * y3 % Q
    return ((t3 * t1 - t4 * y3) % Q, (t1 * z3 + y3 * t0) % Q, (z3 * t4 + t0 * t3) % Q)


def mul(P, k: int):
    """[k]P for an affine point (or None) and ANY non-negative integer k (no reduction mod r: the point may be outside G1)"""
    if P is None or k == 0:
        return None
    acc, base = (0, 1, 0), (P[0], P[1], 1)
    for bit in bin(k)[2:]:
        acc = _padd(acc, acc)
        if bit == "1":
            acc = _padd(acc, base)
    return _affine(acc)


def _affine(P):
    if P[2] == 0:
        return None
    zi = pow(P[2], -1, Q)
    return (P[0] * zi % Q, P[1] * zi % Q)


def add(P, S):
    if P is None:
        return S
    if S is None:
        return P
    return _affine(_padd((P[0], P[1], 1), (S[0], S[1], 1)))


def neg(P):
    return None if P is None else (P[0], (-P[1]) % Q)


def on_curve(P) -> bool:
    return P is None or (P[1] * P[1] - P[0] ** 3 - 4) % Q == 0


def in_g1(P) -> bool:
    """the definition"""
    return mul(P, R) is None


# ---- encodings ----
def compress(P) -> bytes:
    if P is None:
        return bytes([0xC0]) + bytes(47)
    b = bytearray(P[0].to_bytes(48, "big"))
    b[0] |= 0x80 | (0x20 if P[1] > (Q - 1) // 2 else 0)
    return bytes(b)


def _mont_words(v: int):
    return [((v << 384) % Q >> (64 * i)) & (2**64 - 1) for i in range(6)]


def words(P) -> np.ndarray:
    """the normalised Jacobian record: (x, y, 1), (1, 1, 0) for infinity, Montgomery form (radix 2^384)"""
    w = _mont_words(1) * 2 + [0] * 6 if P is None else _mont_words(P[0]) + _mont_words(P[1]) + _mont_words(1)
    return np.array(w, dtype=np.uint64)


def jac_words(P, z: int) -> np.ndarray:
    """the representative (x z^2, y z^3, z) of an affine point"""
    return np.array(_mont_words(P[0] * z * z % Q) + _mont_words(P[1] * z**3 % Q) + _mont_words(z % Q), dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def decompress_check(enc: bytes):
    """48 bytes -> (status, point or None).  The point is given for status 0 and 3"""
    assert len(enc) == 48
    c, inf, sign = enc[0] >> 7 & 1, enc[0] >> 6 & 1, enc[0] >> 5 & 1
    x = int.from_bytes(bytes([enc[0] & 0x1F]) + enc[1:], "big")
    if not c:
        return BAD_ENCODING, None
    if inf:
        return (BAD_ENCODING, None) if sign or x else (OK, None)
    if x >= Q:
        return BAD_ENCODING, None
    rhs = (x**3 + 4) % Q
    y = pow(rhs, (Q + 1) // 4, Q)
    if y * y % Q != rhs:
        return NOT_ON_CURVE, None
    if (y > (Q - 1) // 2) != bool(sign):
        y = Q - y
    return (OK if in_g1((x, y)) else NOT_IN_G1), (x, y)


def expected(encs):
    """what zk_g1_decompress_check returns for a list of encodings: (points [k, 18], status [k])"""
    pts, st = np.zeros((len(encs), 18), dtype=np.uint64), np.zeros(len(encs), dtype=np.uint8)
    for i, e in enumerate(encs):
        s, P = decompress_check(bytes(e))
        st[i] = s
        if s in (OK, NOT_IN_G1):
            pts[i] = words(P)
    return pts, st


def check_words(w) -> int:
    """zk_g1_check of one 18-word Jacobian record"""
    w = [int(v) for v in np.asarray(w, dtype=np.uint64).reshape(18)]
    X, Y, Z = (sum(w[6 * k + i] << (64 * i) for i in range(6)) for k in range(3))
    if X >= Q or Y >= Q or Z >= Q:
        return BAD_ENCODING
    rinv = pow(1 << 384, -1, Q)
    X, Y, Z = X * rinv % Q, Y * rinv % Q, Z * rinv % Q
    if Z == 0:
        return OK
    zi = pow(Z, -1, Q)
    P = (X * zi * zi % Q, Y * zi**3 % Q)
    if not on_curve(P):
        return NOT_ON_CURVE
    return OK if in_g1(P) else NOT_IN_G1


# ---- seeded generators ----
def curve_point(rng):
    """a random point of E(Fq) from a trial x: outside G1 with overwhelming probability"""
    while True:
        x = rng.randrange(Q)
        rhs = (x**3 + 4) % Q
        y = pow(rhs, (Q + 1) // 4, Q)
        if y * y % Q == rhs:
            return (x, y if rng.randrange(2) else Q - y)


def no_root_x(rng) -> int:
    while True:
        x = rng.randrange(Q)
        rhs = (x**3 + 4) % Q
        if pow(rhs, (Q - 1) // 2, Q) != 1:
            return x


def small_order(rng, p: int):
    """a point of order exactly p (3 or 11) from a cofactor part T = [r]Q.  The cofactor part of E(Fq) is not cyclic (its 11-part is
    Z_11 x Z_11: [H / 11]T is always infinity), so the whole p-part of H is divided out and the result is walked down by p until the next
    step would be infinity.  At most 64 draws (one succeeds with probability >= 2/3); a draw that gives infinity is skipped"""
    e = 1
    while H % (p * e) == 0:
        e *= p
    for _ in range(64):
        T = mul(mul(curve_point(rng), R), H // e)
        if T is None:
            continue
        for _ in range(8):
            nxt = mul(T, p)
            if nxt is None:
                return T
            T = nxt
    raise AssertionError(f"no point of order {p} found")


def _raw(x: int, flags: int) -> bytes:
    b = bytearray(x.to_bytes(48, "big"))
    b[0] |= flags
    return bytes(b)


@functools.lru_cache(maxsize=None)
def cases(seed: int = 1):
    """[(name, 48 bytes)]: every kind of point and of malformed encoding; the model's verdict on each is decompress_check"""
    rng = random.Random(seed)
    out = []
    members = [mul(G, k) for k in (1, 2, 3, rng.randrange(R), rng.randrange(R), R - 1)]
    out += [("member", compress(P)) for P in members]
    out += [("member-other-sign", compress(neg(P))) for P in members[:3]]  # the wrong sign bit: -P, valid and a different point
    qs = [curve_point(rng) for _ in range(4)]
    out += [("curve", compress(P)) for P in qs] + [("curve-other-sign", compress(neg(P))) for P in qs[:2]]
    ts = [mul(P, R) for P in qs]
    out += [("cofactor", compress(T)) for T in ts]
    out += [("cofactor+kG", compress(add(T, mul(G, k)))) for T, k in zip(ts, (1, 2, rng.randrange(R), R - 1))]
    t3 = [small_order(rng, 3) for _ in range(2)]
    out += [("order3", compress(T)) for T in t3] + [("order3", compress((0, 2))), ("order3", compress((0, Q - 2)))]
    out += [("order3+G", compress(add(t3[0], G)))]
    out += [("order11", compress(small_order(rng, 11))) for _ in range(2)]
    out += [("infinity", compress(None))]
    out += [("x=q", _raw(Q, 0x80)), ("x=q+1", _raw(Q + 1, 0xA0)), ("x=2^381-1", _raw(2**381 - 1, 0x80))]
    out += [("uncompressed", _raw(G[0], 0)), ("uncompressed-inf", _raw(0, 0x40))]
    out += [("inf+sign", _raw(0, 0xE0)), ("inf+low-byte", _raw(1, 0xC0)), ("inf+high-bits", _raw(1 << 380, 0xC0))]
    out += [("no-root", _raw(no_root_x(rng), 0x80)), ("no-root", _raw(no_root_x(rng), 0xA0))]
    return tuple(out)


def by_status(seed: int = 1):
    """{status: [encodings]} of cases(seed): the test batches draw from it"""
    d = {OK: [], BAD_ENCODING: [], NOT_ON_CURVE: [], NOT_IN_G1: []}
    for _, e in cases(seed):
        d[decompress_check(e)[0]].append(e)
    return d
