"""
The model of zk_g2_decompress_check / zk_g2_check (include/zkhip.h) in Python integers, for tests/test_g2check_model.py,
tests/test_vk_io.py, tests/test_gpu_g2check.py and tests/test_gpu_vk_io.py.  It imports nothing of the product.

The twist is E'(Fq2): y^2 = x^3 + 4 (1 + u), Fq2 = Fq[u] / (u^2 + 1), elements are pairs (c0, c1).  Decompression follows the stated rule
(96 bytes big-endian, x.c1 first, flags in byte 0, the root the sign bit names: c1 decides, c0 when y.c1 = 0); the square root is the
NORM method (Fq square roots), not the two-exponentiation method of the kernel and the hosts.  Membership follows the DEFINITION
[r]P = O in homogeneous projective coordinates with the complete addition law -- neither the endomorphism nor a formula is shared with
the code under test.  psi is here too, with constants derived below, so that tests can compare the rule psi(P) == [x]P with the definition.

#E'(Fq2) = N2 = H2 * R; `mul` asserts nothing, but `twist_point` checks [N2]P = O on what it draws: a wrong H2 cannot pass silently.
"""
import functools
import random

import numpy as np

Q = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
X_ABS = 0xD201000000010000
X = -X_ABS  # the BLS parameter
_H2_NUM = X**8 - 4 * X**7 + 5 * X**6 - 4 * X**4 + 6 * X**3 - 4 * X**2 - 4 * X + 13
assert _H2_NUM % 9 == 0
H2 = _H2_NUM // 9
N2 = H2 * R
assert Q % R == X % R  # the eigenvalue of psi on G2: q = t - 1 = x (mod r)
G2 = ((0x024AA2B2F08F0A91260805272DC51051C6E47AD4FA403B02B4510B647AE3D1770BAC0326A805BBEFD48056C8C121BDB8,
       0x13E02B6052719F607DACD3A088274F65596BD0D09920B61AB5DA61BBDC7F5049334CF11213945D57E5AC7D055D042B7E),
      (0x0CE5D527727D6E118CC9CDC6DA2E351AADFD9BAA8CBDD3A76D429A695160D12C923AC9CC3BACA289E193548608B82801,
       0x0606C4A02EA734CC32ACD2B02BC28B99CB3E287E85A763AF267492AB572E99AB3F370D275CEC1DA1AAA9075FF05F79BE))
OK, BAD_ENCODING, NOT_ON_CURVE, NOT_IN_G2 = 0, 1, 2, 3
B = (4, 4)
B3 = (12, 12)  # 3 b
HALF = (Q - 1) // 2


# ---- Fq2 ----
def f2add(a, b):
    return ((a[0] + b[0]) % Q, (a[1] + b[1]) % Q)


def f2sub(a, b):
    return ((a[0] - b[0]) % Q, (a[1] - b[1]) % Q)


def f2mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q)


def f2scal(a, k: int):
    return (a[0] * k % Q, a[1] * k % Q)


def f2inv(a):
    n = pow(a[0] * a[0] + a[1] * a[1], -1, Q)
    return (a[0] * n % Q, -a[1] * n % Q)


def f2pow(a, e: int):
    r = (1, 0)
    for bit in bin(e)[2:]:
        r = f2mul(r, r)
        if bit == "1":
            r = f2mul(r, a)
    return r


def f2conj(a):
    return (a[0], -a[1] % Q)


def _sqrt_fq(a: int):
    r = pow(a, (Q + 1) // 4, Q)
    return r if r * r % Q == a % Q else None


def f2sqrt(a):
    """a root of a in Fq2, or None: the norm method.  With n = a0^2 + a1^2 = s^2, x0^2 = (a0 +- s) / 2 and x1 = a1 / (2 x0)"""
    a0, a1 = a[0] % Q, a[1] % Q
    if a1 == 0:
        r = _sqrt_fq(a0)
        return (r, 0) if r is not None else (0, _sqrt_fq(-a0 % Q))  # -1 is no square in Fq: one of a0, -a0 is
    s = _sqrt_fq((a0 * a0 + a1 * a1) % Q)
    if s is None:
        return None
    inv2 = pow(2, -1, Q)
    x0 = _sqrt_fq((a0 + s) * inv2 % Q)
    if x0 is None:
        x0 = _sqrt_fq((a0 - s) * inv2 % Q)
    if x0 is None or x0 == 0:
        return None
    r = (x0, a1 * pow(2 * x0, -1, Q) % Q)
    return r if f2mul(r, r) == (a0, a1) else None


# ---- the group: homogeneous projective (X : Y : Z), complete addition for a = 0 (Renes-Costello-Batina 2016, algorithm 7) ----
def _padd(P, S):
    X1, Y1, Z1 = P
    X2, Y2, Z2 = S
    t0, t1, t2 = f2mul(X1, X2), f2mul(Y1, Y2), f2mul(Z1, Z2)
    t3 = f2sub(f2sub(f2mul(f2add(X1, Y1), f2add(X2, Y2)), t0), t1)
    t4 = f2sub(f2sub(f2mul(f2add(Y1, Z1), f2add(Y2, Z2)), t1), t2)
    y3 = f2sub(f2sub(f2mul(f2add(X1, Z1), f2add(X2, Z2)), t0), t2)
    t0 = f2scal(t0, 3)
    t2 = f2mul(B3, t2)
    z3 = f2add(t1, t2)
    t1 = f2sub(t1, t2)
    y3 = f2mul(B3, y3)
    return (f2sub(f2mul(t3, t1), f2mul(t4, y3)), f2add(f2mul(t1, z3), f2mul(y3, t0)), f2add(f2mul(z3, t4), f2mul(t0, t3)))


def _affine(P):
    if P[2] == (0, 0):
        return None
    zi = f2inv(P[2])
    return (f2mul(P[0], zi), f2mul(P[1], zi))


def mul(P, k: int):
    """[k]P for an affine point (or None) and ANY non-negative integer k (no reduction mod r: the point may be outside G2)"""
    if P is None or k == 0:
        return None
    acc, base = ((0, 0), (1, 0), (0, 0)), (P[0], P[1], (1, 0))
    for bit in bin(k)[2:]:
        acc = _padd(acc, acc)
        if bit == "1":
            acc = _padd(acc, base)
    return _affine(acc)


def add(P, S):
    if P is None:
        return S
    if S is None:
        return P
    return _affine(_padd((P[0], P[1], (1, 0)), (S[0], S[1], (1, 0))))


def neg(P):
    return None if P is None else (P[0], (-P[1][0] % Q, -P[1][1] % Q))


def on_curve(P) -> bool:
    return P is None or f2mul(P[1], P[1]) == f2add(f2mul(f2mul(P[0], P[0]), P[0]), B)


def in_g2(P) -> bool:
    """the definition"""
    return mul(P, R) is None


# ---- psi = twist . Frobenius . untwist: (x, y) -> (C_X conj(x), C_Y conj(y)) ----
C_X = f2inv(f2pow((1, 1), (Q - 1) // 3))
C_Y = f2inv(f2pow((1, 1), (Q - 1) // 2))


def psi(P):
    return None if P is None else (f2mul(C_X, f2conj(P[0])), f2mul(C_Y, f2conj(P[1])))


def psi_rule(P) -> bool:
    """Scott's test psi(P) == [x]P = -[|x|]P for a point of the twist; infinity is a member"""
    return P is None or psi(P) == neg(mul(P, X_ABS))


# ---- encodings ----
def y_is_larger(y) -> bool:
    """y > -y lexicographically: c1 decides, c0 when c1 = 0"""
    return y[1] > HALF or (y[1] == 0 and y[0] > HALF)


def compress(P) -> bytes:
    if P is None:
        return bytes([0xC0]) + bytes(95)
    b = bytearray(P[0][1].to_bytes(48, "big") + P[0][0].to_bytes(48, "big"))
    b[0] |= 0x80 | (0x20 if y_is_larger(P[1]) else 0)
    return bytes(b)


def _mont_words(v: int):
    return [((v << 384) % Q >> (64 * i)) & (2**64 - 1) for i in range(6)]


def words(P) -> np.ndarray:
    """the affine record x.c0 | x.c1 | y.c0 | y.c1, Montgomery form (radix 2^384); all zero for infinity"""
    if P is None:
        return np.zeros(24, dtype=np.uint64)
    return np.array(_mont_words(P[0][0]) + _mont_words(P[0][1]) + _mont_words(P[1][0]) + _mont_words(P[1][1]), dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def decompress_check(enc: bytes):
    """96 bytes -> (status, point or None).  The point is given for status 0 and 3"""
    assert len(enc) == 96
    c, inf, sign = enc[0] >> 7 & 1, enc[0] >> 6 & 1, enc[0] >> 5 & 1
    x1 = int.from_bytes(bytes([enc[0] & 0x1F]) + enc[1:48], "big")
    x0 = int.from_bytes(enc[48:], "big")
    if not c:
        return BAD_ENCODING, None
    if inf:
        return (BAD_ENCODING, None) if sign or x0 or x1 else (OK, None)
    if x0 >= Q or x1 >= Q:
        return BAD_ENCODING, None
    x = (x0, x1)
    y = f2sqrt(f2add(f2mul(f2mul(x, x), x), B))
    if y is None:
        return NOT_ON_CURVE, None
    if y_is_larger(y) != bool(sign):
        y = (-y[0] % Q, -y[1] % Q)
    return (OK if in_g2((x, y)) else NOT_IN_G2), (x, y)


def expected(encs):
    """what zk_g2_decompress_check returns for a list of encodings: (points [k, 24], status [k])"""
    pts, st = np.zeros((len(encs), 24), dtype=np.uint64), np.zeros(len(encs), dtype=np.uint8)
    for i, e in enumerate(encs):
        s, P = decompress_check(bytes(e))
        st[i] = s
        if s in (OK, NOT_IN_G2):
            pts[i] = words(P)
    return pts, st


def check_words(w) -> int:
    """zk_g2_check of one 24-word affine record"""
    w = [int(v) for v in np.asarray(w, dtype=np.uint64).reshape(24)]
    c = [sum(w[6 * k + i] << (64 * i) for i in range(6)) for k in range(4)]
    if any(v >= Q for v in c):
        return BAD_ENCODING
    if not any(c):
        return OK
    rinv = pow(1 << 384, -1, Q)
    c = [v * rinv % Q for v in c]
    P = ((c[0], c[1]), (c[2], c[3]))
    if not on_curve(P):
        return NOT_ON_CURVE
    return OK if in_g2(P) else NOT_IN_G2


# ---- seeded generators ----
def twist_point(rng):
    """a random point of E'(Fq2) from a trial x: outside G2 with overwhelming probability.  [N2]P = O is asserted"""
    while True:
        x = (rng.randrange(Q), rng.randrange(Q))
        y = f2sqrt(f2add(f2mul(f2mul(x, x), x), B))
        if y is not None:
            P = (x, y if rng.randrange(2) else (-y[0] % Q, -y[1] % Q))
            assert mul(P, N2) is None, "the twist's order is not H2 * R"
            return P


def no_root_x(rng):
    while True:
        x = (rng.randrange(Q), rng.randrange(Q))
        if f2sqrt(f2add(f2mul(f2mul(x, x), x), B)) is None:
            return x


def small_order(rng, p: int):
    """a point of order exactly p (13 or 23) from a cofactor part T = [r]P: the whole p-part of H2 is divided out and the result is
    walked down by p until the next step would be infinity (this works whether the p-part of the group is cyclic or not, where
    [N2 / p]P alone would always be infinity in the second case).  A draw that gives infinity is skipped"""
    e = 1
    while H2 % (p * e) == 0:
        e *= p
    assert e > 1, f"{p} does not divide the cofactor"
    for _ in range(64):
        T = mul(mul(twist_point(rng), R), H2 // e)
        if T is None:
            continue
        for _ in range(8):
            nxt = mul(T, p)
            if nxt is None:
                return T
            T = nxt
    raise AssertionError(f"no point of order {p} found")


def _raw(x0: int, x1: int, flags: int) -> bytes:
    b = bytearray(x1.to_bytes(48, "big") + x0.to_bytes(48, "big"))
    b[0] |= flags
    return bytes(b)


@functools.lru_cache(maxsize=None)
def points(seed: int = 1):
    """[(name, affine point or None)]: every kind of point of the twist the tests use"""
    rng = random.Random(seed)
    out = []
    members = [mul(G2, k) for k in (1, 2, 3, rng.randrange(R), rng.randrange(R), R - 1)]
    out += [("member", P) for P in members] + [("member-neg", neg(P)) for P in members[:3]]
    qs = [twist_point(rng) for _ in range(3)]
    out += [("twist", P) for P in qs] + [("twist-neg", neg(qs[0]))]
    ts = [mul(P, R) for P in qs]
    out += [("cofactor", T) for T in ts]
    out += [("cofactor+kG", add(T, mul(G2, k))) for T, k in zip(ts, (1, rng.randrange(R), R - 1))]
    t13, t23 = small_order(rng, 13), small_order(rng, 23)
    out += [("order13", t13), ("order13", mul(t13, 5)), ("order23", t23), ("order23", mul(t23, 22))]
    out += [("order13+G", add(t13, G2)), ("order23+kG", add(t23, members[3]))]
    out += [("infinity", None)]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def cases(seed: int = 1):
    """[(name, 96 bytes)]: the points of points(seed) and every kind of malformed encoding; the model's verdict is decompress_check"""
    rng = random.Random(seed + 1000)
    out = [(name, compress(P)) for name, P in points(seed)]
    gx = G2[0]
    out += [("x.c0=q", _raw(Q, gx[1], 0x80)), ("x.c1=q", _raw(gx[0], Q, 0x80)), ("x.c0=q+1", _raw(Q + 1, 5, 0xA0)),
            ("x.c0=2^384-1", _raw(2**384 - 1, 5, 0x80)), ("x.c1=2^381-1", _raw(5, 2**381 - 1, 0x80))]
    out += [("uncompressed", _raw(gx[0], gx[1], 0)), ("uncompressed-inf", _raw(0, 0, 0x40))]
    out += [("inf+sign", _raw(0, 0, 0xE0)), ("inf+c0-byte", _raw(1, 0, 0xC0)), ("inf+c1-byte", _raw(0, 1, 0xC0)), ("inf+c1-high", _raw(0, 1 << 380, 0xC0))]
    out += [("no-root", _raw(*no_root_x(rng), 0x80)), ("no-root", _raw(*no_root_x(rng), 0xA0))]
    return tuple(out)


def by_status(seed: int = 1):
    """{status: [encodings]} of cases(seed): the test batches draw from it"""
    d = {OK: [], BAD_ENCODING: [], NOT_ON_CURVE: [], NOT_IN_G2: []}
    for _, e in cases(seed):
        d[decompress_check(e)[0]].append(e)
    return d
