"""
The model of the Jubjub tests: the curve, the group law and the signature scheme "zkhip-schnorr-v1" in python integers, written from the
formulas alone (it imports nothing of zkhip; the Poseidon hash is tests/poseidon_model.py).

    curve      -x^2 + y^2 = 1 + d x^2 y^2 over Fr of BLS12-381, d = -10240 / 10241
    law        (x1, y1) + (x2, y2) = ((x1 y2 + y1 x2) / (1 + d x1 x2 y1 y2), (y1 y2 + x1 x2) / (1 - d x1 x2 y1 y2)), identity (0, 1)
    subgroup   P is a member when [L] P = (0, 1): the definition, nothing faster
    generator  the smallest y >= 2 with x^2 = (y^2 - 1) / (1 + d y^2) a square, the smaller root x, the point times 8
    signature  k = SHA-256(tag || sk || m) mod L, R = [k] G, e = hash2(hash2(hash2(R), hash2(PK)), m), s = k + e sk mod L
    verify     1: s >= L;  2: PK or R not on the curve;  3: PK outside the subgroup or the identity;  4: [s] G != R + [e] PK;  0: valid
               (the first that applies, in this order; e enters as its canonical integer below r, the group reduces it)
"""
import hashlib
import random

import poseidon_model as pm

R = pm.R
D = (-10240 * pow(10241, -1, R)) % R
L = 0x0E7DB4EA6533AFA906673B0101343B00A6682093CCC81082D0970E5ED6F72CB7
TAG = b"zkhip-schnorr-v1"
O = (0, 1)


def is_square(a: int) -> bool:
    return a % R == 0 or pow(a, (R - 1) // 2, R) == 1


def sqrt(a: int):
    """a square root of a (Tonelli-Shanks; r - 1 = 2^32 t), or None"""
    a %= R
    if a == 0:
        return 0
    if not is_square(a):
        return None
    s, t = 0, R - 1
    while t % 2 == 0:
        s, t = s + 1, t // 2
    z = 2
    while is_square(z):
        z += 1
    m, c, u, x = s, pow(z, t, R), pow(a, t, R), pow(a, (t + 1) // 2, R)
    while u != 1:
        i, w = 0, u
        while w != 1:
            w, i = w * w % R, i + 1
        b = pow(c, 1 << (m - i - 1), R)
        m, c, u, x = i, b * b % R, u * b * b % R, x * b % R
    return x


def on_curve(P) -> bool:
    x, y = P
    if not (0 <= x < R and 0 <= y < R):
        return False
    return (y * y - x * x - 1 - D * x * x % R * y * y) % R == 0


def add(P, Q):
    (x1, y1), (x2, y2) = P, Q
    k = D * x1 * x2 * y1 * y2 % R
    return ((x1 * y2 + y1 * x2) * pow(1 + k, -1, R) % R, (y1 * y2 + x1 * x2) * pow(1 - k, -1, R) % R)


def neg(P):
    return ((-P[0]) % R, P[1])


def mul(k: int, P):
    """[k] P for any integer k >= 0: double-and-add from the top bit"""
    acc = O
    for i in reversed(range(k.bit_length())):
        acc = add(acc, acc)
        if (k >> i) & 1:
            acc = add(acc, P)
    return acc


def in_subgroup(P) -> bool:
    return mul(L, P) == O


def point_of_y(y: int):
    """the point (x, y) with the smaller root x, or None"""
    x2 = (y * y - 1) * pow(1 + D * y * y, -1, R) % R
    x = sqrt(x2)
    if x is None:
        return None
    return (min(x, R - x), y)


def generator():
    y = 2
    while point_of_y(y) is None:
        y += 1
    return y, mul(8, point_of_y(y))


G_Y, G = generator()


def random_point(rng: random.Random):
    """a point of the curve with a torsion part (with probability 7 / 8)"""
    while True:
        P = point_of_y(rng.randrange(R))
        if P is not None:
            return P if rng.getrandbits(1) else neg(P)


def torsion(order: int, rng: random.Random | None = None):
    """a point of exact order 2, 4 or 8"""
    rng = rng or random.Random(8)
    if order == 2:
        return (0, R - 1)
    while True:
        T = mul(L, random_point(rng))  # in the 8-torsion
        T = mul(8 // order, T)
        if mul(order, T) == O and mul(order // 2, T) != O:
            return T


def torsion_plus(order: int, k: int, rng: random.Random | None = None):
    """T + [k] G with T of exact order `order`: on the curve, outside the subgroup"""
    return add(torsion(order, rng), mul(k, G))


def le32(x: int) -> bytes:
    return int(x).to_bytes(32, "little")


def challenge(Rp, PK, m: int) -> int:
    return pm.hash2(pm.hash2(pm.hash2(Rp[0], Rp[1]), pm.hash2(PK[0], PK[1])), m % R)


def keygen(sk: int):
    if not 1 <= sk < L:
        raise ValueError("1 <= sk < L is needed")
    return mul(sk, G)


def sign(sk: int, m: int):
    """-> (R, s)"""
    PK = keygen(sk)
    k = int.from_bytes(hashlib.sha256(TAG + le32(sk) + le32(m % R)).digest(), "little") % L
    if k == 0:
        raise ValueError("the nonce is 0")
    Rp = mul(k, G)
    return Rp, (k + challenge(Rp, PK, m) * sk) % L


def verify(PK, m: int, sig) -> int:
    Rp, s = sig
    if s >= L:
        return 1
    if not (on_curve(PK) and on_curve(Rp)):
        return 2
    if PK == O or not in_subgroup(PK):
        return 3
    return 0 if mul(s, G) == add(Rp, mul(challenge(Rp, PK, m), PK)) else 4


def signature_digest(sig) -> str:
    """SHA-256 of R.x || R.y || s, 32-byte little-endian canonical encodings"""
    (x, y), s = sig
    return hashlib.sha256(le32(x) + le32(y) + le32(s)).hexdigest()


# ---- the cases the CPU and the GPU tests share ----
SCALARS = [0, 1, 2, L - 1, L, L + 1, R - 1, (1 << 255) - 1, (1 << 256) - 1]
_cases = {}


def case_points():
    """the identity, (0, -1), an order-4 and an order-8 point, G, -G, two random subgroup points and three points outside the subgroup
    (a random one, T4 + [5] G, T8 + [7] G): 11 points, built once"""
    if "points" not in _cases:
        rng = random.Random(2024)
        _cases["points"] = [O, (0, R - 1), torsion(4, rng), torsion(8, rng), G, neg(G), mul(rng.randrange(L), G), mul(8, random_point(rng)),
                            random_point(rng), torsion_plus(4, 5, rng), torsion_plus(8, 7, rng)]
    return _cases["points"]


def cached_mul(k: int, P):
    key = ("mul", k, P)
    if key not in _cases:
        _cases[key] = mul(k, P)
    return _cases[key]


def cached_verify(PK, m: int, sig) -> int:
    key = ("verify", PK, m, sig)
    if key not in _cases:
        _cases[key] = verify(PK, m, sig)
    return _cases[key]


def off_curve_point(rng: random.Random):
    while True:
        P = (rng.randrange(R), rng.randrange(R))
        if not on_curve(P):
            return P


def signed_cases():
    """four (sk, PK, m, sig) with valid signatures, built once"""
    if "signed" not in _cases:
        rng = random.Random(77)
        out = []
        for _ in range(4):
            sk, m = rng.randrange(1, L), rng.randrange(R)
            out.append((sk, keygen(sk), m, sign(sk, m)))
        _cases["signed"] = out
    return _cases["signed"]


CORRUPTIONS = ("s_plus_l", "r_off_curve", "pk_plus_t8", "pk_identity", "m_bit", "ry_bit", "r_negated", "s_bit")


def corrupt(kind: str, PK, m: int, sig):
    """-> (PK, m, sig) with one thing wrong, and the status the scheme gives it (verify() must agree)"""
    (rx, ry), s = sig
    if kind == "s_plus_l":
        return (PK, m, ((rx, ry), s + L)), 1
    if kind == "r_off_curve":
        return (PK, m, (((rx + 1) % R, ry), s)), 2
    if kind == "pk_plus_t8":
        return (add(PK, torsion(8)), m, sig), 3
    if kind == "pk_identity":
        return (O, m, sig), 3
    if kind == "m_bit":
        return (PK, m ^ 1, sig), 4
    if kind == "ry_bit":  # a flipped bit of R.y: the equation's status if the point stays on the curve, which it does not for these cases
        Rp = (rx, ry ^ 1)
        return (PK, m, (Rp, s)), 4 if on_curve(Rp) else 2
    if kind == "r_negated":  # a wrong R that IS on the curve: the equation fails
        return (PK, m, (neg((rx, ry)), s)), 4
    if kind == "s_bit":
        s2 = s ^ 1
        return (PK, m, ((rx, ry), s2 if s2 < L else s ^ 2)), 4
    raise ValueError(kind)
