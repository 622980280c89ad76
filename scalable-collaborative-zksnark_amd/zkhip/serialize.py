"""
arkworks wire / on-disk encodings for the types that cross the reference's network and file
boundaries (dist-primitive/src/utils/serializing_net.rs:17,50,88,111 `serialize_compressed`;
examples/delegator.rs:35-39,64-68 `serialize_uncompressed`).  On one MI355X node the exchanges move
raw limbs (no compression on xGMI); these encoders exist so shares and proofs can be handed to /
taken from the Rust prover unchanged.

  Fr            canonical little-endian, 32 bytes (ark-serialize 0.4.2 for Fp)
  Vec<T>        u64 LE length, then the items; tuples = concatenation
  G1 compressed ark-bls12-381 0.4.0 (zcash style): 48-byte BIG-endian x; top three bits of byte 0 =
                (compressed = 1, infinity, y is the lexicographically larger root)
  G1 uncompressed  96 bytes: x || y big-endian, same flag bits with compressed = 0
ASSUMPTION: restated from the public specification; the only in-tree
evidence is message sizes (56 B = 8 + 48 for a one-point Vec<G1>, hack/run-hyperplonk/output.txt:25).
"""
from __future__ import annotations

import struct
from typing import List, Optional, Sequence, Tuple

from .field import Q_MOD, R_MOD

Point = Optional[Tuple[int, int]]


def fr_serialize(x: int) -> bytes:
    return int(x % R_MOD).to_bytes(32, "little")


def fr_deserialize(b: bytes) -> int:
    v = int.from_bytes(b[:32], "little")
    if v >= R_MOD:
        raise ValueError("non-canonical Fr encoding")
    return v


def vec_serialize(items: Sequence[bytes]) -> bytes:
    return struct.pack("<Q", len(items)) + b"".join(items)


def fr_vec_serialize(xs: Sequence[int]) -> bytes:
    return vec_serialize([fr_serialize(x) for x in xs])


def fr_vec_deserialize(b: bytes) -> List[int]:
    (n,) = struct.unpack_from("<Q", b, 0)
    return [fr_deserialize(b[8 + 32 * i : 40 + 32 * i]) for i in range(n)]


def _sqrt_fq(a: int) -> Optional[int]:
    # q = 3 mod 4
    r = pow(a, (Q_MOD + 1) // 4, Q_MOD)
    return r if r * r % Q_MOD == a % Q_MOD else None


def g1_serialize_compressed(P: Point) -> bytes:
    if P is None:
        b = bytearray(48)
        b[0] = 0xC0
        return bytes(b)
    x, y = P
    b = bytearray(x.to_bytes(48, "big"))
    b[0] |= 0x80
    if y > (Q_MOD - 1) // 2:
        b[0] |= 0x20
    return bytes(b)


def g1_deserialize_compressed(b: bytes) -> Point:
    flags = b[0] & 0xE0
    if not flags & 0x80:
        raise ValueError("not a compressed encoding")
    if flags & 0x40:
        return None
    x = int.from_bytes(bytes([b[0] & 0x1F]) + b[1:48], "big")
    y = _sqrt_fq((x * x * x + 4) % Q_MOD)
    if y is None:
        raise ValueError("x is not on the curve")
    if (y > (Q_MOD - 1) // 2) != bool(flags & 0x20):
        y = Q_MOD - y
    return (x, y)


def g1_serialize_uncompressed(P: Point) -> bytes:
    if P is None:
        b = bytearray(96)
        b[0] = 0x40
        return bytes(b)
    return P[0].to_bytes(48, "big") + P[1].to_bytes(48, "big")


def g1_deserialize_uncompressed(b: bytes) -> Point:
    if b[0] & 0x40:
        return None
    x = int.from_bytes(bytes([b[0] & 0x1F]) + b[1:48], "big")
    y = int.from_bytes(b[48:96], "big")
    if (y * y - x * x * x - 4) % Q_MOD:
        raise ValueError("point not on the curve")
    return (x, y)


def g1_vec_serialize_compressed(ps: Sequence[Point]) -> bytes:
    return vec_serialize([g1_serialize_compressed(P) for P in ps])


# ---------------------------------------------------------------------------------------
# share files of dist-primitive/examples/delegator.rs: `<dir>/delegator` holds the witness Vec<Fr>,
# `<dir>/worker_<i>` party i's Vec<Fr> of packed shares, both written with `serialize_uncompressed`
# (:35-39, :64-68, :82-95).  For a prime field the uncompressed encoding IS the canonical 32-byte
# little-endian one, so a file is `u64 LE length || 32-byte elements`.  (The example is instantiated on
# ark_bls12_377::Fr; the layout does not depend on the field, the modulus check below does: BLS12-381.)
# ---------------------------------------------------------------------------------------
def delegator_share(x: Sequence[int], pp) -> List[List[int]]:
    """Delegator::delegate (:48-62): chunks of l secrets -> pack_from_public -> worker j collects share j"""
    workers: List[List[int]] = [[] for _ in range(pp.n)]
    for k in range(0, len(x), pp.l):
        for j, s in enumerate(pp.pack_from_public(list(x[k : k + pp.l]))):
            workers[j].append(s)
    return workers


def delegator_write(directory: str, x: Sequence[int], pp) -> None:
    """main (:71-95): the directory must exist; writes `delegator` and `worker_0 .. worker_{8l-1}`"""
    import os

    if not os.path.isdir(directory):
        raise FileNotFoundError(f"{directory} does not exist")  # the example panics
    with open(os.path.join(directory, "delegator"), "wb") as f:
        f.write(fr_vec_serialize(x))
    for i, w in enumerate(delegator_share(x, pp)):
        with open(os.path.join(directory, f"worker_{i}"), "wb") as f:
            f.write(fr_vec_serialize(w))


def fr_file_to_limbs(path: str):
    """a share file -> [n, 4] uint64 CANONICAL limbs (numpy view of the payload, no per-element python work)"""
    import numpy as np

    raw = open(path, "rb").read()
    (n,) = struct.unpack_from("<Q", raw, 0)
    if len(raw) != 8 + 32 * n:
        raise ValueError(f"{path}: length prefix {n} does not match {len(raw)} bytes")
    a = np.frombuffer(raw, dtype="<u8", offset=8).reshape(n, 4).astype(np.uint64)
    r = np.array([(R_MOD >> (64 * i)) & ((1 << 64) - 1) for i in range(4)], dtype=np.uint64)
    lt, eq = np.zeros(n, dtype=bool), np.ones(n, dtype=bool)
    for k in (3, 2, 1, 0):
        lt |= eq & (a[:, k] < r[k])
        eq &= a[:, k] == r[k]
    if not lt.all():
        raise ValueError(f"{path}: non-canonical Fr encoding")
    return a


_R2 = (1 << 512) % R_MOD


def fr_file_to_device(ctx, path: str):
    """
    a share file -> (device buffer of n Fr in the library's Montgomery form, n).  The conversion runs on the
    GPU: canonical limbs a are the Montgomery form of a/R, one Montgomery multiplication by R^2 gives a*R.
    """
    from .field import int_to_limbs

    a = fr_file_to_limbs(path)
    buf = ctx.to_device(a)
    return ctx.fr_scale(buf, int_to_limbs(_R2, 4), len(a), out=buf), len(a)


def fr_device_to_file(ctx, buf, n: int, path: str) -> None:
    """device Fr vector (Montgomery) -> share file; out of Montgomery form on the GPU (multiplication by 1)"""
    from .field import int_to_limbs

    tmp = ctx.fr_scale(buf, int_to_limbs(1, 4), n)
    a = tmp.download((n, 4))
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", n) + a.astype("<u8").tobytes())


# ---------------------------------------------------------------------------------------
# G1 points from outside: the rule of zk_g1_decompress_check (include/zkhip.h) in Python integers, for callers without a
# device.  status 0 ok, 1 bad encoding, 2 x is not on the curve, 3 on the curve but not in G1.
# ---------------------------------------------------------------------------------------
G1_OK, G1_BAD_ENCODING, G1_NOT_ON_CURVE, G1_NOT_IN_SUBGROUP = 0, 1, 2, 3
G1_STATUS_TEXT = {G1_OK: "ok", G1_BAD_ENCODING: "bad encoding", G1_NOT_ON_CURVE: "x is not on the curve", G1_NOT_IN_SUBGROUP: "not in the subgroup"}
X_ABS = 0xD201000000010000
# phi(x, y) = (BETA x, y) is multiplication by -X_ABS^2 on G1 (X_ABS^4 - X_ABS^2 + 1 = r); the other cube root of unity is X_ABS^2 - 1
BETA = 0x5F19672FDF76CE51BA69C6076A0F77EADDB3A93BE6F89688DE17D813620A00022E01FFFFFFFEFFFE


def _jac_dbl(P):
    X, Y, Z = P
    if Z == 0:
        return P
    A, B = X * X % Q_MOD, Y * Y % Q_MOD
    C = B * B % Q_MOD
    D = 2 * ((X + B) * (X + B) - A - C) % Q_MOD
    E = 3 * A % Q_MOD
    X3 = (E * E - 2 * D) % Q_MOD
    return (X3, (E * (D - X3) - 8 * C) % Q_MOD, 2 * Y * Z % Q_MOD)


def _jac_add(P, R):
    """complete: equal operands, opposite operands and infinity on either side"""
    if P[2] == 0:
        return R
    if R[2] == 0:
        return P
    (X1, Y1, Z1), (X2, Y2, Z2) = P, R
    Z1Z1, Z2Z2 = Z1 * Z1 % Q_MOD, Z2 * Z2 % Q_MOD
    U1, U2 = X1 * Z2Z2 % Q_MOD, X2 * Z1Z1 % Q_MOD
    S1, S2 = Y1 * Z2 * Z2Z2 % Q_MOD, Y2 * Z1 * Z1Z1 % Q_MOD
    if U1 == U2:
        return _jac_dbl(P) if S1 == S2 else (1, 1, 0)
    H, r = (U2 - U1) % Q_MOD, (S2 - S1) % Q_MOD
    HH = H * H % Q_MOD
    HHH, V = H * HH % Q_MOD, U1 * HH % Q_MOD
    X3 = (r * r - HHH - 2 * V) % Q_MOD
    return (X3, (r * (V - X3) - S1 * HHH) % Q_MOD, Z1 * Z2 * H % Q_MOD)


def _jac_mul(P, k: int):
    acc = (1, 1, 0)
    for bit in bin(k)[2:]:
        acc = _jac_dbl(acc)
        if bit == "1":
            acc = _jac_add(acc, P)
    return acc


def g1_in_subgroup(P: Point) -> bool:
    """phi(P) == -[x^2]P for a point of the curve (Scott's test, the one of csrc/zk_g1check.hip); infinity is a member"""
    if P is None:
        return True
    x, y = P
    X, Y, Z = _jac_mul(_jac_mul((x, y, 1), X_ABS), X_ABS)
    if Z == 0:
        return False
    ZZ = Z * Z % Q_MOD
    return (BETA * x * ZZ - X) % Q_MOD == 0 and (y * ZZ * Z + Y) % Q_MOD == 0


def g1_point_words(P: Point):
    """the library's normalised Jacobian record of a point: 18 u64, (x, y, 1) or (1, 1, 0) for infinity, Montgomery form"""
    import numpy as np

    from .field import fq_mont

    one = fq_mont(1)
    if P is None:
        return np.concatenate([one, one, np.zeros(6, dtype=np.uint64)])
    return np.concatenate([fq_mont(P[0]), fq_mont(P[1]), one])


def g1_decompress_check_host(data):
    """k compressed points (bytes or a uint8 array of k x 48) -> (points [k, 18], status [k] uint8): the results of
    Ctx.g1_decompress_check, bit for bit (the points of status 1 and 2 are zero)"""
    import numpy as np

    raw = bytes(data) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8).tobytes()
    if len(raw) % 48:
        raise ValueError(f"{len(raw)} bytes is not a whole number of 48-byte points")
    k = len(raw) // 48
    pts, st = np.zeros((k, 18), dtype=np.uint64), np.zeros(k, dtype=np.uint8)
    for i in range(k):
        b = raw[48 * i : 48 * i + 48]
        rest = int.from_bytes(bytes([b[0] & 0x1F]) + b[1:], "big")
        if not b[0] & 0x80:
            st[i] = G1_BAD_ENCODING
        elif b[0] & 0x40:
            if b[0] & 0x20 or rest:
                st[i] = G1_BAD_ENCODING
            else:
                pts[i] = g1_point_words(None)
        elif rest >= Q_MOD:
            st[i] = G1_BAD_ENCODING
        else:
            y = _sqrt_fq((rest * rest * rest + 4) % Q_MOD)
            if y is None:
                st[i] = G1_NOT_ON_CURVE
                continue
            if (y > (Q_MOD - 1) // 2) != bool(b[0] & 0x20):
                y = Q_MOD - y
            pts[i] = g1_point_words((rest, y))
            if not g1_in_subgroup((rest, y)):
                st[i] = G1_NOT_IN_SUBGROUP
    return pts, st


# ---------------------------------------------------------------------------------------
# G2 points from outside: the rule of zk_g2_decompress_check (include/zkhip.h) in Python integers, for callers without a
# device.  A point of the twist y^2 = x^3 + 4 (1 + u) is ((x.c0, x.c1), (y.c0, y.c1)) as in pairing.py.  96 bytes big-endian, x.c1
# first; the sign bit names the larger of (y, -y): c1 decides, c0 when y.c1 = 0.  The status values are the G1 ones.
# ---------------------------------------------------------------------------------------
G2_OK, G2_BAD_ENCODING, G2_NOT_ON_CURVE, G2_NOT_IN_SUBGROUP = 0, 1, 2, 3
G2_STATUS_TEXT = {G2_OK: "ok", G2_BAD_ENCODING: "bad encoding", G2_NOT_ON_CURVE: "x is not on the curve", G2_NOT_IN_SUBGROUP: "not in the subgroup"}
# psi(x, y) = (PSI_CX conj(x), PSI_CY conj(y)) is multiplication by q = -X_ABS (mod r) on G2: PSI_CX = (1 + u)^(-(q-1)/3),
# PSI_CY = (1 + u)^(-(q-1)/2) (derived, and checked on the generator, in tests/g2check_model.py)
PSI_CX = (0, 0x1A0111EA397FE699EC02408663D4DE85AA0D857D89759AD4897D29650FB85F9B409427EB4F49FFFD8BFD00000000AAAD)
PSI_CY = (0x135203E60180A68EE2E9C448D77A2CD91C3DEDD930B1CF60EF396489F61EB45E304466CF3E67FA0AF1EE7B04121BDEA2,
          0x06AF0E0437FF400B6831E36D6BD17FFE48395DABC2D3435E77F76E17009241C5EE67992F72EC05F4C81084FBEDE3CC09)
_HALF_Q = (Q_MOD - 1) // 2


def _f2mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % Q_MOD, (a[0] * b[1] + a[1] * b[0]) % Q_MOD)


def _f2pow(a, e: int):
    r = (1, 0)
    for bit in bin(e)[2:]:
        r = _f2mul(r, r)
        if bit == "1":
            r = _f2mul(r, a)
    return r


def _sqrt_fq2(a):
    """a root of a in Fq2 or None (q = 3 mod 4: the two-exponentiation method of csrc/zk_g2check.hip, the candidate checked by squaring)"""
    a = (a[0] % Q_MOD, a[1] % Q_MOD)
    a1 = _f2pow(a, (Q_MOD - 3) // 4)
    x0 = _f2mul(a1, a)
    alpha = _f2mul(a1, x0)
    if alpha == (Q_MOD - 1, 0):
        y = (-x0[1] % Q_MOD, x0[0])
    else:
        y = _f2mul(_f2pow(((alpha[0] + 1) % Q_MOD, alpha[1]), (Q_MOD - 1) // 2), x0)
    return y if _f2mul(y, y) == a else None


def _g2_rhs(x):
    t = _f2mul(_f2mul(x, x), x)
    return ((t[0] + 4) % Q_MOD, (t[1] + 4) % Q_MOD)


def _g2_y_is_larger(y) -> bool:
    return y[1] > _HALF_Q or (y[1] == 0 and y[0] > _HALF_Q)


def g2_serialize_compressed(P) -> bytes:
    if P is None:
        return bytes([0xC0]) + bytes(95)
    (x0, x1), y = P
    b = bytearray(x1.to_bytes(48, "big") + x0.to_bytes(48, "big"))
    b[0] |= 0x80 | (0x20 if _g2_y_is_larger(y) else 0)
    return bytes(b)


def g2_deserialize_compressed(b: bytes):
    """96 bytes -> the point of the twist (None: infinity); ValueError for what is no encoding of one.  Membership in G2 is NOT
    tested here: g2_in_subgroup, or g2_decompress_check_host for both"""
    st, P = _g2_decode(bytes(b))
    if st:
        raise ValueError(G2_STATUS_TEXT[st])
    return P


def _g2_decode(b: bytes):
    """(status 0 / 1 / 2, point)"""
    if len(b) != 96:
        raise ValueError(f"{len(b)} bytes: a compressed G2 point has 96")
    x1 = int.from_bytes(bytes([b[0] & 0x1F]) + b[1:48], "big")
    x0 = int.from_bytes(b[48:], "big")
    if not b[0] & 0x80:
        return G2_BAD_ENCODING, None
    if b[0] & 0x40:
        return (G2_BAD_ENCODING if b[0] & 0x20 or x0 or x1 else G2_OK), None
    if x0 >= Q_MOD or x1 >= Q_MOD:
        return G2_BAD_ENCODING, None
    y = _sqrt_fq2(_g2_rhs((x0, x1)))
    if y is None:
        return G2_NOT_ON_CURVE, None
    if _g2_y_is_larger(y) != bool(b[0] & 0x20):
        y = (-y[0] % Q_MOD, -y[1] % Q_MOD)
    return G2_OK, ((x0, x1), y)


def g2_in_subgroup(P) -> bool:
    """psi(P) == [x]P = -[X_ABS]P for a point of the twist (Scott's test, the one of csrc/zk_g2check.hip); infinity is a member"""
    from . import pairing as pr

    if P is None:
        return True
    x, y = P
    psi = (_f2mul(PSI_CX, (x[0], -x[1] % Q_MOD)), _f2mul(PSI_CY, (y[0], -y[1] % Q_MOD)))
    return pr.g2_neg(pr.g2_mul(P, X_ABS)) == psi  # (X_ABS < r: g2_mul's reduction of the scalar does not touch it)


def g2_point_words(P):
    """the affine record of a point: 24 u64 x.c0 | x.c1 | y.c0 | y.c1, Montgomery form; all zero for infinity"""
    import numpy as np

    from .field import fq_mont

    if P is None:
        return np.zeros(24, dtype=np.uint64)
    return np.concatenate([fq_mont(P[0][0]), fq_mont(P[0][1]), fq_mont(P[1][0]), fq_mont(P[1][1])])


def g2_decompress_check_host(data):
    """k compressed points (bytes or a uint8 array of k x 96) -> (points [k, 24], status [k] uint8): the results of
    Ctx.g2_decompress_check, bit for bit (the points of status 1 and 2 and infinity are zero)"""
    import numpy as np

    raw = bytes(data) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8).tobytes()
    if len(raw) % 96:
        raise ValueError(f"{len(raw)} bytes is not a whole number of 96-byte points")
    k = len(raw) // 96
    pts, st = np.zeros((k, 24), dtype=np.uint64), np.zeros(k, dtype=np.uint8)
    for i in range(k):
        st[i], P = _g2_decode(raw[96 * i : 96 * i + 96])
        if st[i] == G2_OK and P is not None:
            pts[i] = g2_point_words(P)
            if not g2_in_subgroup(P):
                st[i] = G2_NOT_IN_SUBGROUP
    return pts, st
