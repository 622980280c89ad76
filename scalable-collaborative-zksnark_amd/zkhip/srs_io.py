"""
Parameter-set bytes for plonk: a structured SRS read from a file and checked on the device, so that a prover never holds the trapdoor.

PolynomialCommitmentCub.new(be, s) builds powers_of_g from the trapdoor s in host memory: whoever runs it can forge any opening.  A
deployed prover loads an SRS somebody else made instead.  With L_k = powers_of_g[k] (2^k points) and the keys
powers_of_g2 = [g2, s_0 g2, .., s_{n-1} g2], for every k < n and j < 2^k

    (A)  L_k[j] = L_{k+1}[j] + L_{k+1}[j + 2^k]
    (B)  e(L_{k+1}[j + 2^k], g2) = e(L_k[j], s_{n-k-1} g2)

so the file carries only the top level L_n and the n + 1 keys; the lower levels are DERIVED by (A), and (B) is checked per level under
random weights rho: A_k = sum_j rho_j L_{k+1}[j + 2^k], B_k = sum_j rho_j L_k[j], e(A_k, g2) e(-B_k, s_{n-k-1} g2) = 1.  By induction from
L_0 = [g], (A) and (B) for all k give L_n[x] = eq(s, x) g for the s the keys define; an error escapes with probability about n / 2^128.

Layout (no length prefixes: the header fixes every length):

    header, 26 bytes:  magic "ZKPLSRS" + version byte (1) | two zero bytes | n u64 LE | eight zero bytes
    body: the 2^n points of L_n as 48-byte compressed G1, then the n + 1 keys as 96-byte compressed G2 (serialize.py)
    bytes = 26 + 48 2^n + 96 (n + 1)

There is ONE encoding per parameter set: parse_srs refuses a wrong magic or version, non-zero padding, n outside 1 .. 30 and any other
length.  The weights are rho_j = the low 128 bits of SHA-256(seed || u32le(1) || u64le(j)), the digest read as a little-endian integer
(its first 16 bytes), with seed = SHA-256(the whole file): nobody can choose points that depend on the weights.

What the check proves: the G1 points are consistent with the G2 keys, i.e. the file IS the SRS of the s its keys define, with every
point in its prime-order subgroup.  What it does NOT prove: that nobody knows s.  That is a property of how the file was made (a
ceremony), not of its bytes.
"""
from __future__ import annotations

import hashlib

import numpy as np

from . import pairing as pr
from . import proof_io as pio
from . import serialize as ser
from .field import Q_MOD, fq_from_mont

MAGIC = b"ZKPLSRS"
VERSION = 1
HEADER_BYTES = pio.HEADER_BYTES
MAX_N = 30
RHO_DOMAIN = 1  # ZK_SRS_CHECK_DOMAIN of include/zkhip.h
G1_INFINITY_REFUSED = 4
G1_STATUS_TEXT = {**ser.G1_STATUS_TEXT, G1_INFINITY_REFUSED: "the point at infinity"}
_FQ_RINV = pow(1 << 384, -1, Q_MOD)
_HALF_Q = (Q_MOD - 1) // 2


def srs_size(n: int) -> int:
    """the length in bytes of the encoding of an SRS of n variables: the formula of the module text"""
    return HEADER_BYTES + 48 * (1 << n) + 96 * (n + 1)


def rho(seed: bytes, count: int, domain: int = RHO_DOMAIN) -> list:
    """the weights of the check as integers: what zk_fr_hash_expand writes (there in Montgomery form)"""
    pre = bytes(seed) + int(domain).to_bytes(4, "little")
    return [int.from_bytes(hashlib.sha256(pre + j.to_bytes(8, "little")).digest()[:16], "little") for j in range(count)]


def file_seed(data) -> bytes:
    return hashlib.sha256(bytes(data)).digest()


def _compress_records(recs: np.ndarray) -> bytes:
    """[k, 12] affine Montgomery records (x = y = 0: infinity) -> k x 48 bytes"""
    out = bytearray()
    raw = np.ascontiguousarray(recs, dtype="<u8").reshape(-1, 12).tobytes()
    for i in range(len(raw) // 96):
        x = int.from_bytes(raw[96 * i:96 * i + 48], "little") * _FQ_RINV % Q_MOD
        y = int.from_bytes(raw[96 * i + 48:96 * i + 96], "little") * _FQ_RINV % Q_MOD
        if x == 0 and y == 0:
            out += ser.g1_serialize_compressed(None)
            continue
        b = bytearray(x.to_bytes(48, "big"))
        b[0] |= 0x80 | (0x20 if y > _HALF_Q else 0)
        out += b
    return bytes(out)


def _header(n: int) -> bytes:
    return MAGIC + bytes([VERSION, 0, 0]) + int(n).to_bytes(8, "little") + bytes(8)


def encode(top_level_points, keys) -> bytes:
    """host only: the 2^n affine points of L_n and the n + 1 G2 keys as python-int points (None: infinity) -> the file"""
    n = len(keys) - 1
    if n < 1 or n > MAX_N or len(top_level_points) != 1 << n:
        raise ValueError(f"{len(top_level_points)} points and {len(keys)} keys: not an SRS of 1 .. {MAX_N} variables")
    data = _header(n) + b"".join(ser.g1_serialize_compressed(P) for P in top_level_points) + b"".join(ser.g2_serialize_compressed(K) for K in keys)
    assert len(data) == srs_size(n)
    return data


def srs_to_bytes(be, pcs, powers_of_g2) -> bytes:
    """pcs: the levels 0 .. n of a parameter set (PolynomialCommitmentCub(..).mature()); powers_of_g2: its n + 1 keys as python-int points
    or [n + 1, 24] Montgomery records.  Only the top level and the keys are written"""
    from .vk_io import _g2_point_of_words, g2_records

    n = len(pcs) - 1
    keys = g2_records(powers_of_g2)
    if n < 1 or n > MAX_N or len(keys) != n + 1 or len(pcs[n]) != 1 << n:
        raise ValueError(f"{len(pcs)} levels and {len(keys)} G2 keys: not an SRS of 1 .. {MAX_N} variables")
    data = _header(n) + _compress_records(pcs[n].download()) + b"".join(ser.g2_serialize_compressed(_g2_point_of_words(w)) for w in keys)
    assert len(data) == srs_size(n)
    return data


def parse_srs(data):
    """bytes -> (n, points [2^n, 48] uint8, keys [n + 1, 96] uint8); host only.  ValueError for whatever is not the one encoding of some
    SRS, the points aside"""
    data = bytes(data)
    if len(data) < HEADER_BYTES:
        raise ValueError(f"{len(data)} bytes: shorter than the header")
    if data[:7] != MAGIC:
        raise ValueError("wrong magic")
    if data[7] != VERSION:
        raise ValueError(f"version {data[7]}, this reader knows {VERSION}")
    if any(data[8:10]) or any(data[18:26]):
        raise ValueError("non-zero padding in the header")
    n = int.from_bytes(data[10:18], "little")
    if n < 1 or n > MAX_N:
        raise ValueError(f"n = {n}: not in 1 .. {MAX_N}")
    want = srs_size(n)
    if len(data) != want:
        raise ValueError(f"{len(data)} bytes, the header's parameter set has {want}")
    pts = np.frombuffer(data, dtype=np.uint8, count=48 << n, offset=HEADER_BYTES).reshape(1 << n, 48)
    keys = np.frombuffer(data, dtype=np.uint8, count=96 * (n + 1), offset=HEADER_BYTES + (48 << n)).reshape(n + 1, 96)
    return n, pts, keys


def _bad_key(k_status, k_inf):
    for i, (s, inf) in enumerate(zip(k_status, k_inf)):
        if s:
            return f"G2 key {i}: {ser.G2_STATUS_TEXT[int(s)]}"
        if inf:
            return f"G2 key {i}: the point at infinity"
    return None


def level_message(k: int, n: int) -> str:
    """relation (B) between levels k and k + 1 failed: the upper level and the key s_{n-k-1} g2 = powers_of_g2[n - k] disagree"""
    return f"level {k + 1} does not match G2 key {n - k}"


def check_srs(be, pcs, powers_of_g2, seed: bytes) -> list:
    """the pairing step on a parameter set that is already loaded: ONE zk_srs_check call (2n MSMs in one batch, one pairing call of n
    groups) -> the messages of the levels that fail, lowest first (empty: every level passes).  The seed must not have been known to
    whoever chose the points: srs_from_bytes takes the SHA-256 of the file"""
    from .vk_io import g2_records

    n = len(pcs) - 1
    ok = be.srs_check(list(pcs), g2_records(powers_of_g2), seed)
    return [level_message(k, n) for k in range(n) if not ok[k]]


def srs_from_bytes(be, data, check: bool = True):
    """the parameter set of the bytes -> (pcs: the levels 0 .. n as Srs, powers_of_g2 [n + 1, 24] Montgomery records).  parse_srs, ONE
    host-to-device copy of the G1 block, ONE zk_g1_decompress_check_device call with infinity refused, ONE zk_g2_decompress_check,
    zk_srs_wrap_device, n zk_srs_halve calls, then check_srs seeded with the SHA-256 of the file (check=False skips only that pairing
    step).  ValueError names the cause: "G1 point 12345: not in the subgroup", "G2 key 3: ...", "level 7 does not match G2 key 14" """
    from .api import ZkError

    n, pts, keys = parse_srs(data)
    d_in, d_rec, levels = be.to_device(pts), None, []
    try:
        d_rec, (bad, first, status) = be.g1_decompress_check_device(d_in, 1 << n, refuse_infinity=True)
        if bad:
            raise ValueError(f"G1 point {first}: {G1_STATUS_TEXT[status]}")
        k_pts, k_st = be.g2_decompress_check(keys)
        msg = _bad_key(k_st, ~k_pts.any(axis=1))
        if msg:
            raise ValueError(msg)
        levels.append(be.srs_wrap_device(d_rec, 1 << n))
        for k in range(n, 0, -1):
            try:
                levels.append(be.srs_halve(levels[-1]))
            except ZkError as e:
                raise ValueError(f"level {k - 1}: " + str(e).split("zk_srs_halve: ", 1)[-1]) from None
        if check:
            failed = check_srs(be, levels[::-1], k_pts, file_seed(data))
            if failed:
                raise ValueError(failed[0])
    except BaseException:  # a refused file leaves nothing on the device
        for lv in levels:
            lv.free()
        raise
    finally:
        d_in.free()
        if d_rec is not None:
            d_rec.free()
    pcs = levels[::-1]
    return pcs, k_pts.copy()


def restrict(pcs, powers_of_g2, nvars: int):
    """the parameter set of the LAST nvars trapdoor coordinates: levels 0 .. nvars and the keys [g2, s_{n-nvars}, .., s_{n-1}] -- what
    preprocess needs for a circuit with mu + 1 = nvars <= n (level k is the eq basis over s_{n-k} .. s_{n-1}): one file serves every
    smaller circuit"""
    n = len(pcs) - 1
    if nvars < 0 or nvars > n or len(powers_of_g2) != n + 1:
        raise ValueError(f"{nvars} variables of a parameter set of {n} with {len(powers_of_g2)} keys")
    keys = powers_of_g2
    sub = [keys[0]] + [keys[1 + i] for i in range(n - nvars, n)]
    return list(pcs[:nvars + 1]), (np.stack(sub) if isinstance(keys, np.ndarray) else sub)


# ---- the same verdict in Python integers (tiny n, the tests, callers without a device) ----
def halve_points(level: list) -> list:
    m = len(level) // 2
    return [pr.g1_add(level[j], level[j + m]) for j in range(m)]


def _lincomb(points, weights):
    acc = None
    for P, w in zip(points, weights):
        acc = pr.g1_add(acc, pr.g1_mul(P, w))
    return acc


def levels_check_host(levels: list, keys: list, seed: bytes) -> list:
    """relation (B) on python-int levels 0 .. n and keys: the messages of check_srs"""
    n = len(levels) - 1
    w = rho(seed, 1 << (n - 1))
    out = []
    for k in range(n):
        h = 1 << k
        A, B, key = _lincomb(levels[k + 1][h:], w[:h]), _lincomb(levels[k], w[:h]), keys[n - k]
        if A is None or B is None or key is None or keys[0] is None or not pr.pairing_product_is_one([(A, keys[0]), (pr.g1_neg(B), key)]):
            out.append(level_message(k, n))
    return out


def srs_check_host(data) -> list:
    """srs_from_bytes' verdict without a device: [] when the file is accepted, otherwise the messages -- ONE for a bad point, a bad key
    or a sum at infinity (the loader stops there too), or one per failing level, lowest first.  ValueError from parse_srs for a file
    that is no encoding.  Python integers and zkhip/pairing.py: for tiny n"""
    n, pts, keys = parse_srs(data)
    top = []
    for i in range(1 << n):
        p18, st = ser.g1_decompress_check_host(pts[i].tobytes())
        if st[0]:
            return [f"G1 point {i}: {G1_STATUS_TEXT[int(st[0])]}"]
        if not p18[0, 12:].any():
            return [f"G1 point {i}: {G1_STATUS_TEXT[G1_INFINITY_REFUSED]}"]
        top.append((fq_from_mont(p18[0, :6]), fq_from_mont(p18[0, 6:12])))
    k_pts, k_st = ser.g2_decompress_check_host(keys)
    msg = _bad_key(k_st, ~k_pts.any(axis=1))
    if msg:
        return [msg]
    from .vk_io import _g2_point_of_words

    levels = [top]
    for k in range(n, 0, -1):
        nxt = halve_points(levels[-1])
        inf = [j for j, P in enumerate(nxt) if P is None]
        if inf:
            return [f"level {k - 1}: {len(inf)} of {len(nxt)} sums are the point at infinity; the first is sum {inf[0]}"]
        levels.append(nxt)
    return levels_check_host(levels[::-1], [_g2_point_of_words(w) for w in k_pts], file_seed(data))
