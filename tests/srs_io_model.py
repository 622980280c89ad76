"""
The model of the parameter-set file (zkhip/srs_io.py, csrc/zk_srsio.hip) in Python integers, for tests/test_srs_io.py and
tests/test_gpu_srs_io.py.

Levels are built from the trapdoor by the DEFINITION (exponents E_0 = [1], E_{k+1} = E_k (1 - s) ++ E_k s, one scalar multiplication per
point) with the complete projective addition of tests/g1check_model.py, so they share no formula with the device's fixed-base tables or
with the affine arithmetic of zkhip/pairing.py.  The verdict checks relations (A) and (B) POINT BY POINT -- no weights -- so it is what
the weighted check must agree with except with probability about n / 2^128.  The only thing borrowed from the product is the pairing
itself (zkhip/pairing.py, tested on its own in tests/test_pairing.py).
"""
import functools
import hashlib

import g1check_model as gm
from zkhip import pairing as pr

R = gm.R


def exponents(s):
    """[E_0, .., E_n] for the trapdoor s = [s_0, .., s_{n-1}] (canonical integers)"""
    n, out = len(s), [[1]]
    for k in range(n):
        t = s[n - k - 1] % R
        out.append([e * (1 - t) % R for e in out[-1]] + [e * t % R for e in out[-1]])
    return out


def levels(s, g=gm.G):
    return [[gm.mul(g, e) for e in E] for E in exponents(s)]


def keys(s):
    return pr.powers_of_g2([x % R for x in s])


def halve(level):
    m = len(level) // 2
    return [gm.add(level[j], level[j + m]) for j in range(m)]


def derive(top):
    """levels 0 .. n from the top level by relation (A)"""
    out = [list(top)]
    while len(out[-1]) > 1:
        out.append(halve(out[-1]))
    return out[::-1]


def rho(seed: bytes, count: int, domain: int = 1):
    """the first 16 bytes of SHA-256(seed || u32le(domain) || u64le(j)) as a little-endian integer"""
    return [int.from_bytes(hashlib.sha256(seed + domain.to_bytes(4, "little") + j.to_bytes(8, "little")).digest()[:16], "little") for j in range(count)]


def rho_mont_words(seed: bytes, count: int, domain: int = 1):
    """what zk_fr_hash_expand writes: count x 4 u64, Montgomery form (radix 2^256)"""
    import numpy as np

    out = np.zeros((count, 4), dtype=np.uint64)
    for j, v in enumerate(rho(seed, count, domain)):
        m = (v << 256) % R
        out[j] = [(m >> (64 * i)) & (2**64 - 1) for i in range(4)]
    return out


def failing_levels(lv, ks):
    """the k < n at which (B) fails for SOME j: e(L_{k+1}[j + 2^k], g2) != e(L_k[j], ks[n - k]); lv must satisfy (A) (derive)"""
    n, out = len(lv) - 1, []
    for k in range(n):
        h = 1 << k
        if not all(pr.pairing_product_is_one([(lv[k + 1][j + h], ks[0]), (gm.neg(lv[k][j]), ks[n - k])]) for j in range(h)):
            out.append(k)
    return out


@functools.lru_cache(maxsize=None)
def sample(n: int, seed: int = 5):
    """(s, levels, keys) of a seeded trapdoor"""
    import random

    rng = random.Random(1000 * seed + n)
    s = tuple(rng.randrange(2, R) for _ in range(n))
    return s, levels(s), keys(s)
