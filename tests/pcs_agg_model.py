"""
The model of the aggregated PCS verification (include/zkhip.h: zk_g1_lincomb_seg, zk_pcs_agg_weights, zk_pcs_verify_agg) in Python
integers, for tests/test_pcs_agg.py, tests/test_gpu_g1seg.py and tests/test_gpu_pcs_agg.py.

  * affine G1 arithmetic by the chord-and-tangent rule (None is infinity) -- neither the XYZZ formulas of the kernel nor the projective
    ones of g1check_model.py;
  * the segmented sum out[s] = sum_{starts[s] <= t < starts[s+1]} k_t P_t;
  * the weight derivation on hashlib, from the stated byte string;
  * the term list of the aggregate: segment 0 is L, segment j is M_j.  It treats points as opaque values, so the same list serves
    curve points (the segmented sum) and discrete logarithms (the aggregate equation in the exponent, with the trapdoor).
"""
import hashlib

import numpy as np

Q = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
G = (0x17F1D3A73197D7942695638C4FA9AC0FC3688C4F9774B905A14E3A3F171BAC586C55E83FF97A1AEFFB3AF00ADB22C6BB,
     0x08B3F481E3AAA0F1A09E30ED741D8AE4FCF5E095D5D00AF600DB18CB2C04B3EDD03CC744A2888AE40CAA232946C5E7E1)
LABEL = b"zkhip-pcs-agg-v1"


# ---- affine G1 ----
def neg(P):
    return None if P is None else (P[0], (-P[1]) % Q)


def add(P, S):
    if P is None:
        return S
    if S is None:
        return P
    if P[0] == S[0]:
        if (P[1] + S[1]) % Q == 0:
            return None
        lam = 3 * P[0] * P[0] * pow(2 * P[1], -1, Q) % Q
    else:
        lam = (S[1] - P[1]) * pow(S[0] - P[0], -1, Q) % Q
    x = (lam * lam - P[0] - S[0]) % Q
    return (x, (lam * (P[0] - x) - P[1]) % Q)


def mul(P, k: int):
    acc = None
    for bit in bin(k)[2:] if k else "":
        acc = add(acc, acc)
        if bit == "1":
            acc = add(acc, P)
    return acc


def seg_sum(starts, points, scalars):
    """points: affine (or None), scalars: integers -> one affine point (or None) per segment"""
    out = []
    for s in range(len(starts) - 1):
        acc = None
        for t in range(starts[s], starts[s + 1]):
            acc = add(acc, mul(points[t], scalars[t]))
        out.append(acc)
    return out


# ---- records ----
def _mont_words(v: int):
    return [((v << 384) % Q >> (64 * i)) & (2**64 - 1) for i in range(6)]


def words(P) -> np.ndarray:
    """the normalised Jacobian record: (x, y, 1), (1, 1, 0) for infinity, Montgomery form (radix 2^384)"""
    return np.array(_mont_words(1) * 2 + [0] * 6 if P is None else _mont_words(P[0]) + _mont_words(P[1]) + _mont_words(1), dtype=np.uint64)


def jac_words(P, z: int) -> np.ndarray:
    """the representative (x z^2, y z^3, z) of an affine point"""
    return np.array(_mont_words(P[0] * z * z % Q) + _mont_words(P[1] * z**3 % Q) + _mont_words(z % Q), dtype=np.uint64)


def raw_words(X: int, Y: int, Z: int) -> np.ndarray:
    """three integers below 2^384 as they stand (no reduction: a coordinate >= q stays one)"""
    return np.array([(v >> (64 * i)) & (2**64 - 1) for v in (X, Y, Z) for i in range(6)], dtype=np.uint64)


def canon_limbs(k: int) -> np.ndarray:
    return np.array([(k >> (64 * i)) & (2**64 - 1) for i in range(4)], dtype=np.uint64)


def fr_mont(x: int) -> np.ndarray:
    return canon_limbs((x << 256) % R)


def fr_ints(a) -> list:
    """[n, 4] Montgomery limbs -> integers"""
    rinv = pow(1 << 256, -1, R)
    return [sum(int(w) << (64 * i) for i, w in enumerate(row)) * rinv % R for row in np.asarray(a, dtype=np.uint64).reshape(-1, 4)]


# ---- the weights ----
def _le(a) -> bytes:
    return np.ascontiguousarray(a, dtype="<u8").tobytes()


def weights(nvars, skip, cstart, cpoints, cscalars, values, proofs, points) -> list:
    """rho_k as integers below 2^128, from the arrays of zk_pcs_agg_weights"""
    count = len(nvars)
    cp, ce = np.asarray(cpoints, dtype=np.uint64).reshape(-1, 18), np.asarray(cscalars, dtype=np.uint64).reshape(-1, 4)
    vals = np.asarray(values, dtype=np.uint64).reshape(-1, 4)
    pf, pts = np.asarray(proofs, dtype=np.uint64).reshape(-1, 18), np.asarray(points, dtype=np.uint64).reshape(-1, 4)
    h = hashlib.sha256(LABEL + count.to_bytes(8, "little"))
    row = 0
    for k in range(count):
        nv, c0, c1 = int(nvars[k]), int(cstart[k]), int(cstart[k + 1])
        h.update(nv.to_bytes(8, "little") + int(skip[k]).to_bytes(8, "little") + (c1 - c0).to_bytes(8, "little"))
        h.update(_le(cp[c0:c1]) + _le(ce[c0:c1]) + _le(vals[k]) + _le(pf[row:row + nv]) + _le(pts[row:row + nv]))
        row += nv
    seed = h.digest()
    return [int.from_bytes(hashlib.sha256(seed + k.to_bytes(8, "little")).digest()[:16], "little") for k in range(count)]


def weights_array(rho) -> np.ndarray:
    return np.array([[r & (2**64 - 1), r >> 64] for r in rho], dtype=np.uint64).reshape(-1, 2)


# ---- the term list ----
def term_list(n_g2: int, openings, rho, g1):
    """openings: [(nvars, skip, [(C, e)], v, [pi_i], [u_i])] with e, v, u integers and C, pi opaque points; rho: integers; g1: the
    point of the key.  -> (starts [n_g2 + 1], points, scalars): segment 0 = L -- per opening its commitment terms (rho e), then its
    proof points (rho u) --, then g1 with -sum rho v; segment j >= 1 = M_j: rho_k pi_{k, j-1-skip_k} in the order of the openings"""
    segs = [[] for _ in range(n_g2)]
    vsum = 0
    for (nv, sk, cterms, v, pis, us), r in zip(openings, rho):
        assert 1 + sk + nv <= n_g2 and len(pis) == nv and len(us) == nv
        segs[0] += [(C, r * e % R) for C, e in cterms]
        segs[0] += [(p, r * u % R) for p, u in zip(pis, us)]
        for i, p in enumerate(pis):
            segs[1 + sk + i].append((p, r % R))
        vsum = (vsum + r * v) % R
    segs[0].append((g1, (-vsum) % R))
    starts = [0]
    for s in segs:
        starts.append(starts[-1] + len(s))
    return starts, [p for s in segs for p, _ in s], [k for s in segs for _, k in s]


def aggregate_holds_in_exponent(s_keys, openings, rho) -> bool:
    """the aggregate equation with every point given as its discrete logarithm to the base g1 (so g1 is 1) and powers_g2[j] =
    s_keys[j - 1] g2:  e(L, g2) prod_j e(-M_j, powers_g2[j]) == 1  <=>  L - sum_j s_{j-1} M_j == 0 (mod r)"""
    n_g2 = len(s_keys) + 1
    starts, pts, ks = term_list(n_g2, openings, rho, 1)
    sums = [sum(p * k for p, k in zip(pts[starts[j]:starts[j + 1]], ks[starts[j]:starts[j + 1]])) % R for j in range(n_g2)]
    return (sums[0] - sum(s * m for s, m in zip(s_keys, sums[1:]))) % R == 0
