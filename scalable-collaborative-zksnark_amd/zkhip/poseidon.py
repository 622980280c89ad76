"""
Poseidon over BLS12-381 Fr: the permutation, the 2-to-1 hash and a Merkle tree of it -- on the device (zk_poseidon_*, csrc/zk_poseidon.hip),
on the host in python integers (the *_host functions: the rule itself, for checks and small inputs), and as a circuit of the wide gate
built with zkhip.circuit (permutation_gadget, merkle_circuit): "I know a leaf and a path to this public root", generated, proved and
verified by the plonk module as it stands.

THE RULE (the same in include/zkhip.h and host/zkhost/poseidon.hpp).  Width t = 3 (capacity 1, rate 2), S-box x^5, rf full rounds (rf / 2
first, rf / 2 last) around rp partial rounds.  The state is (s_0, s_1, s_2); one counter k indexes all rf + rp rounds:
    full round k      s_i += rc[3k + i] for i = 0, 1, 2;  every s_i <- s_i^5;  s <- M s
    partial round k   s_i += rc[3k + i] for i = 0, 1, 2;  only  s_0 <- s_0^5;  s <- M s
    hash2(l, r) = permute(0, l, r)[0];   a Merkle node = hash2(left child, right child)
A tree of n = 2^k leaves is a list of 2n - 1 elements in the order of zk_product_tree's levels: the leaves, then n / 2 nodes, .., the root
at index 2n - 2.

THE INSTANCE "zkhip-poseidon-v1": rf = 8, rp = 57 (the Poseidon paper's round counts for a prime of about 255 bits, t = 3, alpha = 5,
128-bit security -- restated, not re-derived here),
    rc[k] = int_le( SHA-256(tag || u32le(k) || 0x00) || SHA-256(tag || u32le(k) || 0x01) ) mod r,  k < 195,  tag = b"zkhip-poseidon-v1"
    M[i][j] = 1 / (i + j + 3):  a Cauchy matrix on x = 0, 1, 2 and y = 3, 4, 5, hence MDS (every square submatrix is invertible).
It is SELF-DEFINED: not claimed to equal the constants of any other library, and the paper's further checks of the matrix
(invariant-subspace trails) have NOT been done on it.  That is why every function here takes the constants as a parameter (`p`, default
params()) and the kernels take them as a parameter object: another instance is other data, not other code.

THE CIRCUIT.  permutation_gadget folds a round's constant addition into the qC of the previous linear layer's rows; the first round's
constants take three `lin` rows.  A full round is 3 pow5 rows + 3 outputs x 2 lin rows = 9 rows, a partial round 1 + 6 = 7 rows, the v1
permutation 3 + 8 * 9 + 57 * 7 = 474 rows.  merkle_circuit(depth): one public input (the root); private: the leaf, `depth` siblings, `depth`
bits.  Per level: assert_bool(bit), d = sib - cur, e = bit d, left = cur + e, right = sib - e (bit = 1: the running node is the RIGHT
child), a constant-0 row, the permutation on (0, left, right): 480 rows.  After the last level the output is put into the public
root's copy class.  Depth 1 has 481 rows (mu = 9), depth 2 has 961 (mu = 10).
"""
from __future__ import annotations

import ctypes
import hashlib

import numpy as np

from ._lib import ZK_ERR_INVALID
from .api import _h, _ptr
from .field import R_MOD, fr_mont

TAG = b"zkhip-poseidon-v1"
RF, RP = 8, 57

_params = None


def params() -> dict:
    """the v1 instance: {"rf", "rp", "rc": 195 ints, "mds": 3 x 3 ints, "rc_mont": [195, 4], "mds_mont": [9, 4] (row-major) u64 Montgomery limbs}"""
    global _params
    if _params is None:
        sha = lambda k, b: hashlib.sha256(TAG + k.to_bytes(4, "little") + bytes([b])).digest()
        rc = [int.from_bytes(sha(k, 0) + sha(k, 1), "little") % R_MOD for k in range(3 * (RF + RP))]
        mds = [[pow(i + j + 3, -1, R_MOD) for j in range(3)] for i in range(3)]
        _params = make_params(RF, RP, rc, mds)
    return _params


def make_params(rf: int, rp: int, rc, mds) -> dict:
    """a params dict of any instance at t = 3 from its integers (rc: 3 (rf + rp), mds: 3 x 3)"""
    rc, mds = [int(x) % R_MOD for x in rc], [[int(x) % R_MOD for x in row] for row in mds]
    if len(rc) != 3 * (rf + rp) or len(mds) != 3 or any(len(row) != 3 for row in mds):
        raise ValueError("3 (rf + rp) round constants and a 3 x 3 matrix are needed")
    return {"rf": rf, "rp": rp, "rc": rc, "mds": mds, "rc_mont": np.stack([fr_mont(x) for x in rc]),
            "mds_mont": np.stack([fr_mont(x) for row in mds for x in row])}


# ---- the rule on the host ----
def permute_host(state, p: dict | None = None) -> tuple:
    p = p or params()
    half, rp, rc, m = p["rf"] // 2, p["rp"], p["rc"], p["mds"]
    s = [int(x) % R_MOD for x in state]
    for k in range(p["rf"] + rp):
        s = [(s[i] + rc[3 * k + i]) % R_MOD for i in range(3)]
        s[0] = pow(s[0], 5, R_MOD)
        if k < half or k >= half + rp:
            s[1], s[2] = pow(s[1], 5, R_MOD), pow(s[2], 5, R_MOD)
        s = [(m[i][0] * s[0] + m[i][1] * s[1] + m[i][2] * s[2]) % R_MOD for i in range(3)]
    return tuple(s)


def hash2_host(left: int, right: int, p: dict | None = None) -> int:
    return permute_host((0, left, right), p)[0]


def merkle_host(leaves, p: dict | None = None) -> list:
    """the 2n - 1 elements of the tree of n = 2^k leaves (module text)"""
    n = len(leaves)
    if n == 0 or n & (n - 1):
        raise ValueError("the number of leaves must be a power of two")
    tree = [int(x) % R_MOD for x in leaves]
    lo, cnt = 0, n
    while cnt > 1:
        tree += [hash2_host(tree[lo + 2 * i], tree[lo + 2 * i + 1], p) for i in range(cnt // 2)]
        lo, cnt = lo + cnt, cnt // 2
    return tree


def merkle_path(tree, n: int, index: int) -> tuple:
    """(siblings, bits) of leaf `index` in a tree of n leaves, from the leaf level up: bits[0] belongs to the leaf level, and bit = 1 means the
    running node is the right child"""
    if not 0 <= index < n:
        raise ValueError("no such leaf")
    sibs, bits, lo, cnt = [], [], 0, n
    while cnt > 1:
        sibs.append(tree[lo + (index ^ 1)])
        bits.append(index & 1)
        lo, cnt, index = lo + cnt, cnt // 2, index >> 1
    return sibs, bits


def path_root_host(leaf: int, siblings, bits, p: dict | None = None) -> int:
    cur = leaf
    for sib, bit in zip(siblings, bits):
        cur = hash2_host(sib, cur, p) if bit else hash2_host(cur, sib, p)
    return cur


# ---- the device ----
class Poseidon:
    """zk_poseidon_params of one instance on one Ctx, with the three device calls.  Arguments that name device memory are what Ctx takes
    (DeviceBuffer, view, address); Fr are Montgomery, fully reduced.  A refusal of the library (ZK_ERR_INVALID): ValueError with its message."""

    def __init__(self, be, p: dict | None = None):
        self.be, self.p, self.h = be, p or params(), 0
        rc, mds = np.ascontiguousarray(self.p["rc_mont"], dtype=np.uint64), np.ascontiguousarray(self.p["mds_mont"], dtype=np.uint64)
        h = ctypes.c_void_p()
        self._check(be.lib.zk_poseidon_params_create(be.h, int(self.p["rf"]), int(self.p["rp"]), _h(rc), _h(mds), ctypes.byref(h)))
        self.h = h.value

    def _check(self, rc: int):
        if rc == ZK_ERR_INVALID:
            raise ValueError((self.be.lib.zk_last_error(self.be.h) or b"").decode())
        self.be._check(rc)

    def permute(self, states, n: int, out=None):
        """out[i] = permute(states[i]) on n states of three Fr (asynchronous); out may be `states` itself (default: a new buffer)"""
        out = out or self.be.alloc(max(96 * n, 1))
        self._check(self.be.lib.zk_poseidon_permute(self.be.h, self.h, _ptr(states), _ptr(out), n))
        return out

    def hash2(self, left, right, n: int, out=None):
        """out[i] = hash2(left[i], right[i]), n Fr each (asynchronous); out may be left or right"""
        out = out or self.be.alloc(max(32 * n, 1))
        self._check(self.be.lib.zk_poseidon_hash2(self.be.h, self.h, _ptr(left), _ptr(right), _ptr(out), n))
        return out

    def merkle(self, leaves, n: int, out=None):
        """the tree of n = 2^k leaves: 2n - 1 Fr, the root last (asynchronous)"""
        out = out or self.be.alloc(32 * max(2 * n - 1, 1))
        self._check(self.be.lib.zk_poseidon_merkle(self.be.h, self.h, _ptr(leaves), n, _ptr(out)))
        return out

    def free(self):
        if self.h and getattr(self.be, "h", None):
            self.be.lib.zk_poseidon_params_free(self.h)
        self.h = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


# ---- the circuit ----
def permutation_gadget(b, state, p: dict | None = None) -> tuple:
    """the permutation on three variables of a circuit.Builder -> its three output variables (row counts: module text)"""
    p = p or params()
    half, rp, rc, m = p["rf"] // 2, p["rp"], p["rc"], p["mds"]
    rounds = p["rf"] + rp
    s = [b.lin(1, state[i], 0, None, rc[i]) for i in range(3)]
    for k in range(rounds):
        full = k < half or k >= half + rp
        u = [b.pow5(s[0]), b.pow5(s[1]) if full else s[1], b.pow5(s[2]) if full else s[2]]
        nxt = rc[3 * (k + 1):3 * (k + 2)] if k + 1 < rounds else (0, 0, 0)
        s = [b.lin(1, b.lin(m[i][0], u[0], m[i][1], u[1], 0), m[i][2], u[2], nxt[i]) for i in range(3)]
    return tuple(s)


def merkle_circuit(depth: int, p: dict | None = None):
    """-> (circuit, layout, vars): the circuit dict of "leaf, siblings and bits hash up to the public root" as preprocess / witness_plan take
    it, the builder's layout, and vars = {"root", "leaf", "siblings": [depth], "bits": [depth], "out": the last hash's output variable}"""
    from .circuit import Builder

    if depth < 1:
        raise ValueError("depth >= 1 is needed")
    b = Builder()
    root = b.public()
    leaf = b.private()
    sibs, bits = [b.private() for _ in range(depth)], [b.private() for _ in range(depth)]
    cur = leaf
    for sib, bit in zip(sibs, bits):
        b.assert_bool(bit)
        d = b.lin(1, sib, -1, cur, 0)
        e = b.mul(bit, d)
        left, right = b.lin(1, cur, 1, e, 0), b.lin(1, sib, -1, e, 0)
        zero = b.lin(0, None, 0, None, 0)
        cur = permutation_gadget(b, (zero, left, right), p)[0]
    b.assert_equal(cur, root)
    circuit, layout = b.build()
    return circuit, layout, {"root": root, "leaf": leaf, "siblings": sibs, "bits": bits, "out": cur}


def merkle_witness_inputs(layout, vars: dict, leaf: int, siblings, bits) -> np.ndarray:
    """the `free` array ([3N, 4] Montgomery Fr) of plonk.witness for one path: integers, bits as 0 / 1 (any integer is stored as given)"""
    if len(siblings) != len(vars["siblings"]) or len(bits) != len(vars["bits"]):
        raise ValueError("the path does not have the circuit's depth")
    values = {vars["leaf"]: leaf}
    values.update(zip(vars["siblings"], siblings))
    values.update(zip(vars["bits"], bits))
    return layout.free(values)
