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

A TREE KEPT ON THE DEVICE.  Poseidon.paths / roots / verify_paths / update open many leaves, hash many paths up to their roots and apply a
batch of leaf writes to the tree in place, touching only the nodes above the written leaves (zk_poseidon_merkle_paths / _roots / _update;
paths_host and update_host are the same rules on python integers, with the same refusals).  The bits of a path are the bits of its index.
merkle_update_circuit(depth, count) is the statement "the tree with public root R became the tree with public root R' by `count` leaf
writes, one after another, and nothing else changed": two public inputs (old root, new root); private, per write: old leaf, new leaf,
`depth` siblings, `depth` bits.  Per level ONE assert_bool(bit) row, then the level of merkle_circuit without its assertion (d, e, left,
right, the constant 0, the permutation: 5 + 474 = 479 rows) twice -- on the old running node and on the new one, against the SAME sibling
and bit variables: 1 + 2 * 479 = 959 rows per level, 959 depth per write, 2 + 959 depth count in all.  The old chain of the first write is
put into the old root's copy class, the old chain of every later write into the class of the new chain before it, the last new chain
into the new root's.  (depth, count) = (1, 1) has 961 rows (mu = 10), (2, 1) has 1920 (mu = 11), (2, 2) has 3838 (mu = 12).
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


def _tree_depth(tree, n: int) -> int:
    if n < 1 or n & (n - 1) or len(tree) != 2 * n - 1:
        raise ValueError("a tree of n = 2^d leaves has 2n - 1 elements")
    return n.bit_length() - 1


def _refuse_not_below(what: str, indices, limit: int, text: str):
    """the library's refusal of indices >= limit, with its message"""
    bad = [k for k, i in enumerate(indices) if not 0 <= i < limit]
    if bad:
        raise ValueError(f"{what}: {len(bad)} of {len(indices)} indices {text}; the first is position {bad[0]}")


def paths_host(tree, n: int, indices) -> list:
    """the sibling lists of zk_poseidon_merkle_paths: one list of d siblings per index, from the leaf level up (the bits are the index's)"""
    _tree_depth(tree, n)
    indices = [int(i) for i in indices]
    _refuse_not_below("zk_poseidon_merkle_paths", indices, n, f"are not below n = {n}")
    return [merkle_path(tree, n, i)[0] for i in indices]


def update_host(tree, n: int, writes, p: dict | None = None) -> list:
    """a NEW tree list: the leaf writes (index, value) applied in order -- any order, repeats allowed, the last write of a leaf wins -- and
    only the nodes above a written leaf hashed again (zk_poseidon_merkle_update after the wrapper's sort)"""
    d = _tree_depth(tree, n)
    writes = [(int(i), int(v) % R_MOD) for i, v in writes]
    _refuse_not_below("zk_poseidon_merkle_update", [i for i, _ in writes], n, f"are not below n = {n}")
    out = list(tree)
    for i, v in writes:
        out[i] = v
    touched, lo = sorted({i for i, _ in writes}), 0
    for j in range(d):
        touched = sorted({i >> 1 for i in touched})
        for q in touched:
            out[lo + (n >> j) + q] = hash2_host(out[lo + 2 * q], out[lo + 2 * q + 1], p)
        lo += n >> j
    return out


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

    # ---- a tree kept on the device (zk_poseidon_merkle_paths / _roots / _update).  Indices are host integers; the library validates them ----
    @staticmethod
    def _indices(indices) -> np.ndarray:
        return np.ascontiguousarray(np.asarray(indices, dtype=np.uint64).reshape(-1))

    def paths(self, tree, n: int, indices, out=None):
        """the sibling paths of the leaves `indices` (any order, repeats allowed) of the device tree of n leaves: [count][d] Fr, path k contiguous
        from the leaf level up (asynchronous).  The bits of path k are the bits of indices[k]"""
        idx = self._indices(indices)
        out = out or self.be.alloc(max(32 * len(idx) * max(int(n).bit_length() - 1, 0), 1))
        self._check(self.be.lib.zk_poseidon_merkle_paths(self.be.h, _ptr(tree), n, _h(idx), len(idx), _ptr(out)))
        return out

    def roots(self, leaves, indices, siblings, depth: int, out=None):
        """out[k] = the root that leaf k reaches through siblings[k][0 .. depth) with the bits of indices[k] (asynchronous); out may be `leaves`"""
        idx = self._indices(indices)
        out = out or self.be.alloc(max(32 * len(idx), 1))
        self._check(self.be.lib.zk_poseidon_merkle_roots(self.be.h, self.h, _ptr(leaves), _h(idx), _ptr(siblings), depth, len(idx), _ptr(out)))
        return out

    def verify_paths(self, root: int, leaves, indices, siblings, depth: int) -> np.ndarray:
        """a boolean per path: does it reach `root` (a canonical integer)?  Blocking: the roots are read back"""
        count = len(self._indices(indices))
        got = self.roots(leaves, indices, siblings, depth).download((count, 4))
        return (got == fr_mont(int(root) % R_MOD).reshape(1, 4)).all(axis=1)

    def update(self, tree, n: int, indices, values):
        """tree[indices[k]] = values[k], then the nodes above the written leaves are hashed again, in place (asynchronous).  values: a host
        [count, 4] array of Montgomery limbs -- the indices may then come in any order and repeat, the LAST write of a leaf wins (a stable
        numpy sort, then the library's strictly ascending form); or device memory, which is handed to the library as it is, so the indices
        must already ascend strictly"""
        idx = self._indices(indices)
        if isinstance(values, np.ndarray):
            values = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1, 4)
            if len(values) != len(idx):
                raise ValueError("one value per index is needed")
            order = np.argsort(idx, kind="stable")
            last = np.ones(len(idx), dtype=bool)
            last[:-1] = idx[order][1:] != idx[order][:-1]
            order = order[last]
            idx, values = np.ascontiguousarray(idx[order]), self.be.to_device(values[order])
        self._check(self.be.lib.zk_poseidon_merkle_update(self.be.h, self.h, _ptr(tree), n, _h(idx), _ptr(values), len(idx)))
        return tree

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


def _merkle_level(b, cur, sib, bit, p):
    """the rows of one level after the bit's assertion: left / right selected by the bit, then the hash -- 5 + permutation rows"""
    d = b.lin(1, sib, -1, cur, 0)
    e = b.mul(bit, d)
    left, right = b.lin(1, cur, 1, e, 0), b.lin(1, sib, -1, e, 0)
    zero = b.lin(0, None, 0, None, 0)
    return permutation_gadget(b, (zero, left, right), p)[0]


def merkle_update_circuit(depth: int, count: int = 1, p: dict | None = None):
    """-> (circuit, layout, vars) of "`count` chained leaf writes take the public old root to the public new root" (module text).
    vars = {"old_root", "new_root", "writes": [count x {"old_leaf", "new_leaf", "siblings": [depth], "bits": [depth], "old_out", "new_out"}]}"""
    from .circuit import Builder

    if depth < 1 or count < 1:
        raise ValueError("depth >= 1 and count >= 1 are needed")
    b = Builder()
    old_root, new_root = b.public(), b.public()
    writes = []
    for _ in range(count):
        w = {"old_leaf": b.private(), "new_leaf": b.private()}
        w["siblings"], w["bits"] = [b.private() for _ in range(depth)], [b.private() for _ in range(depth)]
        writes.append(w)
    prev = None
    for i, w in enumerate(writes):
        old, new = w["old_leaf"], w["new_leaf"]
        for sib, bit in zip(w["siblings"], w["bits"]):
            b.assert_bool(bit)
            old = _merkle_level(b, old, sib, bit, p)
            new = _merkle_level(b, new, sib, bit, p)
        b.assert_equal(old, old_root if i == 0 else prev)
        w["old_out"], w["new_out"] = old, new
        prev = new
    b.assert_equal(prev, new_root)
    circuit, layout = b.build()
    return circuit, layout, {"old_root": old_root, "new_root": new_root, "writes": writes}


def merkle_update_inputs(layout, vars: dict, steps) -> np.ndarray:
    """the `free` array of plonk.witness for a chain of writes: steps = one (old_leaf, new_leaf, siblings, bits) per write, integers"""
    steps = list(steps)
    if len(steps) != len(vars["writes"]):
        raise ValueError("the chain does not have the circuit's number of writes")
    values = {}
    for w, (old_leaf, new_leaf, siblings, bits) in zip(vars["writes"], steps):
        if len(siblings) != len(w["siblings"]) or len(bits) != len(w["bits"]):
            raise ValueError("the path does not have the circuit's depth")
        values[w["old_leaf"]], values[w["new_leaf"]] = old_leaf, new_leaf
        values.update(zip(w["siblings"], siblings))
        values.update(zip(w["bits"], bits))
    return layout.free(values)


def merkle_transfer_circuit(depth: int, bits: int = 64, p: dict | None = None):
    """-> (circuit, layout, vars) of "the tree with public root R became the tree with public root R' by moving a private non-zero amount
    from one leaf to another; the amount and both new balances lie below 2^bits".  merkle_update_circuit with count = 2, except that the
    new leaves are COMPUTED: after the private variables come the rows
        amt = amount (a lin copy: to_bits wants a computed value), new_from = old_from - amt, new_to = old_to + amt,
        assert_nonzero(amt), assert_range(amt, bits), assert_range(new_from, bits), assert_range(new_to, bits)
    -- 3 + 2 + 3 (3 bits - 1) rows -- and then the two writes' levels.  An amount above the sender's balance wraps new_from round r, far
    above 2^bits.  Every inverse and every bit is advice (circuit.Builder), generated on the device: the caller gives balances, amount
    and paths only.  The old balances are not range-checked: that they lie below 2^bits is the invariant the statement keeps.
    vars = {"old_root", "new_root", "amount", "writes": [2 x {"old_leaf", "new_leaf", "siblings", "bits", "old_out", "new_out"}]} (write
    0: the sender, write 1: the receiver, whose path is one of the tree AFTER write 0)"""
    from .circuit import Builder

    if depth < 1 or not 1 <= bits <= 253:
        raise ValueError("depth >= 1 and 1 <= bits <= 253 are needed")
    b = Builder()
    old_root, new_root = b.public(), b.public()
    writes = []
    for _ in range(2):
        w = {"old_leaf": b.private()}
        w["siblings"], w["bits"] = [b.private() for _ in range(depth)], [b.private() for _ in range(depth)]
        writes.append(w)
    amount = b.private()
    amt = b.lin(1, amount, 0, None, 0)
    writes[0]["new_leaf"] = b.lin(1, writes[0]["old_leaf"], -1, amt, 0)
    writes[1]["new_leaf"] = b.lin(1, writes[1]["old_leaf"], 1, amt, 0)
    b.assert_nonzero(amt)
    for v in (amt, writes[0]["new_leaf"], writes[1]["new_leaf"]):
        b.assert_range(v, bits)
    prev = None
    for i, w in enumerate(writes):
        old, new = w["old_leaf"], w["new_leaf"]
        for sib, bit in zip(w["siblings"], w["bits"]):
            b.assert_bool(bit)
            old = _merkle_level(b, old, sib, bit, p)
            new = _merkle_level(b, new, sib, bit, p)
        b.assert_equal(old, old_root if i == 0 else prev)
        w["old_out"], w["new_out"] = old, new
        prev = new
    b.assert_equal(prev, new_root)
    circuit, layout = b.build()
    return circuit, layout, {"old_root": old_root, "new_root": new_root, "amount": amount, "writes": writes}


def merkle_transfer_inputs(layout, vars: dict, amount: int, sender, receiver) -> np.ndarray:
    """the `free` array of plonk.witness for one transfer: the amount, and sender / receiver = (old balance, siblings, bits), integers; the
    receiver's siblings are those of the tree after the sender's leaf was written"""
    values = {vars["amount"]: amount}
    for w, (old_leaf, siblings, bits) in zip(vars["writes"], (sender, receiver)):
        if len(siblings) != len(w["siblings"]) or len(bits) != len(w["bits"]):
            raise ValueError("the path does not have the circuit's depth")
        values[w["old_leaf"]] = old_leaf
        values.update(zip(w["siblings"], siblings))
        values.update(zip(w["bits"], bits))
    return layout.free(values)


def merkle_witness_inputs(layout, vars: dict, leaf: int, siblings, bits) -> np.ndarray:
    """the `free` array ([3N, 4] Montgomery Fr) of plonk.witness for one path: integers, bits as 0 / 1 (any integer is stored as given)"""
    if len(siblings) != len(vars["siblings"]) or len(bits) != len(vars["bits"]):
        raise ValueError("the path does not have the circuit's depth")
    values = {vars["leaf"]: leaf}
    values.update(zip(vars["siblings"], siblings))
    values.update(zip(vars["bits"], bits))
    return layout.free(values)
