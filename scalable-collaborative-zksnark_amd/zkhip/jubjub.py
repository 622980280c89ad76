"""
Jubjub over BLS12-381 Fr and the Schnorr signature "zkhip-schnorr-v1": on the device (zk_jubjub_mul / _check, zk_schnorr_verify,
csrc/zk_jubjub.hip), on the host in python integers (the *_host functions: the rule itself, and signing, which is host code only), and as
gadgets on circuit.Builder with the circuit "I know a signature under this public key on this public message".

THE CURVE (the same in include/zkhip.h).  -x^2 + y^2 = 1 + d x^2 y^2 over Fr, D = -10240 / 10241, a non-square, so
    (x1, y1) + (x2, y2) = ((x1 y2 + y1 x2) / (1 + d x1 x2 y1 y2), (y1 y2 + x1 x2) / (1 - d x1 x2 y1 y2))
is complete on the curve; identity (0, 1), -(x, y) = (-x, y), cofactor 8, prime subgroup order L (252 bits).  G is derived by rule (the
smallest y >= 2 with (y^2 - 1) / (1 + d y^2) a square -- y = 3 --, the smaller root x, times 8); generator_by_rule() re-derives it.

THE SCHEME.  sk in [1, L), PK = [sk] G.  sign_host(sk, m): k = SHA-256(TAG || sk || m) mod L over 32-byte little-endian canonical
encodings (k = 0 is refused), R = [k] G, e = hash2(hash2(hash2(R.x, R.y), hash2(PK.x, PK.y)), m), s = k + e sk mod L: deterministic.  e enters
every scalar multiplication as its canonical integer below r, not reduced by hand.  verify_host -> the FIRST status that applies:
    1  s >= L       2  PK or R not on the curve       3  PK outside the subgroup, or the identity       4  [s] G != R + [e] PK       0  valid
No cofactor multiplication: an R with a torsion part fails the equality by itself.

THE CIRCUITS.  schnorr_circuit(): public PK and m, private R and s (15 090 rows, mu = 14).  merkle_signed_transfer_circuit(depth, bits):
poseidon.merkle_transfer_circuit with leaves hash2(hash2(PK.x, PK.y), balance) and the sender's signature on m = hash2(hash2(receiver key hash,
amount), old_root) -- see its text for the rows and for what it does NOT protect against (replay is bound to old_root only).

THE GADGETS are plain functions on a circuit.Builder (rows appended in brackets).  A point is a pair of variables.
    assert_on_curve(b, P)          [5]    x^2, y^2, x^2 y^2, y^2 - x^2 - 1, and the assertion that this equals d x^2 y^2
    ed_add(b, P, Q) -> point       [14]   four products, two numerators, the two denominators 1 +- d x1 x2 y1 y2 (one mul row each), b.inverse of
                                          both (2 rows each: a vanishing denominator has NO witness), two products
    ed_double(b, P) -> point       [13]   ed_add(P, P) with the product x y shared
    ed_select(b, bit, P, Q)        [6]    P when bit = 1, Q when bit = 0 (b.select per coordinate; the bit is not asserted boolean here)
    ed_mul_fixed(b, bits, base=G)  [16 n - 14]  sum of bits[i] [2^i] base, bits[0] the LEAST significant: the constant [2^i] base is folded into two
                                          lin rows (bit x_i, 1 + bit (y_i - 1)): a conditional constant point costs 2 rows; n - 1 ed_add
    ed_mul(b, bits, P)             [30 n - 27]  double-and-add, LEAST significant bit first: per bit the term (bit x, 1 + bit (y - 1)) of the running
                                          double [3], ed_add into the sum [14, not for bit 0], ed_double of the running double [13, not after the last bit]
    schnorr_gadget(b, pk, m, R, s_bits, p=None)   asserts R and pk on the curve, e by four permutation_gadget hashes, e_bits =
                                          b.to_bits_strict(e) (the bits of e's canonical integer and no other), and
                                          ed_mul_fixed(s_bits) = ed_add(R, ed_mul(e_bits, pk)) coordinate by coordinate with assert_equal.
There is NO subgroup check of pk in the circuit: a public pk is checked by the verifier natively (in_subgroup_host, Jubjub.check); a
committed pk is its owner's business.
"""
from __future__ import annotations

import ctypes
import hashlib

import numpy as np

from ._lib import ZK_ERR_INVALID
from .api import _ptr
from .field import R_MOD
from .poseidon import hash2_host, permutation_gadget

TAG = b"zkhip-schnorr-v1"
D = 0x2A9318E74BFA2B48F5FD9207E6BD7FD4292D7F6D37579D2601065FD6D6343EB1
L = 0x0E7DB4EA6533AFA906673B0101343B00A6682093CCC81082D0970E5ED6F72CB7
G = (0x3A6C6DA047782F422FAD2D689CB64925D3E0878DF5BAAC0E33300795B6AE05E6, 0x4AE1F1107694F36ABA6D493320C0C7913492976D964D11ADAA206BA5C9701810)
IDENTITY = (0, 1)


# ---- the rule on the host ----
def on_curve_host(P) -> bool:
    x, y = int(P[0]), int(P[1])
    if not (0 <= x < R_MOD and 0 <= y < R_MOD):
        return False
    x2, y2 = x * x % R_MOD, y * y % R_MOD
    return (y2 - x2 - 1 - D * x2 % R_MOD * y2) % R_MOD == 0


def add_host(P, Q) -> tuple:
    x1, y1, x2, y2 = int(P[0]), int(P[1]), int(Q[0]), int(Q[1])
    k = D * x1 % R_MOD * x2 % R_MOD * y1 % R_MOD * y2 % R_MOD
    return ((x1 * y2 + y1 * x2) * pow(1 + k, -1, R_MOD) % R_MOD, (y1 * y2 + x1 * x2) * pow(1 - k, -1, R_MOD) % R_MOD)


def neg_host(P) -> tuple:
    return ((-int(P[0])) % R_MOD, int(P[1]))


def mul_host(k: int, P) -> tuple:
    """[k] P for an integer k >= 0 (any size: the group reduces it)"""
    k = int(k)
    if k < 0:
        raise ValueError("a scalar is a non-negative integer")
    acc, P = IDENTITY, (int(P[0]), int(P[1]))
    for i in reversed(range(k.bit_length())):
        acc = add_host(acc, acc)
        if (k >> i) & 1:
            acc = add_host(acc, P)
    return acc


def in_subgroup_host(P) -> bool:
    return on_curve_host(P) and mul_host(L, P) == IDENTITY


def generator_by_rule() -> tuple:
    """(y, G): the rule of the module text, from nothing but D"""
    y = 2
    while True:
        x2 = (y * y - 1) * pow(1 + D * y * y, -1, R_MOD) % R_MOD
        if pow(x2, (R_MOD - 1) // 2, R_MOD) == 1:
            break
        y += 1
    # Tonelli-Shanks: r - 1 = 2^32 t
    s, t = 32, (R_MOD - 1) >> 32
    z = 2
    while pow(z, (R_MOD - 1) // 2, R_MOD) == 1:
        z += 1
    m, c, u, x = s, pow(z, t, R_MOD), pow(x2, t, R_MOD), pow(x2, (t + 1) // 2, R_MOD)
    while u != 1:
        i, w = 0, u
        while w != 1:
            w, i = w * w % R_MOD, i + 1
        bb = pow(c, 1 << (m - i - 1), R_MOD)
        m, c, u, x = i, bb * bb % R_MOD, u * bb * bb % R_MOD, x * bb % R_MOD
    return y, mul_host(8, (min(x, R_MOD - x), y))


def _le32(x: int) -> bytes:
    return int(x).to_bytes(32, "little")


def keygen_host(sk: int) -> tuple:
    if not 1 <= int(sk) < L:
        raise ValueError("a secret key lies in [1, L)")
    return mul_host(sk, G)


def challenge_host(R, pk, m: int, p: dict | None = None) -> int:
    return hash2_host(hash2_host(hash2_host(R[0], R[1], p), hash2_host(pk[0], pk[1], p), p), int(m) % R_MOD, p)


def sign_host(sk: int, m: int, p: dict | None = None) -> tuple:
    """-> (R, s), deterministic (module text)"""
    pk = keygen_host(sk)
    m = int(m) % R_MOD
    k = int.from_bytes(hashlib.sha256(TAG + _le32(sk) + _le32(m)).digest(), "little") % L
    if k == 0:
        raise ValueError("the nonce of this key and message is 0")
    R = mul_host(k, G)
    return R, (k + challenge_host(R, pk, m, p) * int(sk)) % L


def verify_host(pk, m: int, sig, p: dict | None = None) -> int:
    R, s = sig
    if not 0 <= int(s) < L:
        return 1
    if not (on_curve_host(pk) and on_curve_host(R)):
        return 2
    pk, R = (int(pk[0]), int(pk[1])), (int(R[0]), int(R[1]))
    if pk == IDENTITY or mul_host(L, pk) != IDENTITY:
        return 3
    return 0 if mul_host(s, G) == add_host(R, mul_host(challenge_host(R, pk, m, p), pk)) else 4


def signature_bytes(sig) -> bytes:
    """R.x || R.y || s, 32-byte little-endian canonical encodings (the tools print their SHA-256)"""
    return _le32(sig[0][0]) + _le32(sig[0][1]) + _le32(sig[1])


# ---- the device ----
def _mont_rows(xs) -> np.ndarray:
    return np.frombuffer(b"".join(((int(x) << 256) % R_MOD).to_bytes(32, "little") for x in xs), dtype="<u8").astype(np.uint64).reshape(-1, 4)


def _plain_rows(xs) -> np.ndarray:
    return np.frombuffer(b"".join(int(x).to_bytes(32, "little") for x in xs), dtype="<u8").astype(np.uint64).reshape(-1, 4)


def points_limbs(points) -> np.ndarray:
    """[(x, y)] integers below r -> [n, 2, 4] u64 Montgomery limbs"""
    return _mont_rows([c for P in points for c in P]).reshape(-1, 2, 4)


def points_ints(a) -> list:
    rinv = pow(1 << 256, -1, R_MOD)
    v = [int.from_bytes(np.ascontiguousarray(row, dtype="<u8").tobytes(), "little") * rinv % R_MOD for row in np.asarray(a).reshape(-1, 4)]
    return list(zip(v[0::2], v[1::2]))


def scalars_limbs(ks) -> np.ndarray:
    """integers below 2^256 -> [n, 4] u64 plain limbs"""
    return _plain_rows(ks)


def signatures_limbs(sigs) -> np.ndarray:
    """[((R.x, R.y), s)] -> [n, 3, 4] u64: R in Montgomery form, s a plain integer"""
    out = np.zeros((len(sigs), 3, 4), dtype=np.uint64)
    if len(sigs):
        out[:, :2] = points_limbs([R for R, _ in sigs])
        out[:, 2] = _plain_rows([s for _, s in sigs])
    return out


class Jubjub:
    """the device calls on one Ctx (`poseidon`: a poseidon.Poseidon of the same Ctx, whose constants the challenge uses).  Arguments that name
    device memory are what Ctx takes (DeviceBuffer, view, address).  A refusal of the library (ZK_ERR_INVALID): ValueError with its message."""

    def __init__(self, be, poseidon):
        self.be, self.poseidon = be, poseidon

    def _check(self, rc: int):
        if rc == ZK_ERR_INVALID:
            raise ValueError((self.be.lib.zk_last_error(self.be.h) or b"").decode())
        self.be._check(rc)

    def mul(self, points, scalars, n: int, out=None):
        """out[i] = [scalars[i]] points[i] ([n][2] Fr; points = None: the base G).  With points the call waits for their on-curve check and
        raises "K of N points are not on the curve; the first is I" before anything is written; the multiplication itself is enqueued"""
        if out is None:
            out = self.be.alloc(max(64 * n, 1))
        self._check(self.be.lib.zk_jubjub_mul(self.be.h, _ptr(points), _ptr(scalars), _ptr(out), n))
        return out

    def check(self, points, n: int) -> np.ndarray:
        """[n] u32: 0 in the prime-order subgroup, 2 not on the curve, 3 on the curve but outside the subgroup.  Blocking (the statuses are read)"""
        st = self.be.alloc(max(4 * n, 1))
        self._check(self.be.lib.zk_jubjub_check(self.be.h, _ptr(points), _ptr(st), n))
        return st.download((n,), np.uint32)

    def schnorr_verify(self, pk, msg, sig, n: int) -> np.ndarray:
        """[n] u32 statuses (module text) of n signatures: pk [n][2] Fr, msg [n] Fr, sig [n][3] words (signatures_limbs).  Blocking"""
        st = self.be.alloc(max(4 * n, 1))
        self._check(self.be.lib.zk_schnorr_verify(self.be.h, self.poseidon.h, _ptr(pk), _ptr(msg), _ptr(sig), _ptr(st), n))
        return st.download((n,), np.uint32)


# ---- the gadgets ----
def assert_on_curve(b, P) -> None:
    x2, y2 = b.mul(P[0], P[0]), b.mul(P[1], P[1])
    b.assert_zero_of(1, b.lin(1, y2, -1, x2, -1), -D, b.mul(x2, y2), 0, 0)


def _ed_finish(b, nx, ny, u, v) -> tuple:
    """(nx / (1 + d u v), ny / (1 - d u v)): 8 rows"""
    ix, iy = b.inverse(b.mul(u, v, D, 1)), b.inverse(b.mul(u, v, -D, 1))
    return b.mul(nx, ix), b.mul(ny, iy)


def ed_add(b, P, Q) -> tuple:
    u, v = b.mul(P[0], Q[1]), b.mul(P[1], Q[0])
    yy, xx = b.mul(P[1], Q[1]), b.mul(P[0], Q[0])
    return _ed_finish(b, b.lin(1, u, 1, v, 0), b.lin(1, yy, 1, xx, 0), u, v)


def ed_double(b, P) -> tuple:
    u = b.mul(P[0], P[1])
    yy, xx = b.mul(P[1], P[1]), b.mul(P[0], P[0])
    return _ed_finish(b, b.lin(2, u, 0, None, 0), b.lin(1, yy, 1, xx, 0), u, u)


def ed_select(b, bit, P, Q) -> tuple:
    return b.select(bit, P[0], Q[0]), b.select(bit, P[1], Q[1])


def ed_mul_fixed(b, bits, base=G) -> tuple:
    acc, cur = None, (int(base[0]), int(base[1]))
    for bit in bits:
        term = (b.lin(cur[0], bit, 0, None, 0), b.lin(cur[1] - 1, bit, 0, None, 1))
        acc = term if acc is None else ed_add(b, acc, term)
        cur = add_host(cur, cur)
    return acc


def ed_mul(b, bits, P) -> tuple:
    acc, cur = None, P
    for i, bit in enumerate(bits):
        term = (b.mul(bit, cur[0]), b.mul(bit, b.lin(1, cur[1], 0, None, -1), 1, 1))
        acc = term if acc is None else ed_add(b, acc, term)
        if i + 1 < len(bits):
            cur = ed_double(b, cur)
    return acc


S_BITS = 252


def _hash2_gadget(b, left, right, p):
    return permutation_gadget(b, (b.lin(0, None, 0, None, 0), left, right), p)[0]


def schnorr_gadget(b, pk, m, R, s_bits, p: dict | None = None) -> dict:
    """the rows of one verification (module text) -> {"e", "e_bits", "lhs", "rhs"}.  s_bits: 252 variables the CALLER asserts boolean, least
    significant first.  Rows: 2 x 5 on-curve, 251 for s <= L - 1 (Builder.assert_bits_at_most: s + L has no witness), 4 x 475 hashes,
    to_bits_strict, ed_mul_fixed, ed_mul over 255 bits, one ed_add: 14 834 in all"""
    if len(s_bits) != S_BITS:
        raise ValueError(f"{S_BITS} bits of s are needed")
    b.assert_bits_at_most(s_bits, L - 1)
    assert_on_curve(b, R)
    assert_on_curve(b, pk)
    e = _hash2_gadget(b, _hash2_gadget(b, _hash2_gadget(b, R[0], R[1], p), _hash2_gadget(b, pk[0], pk[1], p), p), m, p)
    e_bits = b.to_bits_strict(e)
    lhs = ed_mul_fixed(b, s_bits)
    rhs = ed_add(b, R, ed_mul(b, e_bits, pk))
    b.assert_equal(lhs[0], rhs[0])
    b.assert_equal(lhs[1], rhs[1])
    return {"e": e, "e_bits": e_bits, "lhs": lhs, "rhs": rhs}


SCHNORR_ROWS = (15090, 14, 4)  # rows (the 4 input rows included), mu, l of schnorr_circuit() with the v1 Poseidon instance: counted by building it


def schnorr_circuit(p: dict | None = None):
    """-> (circuit, layout, vars) of "I know a signature (R, s) under the public key (public inputs PK.x, PK.y) on the public message m
    (the third public input)".  Private: R.x, R.y and the 252 bits of s, each asserted boolean.  The private values pass through one lin
    copy each where a gadget wants a computed value.  vars = {"pk": (x, y), "m", "R": (x, y), "s_bits": [252], ...schnorr_gadget's}.
    The bits of s are compared with L - 1 (schnorr_gadget), so s is the canonical scalar as in the native rule: s + L has no witness.
    15 090 rows, mu = 14 (SCHNORR_ROWS): 4 input rows, 252 bit assertions, 14 834 of the gadget"""
    from .circuit import Builder

    b = Builder()
    pk, m = (b.public(), b.public()), b.public()
    R = (b.private(), b.private())
    s_bits = [b.private() for _ in range(S_BITS)]
    for v in s_bits:
        b.assert_bool(v)
    out = schnorr_gadget(b, pk, m, R, s_bits, p)
    circuit, layout = b.build()
    out.update({"pk": pk, "m": m, "R": R, "s_bits": s_bits})
    return circuit, layout, out


def schnorr_inputs(layout, vars: dict, sig) -> np.ndarray:
    """the `free` array of plonk.witness for one signature ((R.x, R.y), s), integers; the public inputs are (PK.x, PK.y, m, 0)"""
    (rx, ry), s = sig
    if not 0 <= int(s) < 1 << S_BITS:
        raise ValueError(f"s does not fit the circuit's {S_BITS} bits")
    values = {vars["R"][0]: rx, vars["R"][1]: ry}
    values.update({v: (int(s) >> i) & 1 for i, v in enumerate(vars["s_bits"])})
    return layout.free(values)


def merkle_signed_transfer_circuit(depth: int, bits: int = 64, p: dict | None = None):
    """-> (circuit, layout, vars) of "the tree with public root R became the tree with public root R' by moving a private non-zero amount
    from one leaf to another, amount and new balances below 2^bits, AND the owner of the sending leaf signed it".  It is
    poseidon.merkle_transfer_circuit with
        leaf = hash2(key hash, balance),   key hash = hash2(PK.x, PK.y)
    for both leaves, old and new: a write changes the balance and keeps the key hash.  The sender's key hash is COMPUTED from the private
    PK; the receiver's is a private value (its preimage is not needed).  schnorr_gadget under the sender's PK checks a private signature on
        m = hash2(hash2(receiver key hash, amount), old_root).
    REPLAY: m is bound to old_root, and that is the only protection -- the same signature is valid again whenever the tree returns to that
    root.  A per-leaf nonce is out of scope.  There is no subgroup check of the committed PK (module text): it is its owner's business.
    Rows: amt, the two new balances, assert_nonzero, three range checks (3 + 2 + 3 (3 bits - 1), as merkle_transfer_circuit); 475 for the
    sender's key hash, 4 x 475 for the leaves, 2 x 475 for m; 252 bit assertions and the 14 834 rows of schnorr_gadget; 959 per level and write.
    (depth, bits) = (2, 8): 22 323 rows with the 2 input rows, mu = 15.
    vars = {"old_root", "new_root", "amount", "pk": (x, y), "receiver_key", "R", "s_bits", "m", "writes": [2 x {"balance", "new_balance",
    "old_leaf", "new_leaf", "siblings", "bits", "old_out", "new_out"}]} (write 0: the sender; write 1: the receiver, whose path is one of the
    tree AFTER write 0)"""
    from .circuit import Builder
    from .poseidon import _merkle_level

    if depth < 1 or not 1 <= bits <= 253:
        raise ValueError("depth >= 1 and 1 <= bits <= 253 are needed")
    b = Builder()
    old_root, new_root = b.public(), b.public()
    pk, receiver_key = (b.private(), b.private()), b.private()
    writes = []
    for _ in range(2):
        w = {"balance": b.private()}
        w["siblings"], w["bits"] = [b.private() for _ in range(depth)], [b.private() for _ in range(depth)]
        writes.append(w)
    amount = b.private()
    R = (b.private(), b.private())
    s_bits = [b.private() for _ in range(S_BITS)]
    amt = b.lin(1, amount, 0, None, 0)
    writes[0]["new_balance"] = b.lin(1, writes[0]["balance"], -1, amt, 0)
    writes[1]["new_balance"] = b.lin(1, writes[1]["balance"], 1, amt, 0)
    b.assert_nonzero(amt)
    for v in (amt, writes[0]["new_balance"], writes[1]["new_balance"]):
        b.assert_range(v, bits)
    keys = (_hash2_gadget(b, pk[0], pk[1], p), receiver_key)
    for w, key in zip(writes, keys):
        w["old_leaf"], w["new_leaf"] = _hash2_gadget(b, key, w["balance"], p), _hash2_gadget(b, key, w["new_balance"], p)
    m = _hash2_gadget(b, _hash2_gadget(b, receiver_key, amt, p), old_root, p)
    for v in s_bits:
        b.assert_bool(v)
    out = schnorr_gadget(b, pk, m, R, s_bits, p)
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
    out.update({"old_root": old_root, "new_root": new_root, "amount": amount, "pk": pk, "receiver_key": receiver_key, "R": R, "s_bits": s_bits,
                "m": m, "writes": writes})
    return circuit, layout, out


def signed_transfer_message(receiver_key: int, amount: int, old_root: int, p: dict | None = None) -> int:
    """the message the sender signs: hash2(hash2(receiver key hash, amount), old_root)"""
    return hash2_host(hash2_host(receiver_key, amount, p), old_root, p)


def merkle_signed_transfer_inputs(layout, vars: dict, amount: int, pk, receiver_key: int, sig, sender, receiver) -> np.ndarray:
    """the `free` array of plonk.witness for one signed transfer: the amount, the sender's PK, the receiver's key hash, the signature
    ((R.x, R.y), s) on signed_transfer_message(...), and sender / receiver = (old balance, siblings, bits), integers; the receiver's
    siblings are those of the tree after the sender's leaf was written.  The public inputs are (old root, new root)"""
    (rx, ry), s = sig
    if not 0 <= int(s) < 1 << S_BITS:
        raise ValueError(f"s does not fit the circuit's {S_BITS} bits")
    values = {vars["amount"]: amount, vars["pk"][0]: pk[0], vars["pk"][1]: pk[1], vars["receiver_key"]: receiver_key, vars["R"][0]: rx, vars["R"][1]: ry}
    values.update({v: (int(s) >> i) & 1 for i, v in enumerate(vars["s_bits"])})
    for w, (balance, siblings, bits) in zip(vars["writes"], (sender, receiver)):
        if len(siblings) != len(w["siblings"]) or len(bits) != len(w["bits"]):
            raise ValueError("the path does not have the circuit's depth")
        values[w["balance"]] = balance
        values.update(zip(w["siblings"], siblings))
        values.update(zip(w["bits"], bits))
    return layout.free(values)
