// Jubjub over BLS12-381 Fr and the Schnorr signature "zkhip-schnorr-v1" -- the compiled mirror of zkhip/jubjub.py, which carries the full
// text: the constants, the host rules on zkhost's Fr (signing included, which is host code only), and the gadgets and the two circuits on
// CircuitBuilder, ROW FOR ROW as the Python builder emits them, so both hosts print one circuit digest.  The device calls are
// Ctx::jubjub_mul / jubjub_check / schnorr_verify (device.hpp).
//
// THE CURVE: -x^2 + y^2 = 1 + d x^2 y^2, d = -10240 / 10241 (a non-square: the addition law is complete), identity (0, 1), cofactor 8,
// prime subgroup order l.  THE SCHEME: PK = [sk] G; k = SHA-256(tag || sk || m) mod l over 32-byte little-endian canonical encodings,
// R = [k] G, e = hash2(hash2(hash2(R.x, R.y), hash2(PK.x, PK.y)), m), s = k + e sk mod l; e enters every multiplication as its canonical
// integer below r.  jubjub_verify_host -> the FIRST status that applies: 1 s >= l; 2 PK or R not on the curve; 3 PK outside the
// subgroup or the identity; 4 [s] G != R + [e] PK; 0 valid.
// Scalars are 4 little-endian uint64_t (a plain integer).  The host multiplies in extended coordinates with the unified a = -1 addition
// (the formulas of csrc/zk_jubjub.hip) and inverts once: the affine result is the same field elements as the affine law gives.
#pragma once
#include <array>

#include "poseidon.hpp"

namespace zkhost {

using JjScalar = std::array<uint64_t, 4>;
struct JjPoint {
    Fr x, y;
    bool operator==(const JjPoint &o) const { return x == o.x && y == o.y; }
};
struct JjSignature {
    JjPoint R;
    JjScalar s;
};

namespace jubjub {
static constexpr JjScalar kL = {0xd0970e5ed6f72cb7ull, 0xa6682093ccc81082ull, 0x06673b0101343b00ull, 0x0e7db4ea6533afa9ull};
static constexpr JjScalar kLm1 = {0xd0970e5ed6f72cb6ull, 0xa6682093ccc81082ull, 0x06673b0101343b00ull, 0x0e7db4ea6533afa9ull};
static constexpr JjScalar kRm1 = {0xffffffff00000000ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull, 0x73eda753299d7d48ull};
static constexpr size_t kSBits = 252;
inline Fr fr_of(const JjScalar &c) {  // a canonical integer below r
    Fr t;
    for (size_t i = 0; i < 4; ++i) t.v[i] = c[i];
    return Fr::from_canonical(t);
}
inline JjScalar canonical(const Fr &x) {
    const Fr c = x.to_canonical();
    return {c.v[0], c.v[1], c.v[2], c.v[3]};
}
inline const Fr &d() {
    static const Fr k = -(Fr::from_u64(10240) * Fr::from_u64(10241).inverse());
    return k;
}
inline const JjPoint &g() {
    static const JjPoint k{fr_of({0x33300795b6ae05e6ull, 0xd3e0878df5baac0eull, 0x2fad2d689cb64925ull, 0x3a6c6da047782f42ull}),
                           fr_of({0xaa206ba5c9701810ull, 0x3492976d964d11adull, 0xba6d493320c0c791ull, 0x4ae1f1107694f36aull})};
    return k;
}
inline JjPoint identity() { return {Fr::zero(), Fr::one()}; }
inline bool bit(const JjScalar &k, size_t i) { return (k[i / 64] >> (i % 64)) & 1; }
inline bool less(const JjScalar &a, const JjScalar &b) {
    for (size_t i = 4; i-- > 0;)
        if (a[i] != b[i]) return a[i] < b[i];
    return false;
}
// (the little-endian integer of `n` limbs) mod l, bit by bit: the running value stays below l < 2^252
inline JjScalar mod_l(const uint64_t *w, size_t n) {
    JjScalar acc = {0, 0, 0, 0};
    for (size_t i = 64 * n; i-- > 0;) {
        for (size_t j = 4; j-- > 1;) acc[j] = (acc[j] << 1) | (acc[j - 1] >> 63);
        acc[0] = (acc[0] << 1) | ((w[i / 64] >> (i % 64)) & 1);
        if (!less(acc, kL)) {
            unsigned __int128 borrow = 0;
            for (size_t j = 0; j < 4; ++j) {
                const unsigned __int128 t = (unsigned __int128)acc[j] - kL[j] - borrow;
                acc[j] = (uint64_t)t;
                borrow = (t >> 64) & 1;
            }
        }
    }
    return acc;
}
// (a b + c) mod l
inline JjScalar mul_add_mod_l(const JjScalar &a, const JjScalar &b, const JjScalar &c) {
    uint64_t w[9] = {0};
    for (size_t i = 0; i < 4; ++i) {
        unsigned __int128 carry = 0;
        for (size_t j = 0; j < 4; ++j) {
            const unsigned __int128 t = (unsigned __int128)a[i] * b[j] + w[i + j] + carry;
            w[i + j] = (uint64_t)t;
            carry = t >> 64;
        }
        w[i + 4] = (uint64_t)carry;
    }
    unsigned __int128 carry = 0;
    for (size_t i = 0; i < 9; ++i) {
        const unsigned __int128 t = (unsigned __int128)w[i] + (i < 4 ? c[i] : 0) + carry;
        w[i] = (uint64_t)t;
        carry = t >> 64;
    }
    return mod_l(w, 9);
}
struct Ext {
    Fr x, y, z, t;
};
inline Ext ext_add(const Ext &p, const Ext &q, const Fr &d2) {
    const Fr a = (p.y - p.x) * (q.y - q.x), b = (p.y + p.x) * (q.y + q.x), c = p.t * q.t * d2, zz = p.z * q.z, dd = zz + zz;
    const Fr e = b - a, f = dd - c, g = dd + c, h = b + a;
    return {e * f, g * h, f * g, e * h};
}
inline void le32(const JjScalar &k, uint8_t out[32]) {
    for (size_t i = 0; i < 32; ++i) out[i] = uint8_t(k[i / 8] >> (8 * (i % 8)));
}
}  // namespace jubjub

// ---- the rule on the host ----
inline bool jubjub_on_curve_host(const JjPoint &P) {
    const Fr x2 = P.x * P.x, y2 = P.y * P.y;
    return y2 - x2 - Fr::one() == jubjub::d() * x2 * y2;
}
inline JjPoint jubjub_add_host(const JjPoint &P, const JjPoint &Q) {
    const Fr k = jubjub::d() * P.x * Q.x * P.y * Q.y;
    return {(P.x * Q.y + P.y * Q.x) * (Fr::one() + k).inverse(), (P.y * Q.y + P.x * Q.x) * (Fr::one() - k).inverse()};
}
inline JjPoint jubjub_neg_host(const JjPoint &P) { return {-P.x, P.y}; }
inline JjPoint jubjub_mul_host(const JjScalar &k, const JjPoint &P) {
    const Fr d2 = jubjub::d() + jubjub::d();
    const jubjub::Ext base{P.x, P.y, Fr::one(), P.x * P.y};
    jubjub::Ext acc{Fr::zero(), Fr::one(), Fr::one(), Fr::zero()};
    for (size_t i = 256; i-- > 0;) {
        acc = jubjub::ext_add(acc, acc, d2);
        if (jubjub::bit(k, i)) acc = jubjub::ext_add(acc, base, d2);
    }
    const Fr zi = acc.z.inverse();
    return {acc.x * zi, acc.y * zi};
}
inline bool jubjub_in_subgroup_host(const JjPoint &P) { return jubjub_on_curve_host(P) && jubjub_mul_host(jubjub::kL, P) == jubjub::identity(); }
inline JjPoint jubjub_keygen_host(const JjScalar &sk) {
    if (!jubjub::less(sk, jubjub::kL) || (sk[0] | sk[1] | sk[2] | sk[3]) == 0) throw ZkError(ZK_ERR_INVALID, "jubjub: a secret key lies in [1, L)");
    return jubjub_mul_host(sk, jubjub::g());
}
inline Fr jubjub_challenge_host(const JjPoint &R, const JjPoint &pk, const Fr &m, const PoseidonConsts &p = poseidon_v1()) {
    return poseidon_hash2_host(poseidon_hash2_host(poseidon_hash2_host(R.x, R.y, p), poseidon_hash2_host(pk.x, pk.y, p), p), m, p);
}
inline JjSignature jubjub_sign_host(const JjScalar &sk, const Fr &m, const PoseidonConsts &p = poseidon_v1()) {
    const JjPoint pk = jubjub_keygen_host(sk);
    uint8_t buf[64], dig[32];
    jubjub::le32(sk, buf);
    jubjub::le32(jubjub::canonical(m), buf + 32);
    Sha256 h;
    h.update("zkhip-schnorr-v1", 16);
    h.update(buf, 64);
    h.digest(dig);
    uint64_t w[4] = {0, 0, 0, 0};
    for (size_t i = 0; i < 32; ++i) w[i / 8] |= uint64_t(dig[i]) << (8 * (i % 8));
    const JjScalar k = jubjub::mod_l(w, 4);
    if ((k[0] | k[1] | k[2] | k[3]) == 0) throw ZkError(ZK_ERR_INVALID, "jubjub: the nonce of this key and message is 0");
    JjSignature sig;
    sig.R = jubjub_mul_host(k, jubjub::g());
    sig.s = jubjub::mul_add_mod_l(jubjub::canonical(jubjub_challenge_host(sig.R, pk, m, p)), sk, k);
    return sig;
}
inline int jubjub_verify_host(const JjPoint &pk, const Fr &m, const JjSignature &sig, const PoseidonConsts &p = poseidon_v1()) {
    if (!jubjub::less(sig.s, jubjub::kL)) return 1;
    if (!(jubjub_on_curve_host(pk) && jubjub_on_curve_host(sig.R))) return 2;
    if (pk == jubjub::identity() || !(jubjub_mul_host(jubjub::kL, pk) == jubjub::identity())) return 3;
    const JjPoint rhs = jubjub_add_host(sig.R, jubjub_mul_host(jubjub::canonical(jubjub_challenge_host(sig.R, pk, m, p)), pk));
    return jubjub_mul_host(sig.s, jubjub::g()) == rhs ? 0 : 4;
}
// SHA-256 of R.x || R.y || s, 32-byte little-endian canonical encodings
inline std::string jubjub_signature_digest(const JjSignature &sig) {
    uint8_t buf[96];
    jubjub::le32(jubjub::canonical(sig.R.x), buf);
    jubjub::le32(jubjub::canonical(sig.R.y), buf + 32);
    jubjub::le32(sig.s, buf + 64);
    Sha256 h;
    h.update(buf, 96);
    return h.hex();
}

// ---- the gadgets (zkhip/jubjub.py and zkhip/circuit.py have the text and the row counts) ----
using VarPoint = std::array<Var, 2>;
// the integer of n boolean variables, least significant first, is <= c; c has exactly n bits  [n - 1 rows]
inline void assert_bits_at_most(CircuitBuilder &b, const std::vector<Var> &bits, const JjScalar &c) {
    const size_t n = bits.size();
    if (n < 2 || n > 256 || !jubjub::bit(c, n - 1)) throw ZkError(ZK_ERR_INVALID, "assert_bits_at_most takes n >= 2 bits and a constant of exactly n bits");
    Var e = bits[n - 1];
    for (size_t k = n - 1; k-- > 0;) {
        if (jubjub::bit(c, k)) e = b.mul(e, bits[k]);
        else b.assert_zero_of(Fr::zero(), e, Fr::zero(), bits[k], Fr::one(), Fr::zero());
    }
}
// the 255 bits of x's canonical integer and of no other  [1018 rows]
inline std::vector<Var> to_bits_strict(CircuitBuilder &b, Var x) {
    std::vector<Var> bits;
    for (size_t k = 0; k < 255; ++k) bits.push_back(b.bits_of(x, k, 1));
    for (Var v : bits) b.assert_bool(v);
    Var acc = bits[0];
    Fr pw = Fr::one();
    for (size_t k = 1; k < 255; ++k) {
        pw += pw;
        acc = b.lin(Fr::one(), acc, pw, bits[k]);
    }
    b.assert_equal(acc, x);
    assert_bits_at_most(b, bits, jubjub::kRm1);
    return bits;
}
inline void jubjub_assert_on_curve(CircuitBuilder &b, const VarPoint &P) {
    const Var x2 = b.mul(P[0], P[0]), y2 = b.mul(P[1], P[1]);
    const Var t = b.lin(Fr::one(), y2, -Fr::one(), x2, -Fr::one());
    const Var q = b.mul(x2, y2);
    b.assert_zero_of(Fr::one(), t, -jubjub::d(), q, Fr::zero(), Fr::zero());
}
namespace jubjub {
inline VarPoint ed_finish(CircuitBuilder &b, Var nx, Var ny, Var u, Var v) {
    const Var ix = b.inverse(b.mul(u, v, d(), Fr::one()));
    const Var iy = b.inverse(b.mul(u, v, -d(), Fr::one()));
    const Var x = b.mul(nx, ix);
    const Var y = b.mul(ny, iy);
    return {x, y};
}
inline Var hash2_gadget(CircuitBuilder &b, Var left, Var right, const PoseidonConsts &p) {
    const Var z = b.lin(Fr::zero(), kNoVar, Fr::zero(), kNoVar, Fr::zero());
    return poseidon_permutation_gadget(b, {z, left, right}, p)[0];
}
}  // namespace jubjub
inline VarPoint jubjub_ed_add(CircuitBuilder &b, const VarPoint &P, const VarPoint &Q) {
    const Var u = b.mul(P[0], Q[1]), v = b.mul(P[1], Q[0]);
    const Var yy = b.mul(P[1], Q[1]), xx = b.mul(P[0], Q[0]);
    const Var nx = b.lin(Fr::one(), u, Fr::one(), v);
    const Var ny = b.lin(Fr::one(), yy, Fr::one(), xx);
    return jubjub::ed_finish(b, nx, ny, u, v);
}
inline VarPoint jubjub_ed_double(CircuitBuilder &b, const VarPoint &P) {
    const Var u = b.mul(P[0], P[1]);
    const Var yy = b.mul(P[1], P[1]), xx = b.mul(P[0], P[0]);
    const Var nx = b.lin(Fr::from_u64(2), u, Fr::zero(), kNoVar);
    const Var ny = b.lin(Fr::one(), yy, Fr::one(), xx);
    return jubjub::ed_finish(b, nx, ny, u, u);
}
inline VarPoint jubjub_ed_select(CircuitBuilder &b, Var bit, const VarPoint &P, const VarPoint &Q) {
    const Var x = b.select(bit, P[0], Q[0]);
    const Var y = b.select(bit, P[1], Q[1]);
    return {x, y};
}
// sum of bits[i] [2^i] base, bits[0] the least significant
inline VarPoint jubjub_ed_mul_fixed(CircuitBuilder &b, const std::vector<Var> &bits, JjPoint cur = jubjub::g()) {
    VarPoint acc{kNoVar, kNoVar};
    for (size_t i = 0; i < bits.size(); ++i) {
        const Var tx = b.lin(cur.x, bits[i], Fr::zero(), kNoVar, Fr::zero());
        const Var ty = b.lin(cur.y - Fr::one(), bits[i], Fr::zero(), kNoVar, Fr::one());
        acc = i == 0 ? VarPoint{tx, ty} : jubjub_ed_add(b, acc, {tx, ty});
        cur = jubjub_add_host(cur, cur);
    }
    return acc;
}
// double-and-add, least significant bit first
inline VarPoint jubjub_ed_mul(CircuitBuilder &b, const std::vector<Var> &bits, VarPoint cur) {
    VarPoint acc{kNoVar, kNoVar};
    for (size_t i = 0; i < bits.size(); ++i) {
        const Var tx = b.mul(bits[i], cur[0]);
        const Var ym1 = b.lin(Fr::one(), cur[1], Fr::zero(), kNoVar, -Fr::one());
        const Var ty = b.mul(bits[i], ym1, Fr::one(), Fr::one());
        acc = i == 0 ? VarPoint{tx, ty} : jubjub_ed_add(b, acc, {tx, ty});
        if (i + 1 < bits.size()) cur = jubjub_ed_double(b, cur);
    }
    return acc;
}
// the rows of one verification; s_bits: 252 variables the caller asserts boolean.  No subgroup check of pk (zkhip/jubjub.py)
inline void jubjub_schnorr_gadget(CircuitBuilder &b, const VarPoint &pk, Var m, const VarPoint &R, const std::vector<Var> &s_bits, const PoseidonConsts &p = poseidon_v1()) {
    if (s_bits.size() != jubjub::kSBits) throw ZkError(ZK_ERR_INVALID, "schnorr_gadget: 252 bits of s are needed");
    assert_bits_at_most(b, s_bits, jubjub::kLm1);
    jubjub_assert_on_curve(b, R);
    jubjub_assert_on_curve(b, pk);
    const Var hr = jubjub::hash2_gadget(b, R[0], R[1], p);
    const Var hp = jubjub::hash2_gadget(b, pk[0], pk[1], p);
    const Var h2 = jubjub::hash2_gadget(b, hr, hp, p);
    const Var e = jubjub::hash2_gadget(b, h2, m, p);
    const std::vector<Var> e_bits = to_bits_strict(b, e);
    const VarPoint lhs = jubjub_ed_mul_fixed(b, s_bits);
    const VarPoint ep = jubjub_ed_mul(b, e_bits, pk);
    const VarPoint rhs = jubjub_ed_add(b, R, ep);
    b.assert_equal(lhs[0], rhs[0]);
    b.assert_equal(lhs[1], rhs[1]);
}

struct SchnorrVars {
    VarPoint pk{kNoVar, kNoVar}, R{kNoVar, kNoVar};
    Var m = kNoVar;
    std::vector<Var> s_bits;
};
// public PK.x, PK.y, m; private R and the 252 bits of s (zkhip.jubjub.schnorr_circuit): 15 090 rows, mu = 14
inline PlonkCircuit jubjub_schnorr_circuit(CircuitLayout &layout, SchnorrVars &v, const PoseidonConsts &p = poseidon_v1()) {
    CircuitBuilder b;
    v = SchnorrVars();
    v.pk[0] = b.pub(), v.pk[1] = b.pub(), v.m = b.pub();
    v.R[0] = b.priv(), v.R[1] = b.priv();
    for (size_t i = 0; i < jubjub::kSBits; ++i) v.s_bits.push_back(b.priv());
    for (Var s : v.s_bits) b.assert_bool(s);
    jubjub_schnorr_gadget(b, v.pk, v.m, v.R, v.s_bits, p);
    return b.build(layout);
}
namespace jubjub {
inline void signature_values(std::vector<std::pair<Var, Fr>> &values, const VarPoint &R, const std::vector<Var> &s_bits, const JjSignature &sig) {
    if (sig.s[3] >> (kSBits - 192)) throw ZkError(ZK_ERR_INVALID, "s does not fit the circuit's 252 bits");
    values.push_back({R[0], sig.R.x});
    values.push_back({R[1], sig.R.y});
    for (size_t i = 0; i < s_bits.size(); ++i) values.push_back({s_bits[i], Fr::from_u64(bit(sig.s, i))});
}
}  // namespace jubjub
inline FrVec jubjub_schnorr_inputs(const CircuitLayout &layout, const SchnorrVars &v, const JjSignature &sig) {
    std::vector<std::pair<Var, Fr>> values;
    jubjub::signature_values(values, v.R, v.s_bits, sig);
    return layout.free(values);
}

// the transfer circuit on leaves hash2(hash2(PK.x, PK.y), balance) with the sender's signature on
// m = hash2(hash2(receiver key hash, amount), old_root) checked inside (zkhip.jubjub.merkle_signed_transfer_circuit, row for row).  Binding m
// to the old root is the only replay protection; there is no subgroup check of the committed PK
struct SignedTransferWrite {
    Var balance = kNoVar, new_balance = kNoVar, old_leaf = kNoVar, new_leaf = kNoVar, old_out = kNoVar, new_out = kNoVar;
    std::vector<Var> siblings, bits;
};
struct SignedTransferVars {
    Var old_root = kNoVar, new_root = kNoVar, amount = kNoVar, receiver_key = kNoVar, m = kNoVar;
    VarPoint pk{kNoVar, kNoVar}, R{kNoVar, kNoVar};
    std::vector<Var> s_bits;
    SignedTransferWrite writes[2];
};
struct SignedTransferSide {  // one side, on the tree before its write
    Fr balance;
    FrVec siblings;
    std::vector<uint64_t> bits;
};
inline Fr jubjub_signed_transfer_message(const Fr &receiver_key, const Fr &amount, const Fr &old_root, const PoseidonConsts &p = poseidon_v1()) {
    return poseidon_hash2_host(poseidon_hash2_host(receiver_key, amount, p), old_root, p);
}
inline PlonkCircuit jubjub_merkle_signed_transfer_circuit(size_t depth, size_t bits, CircuitLayout &layout, SignedTransferVars &v, const PoseidonConsts &p = poseidon_v1()) {
    if (depth < 1 || bits < 1 || bits > 253) throw ZkError(ZK_ERR_INVALID, "merkle_signed_transfer_circuit: depth >= 1 and 1 <= bits <= 253 are needed");
    CircuitBuilder b;
    v = SignedTransferVars();
    const Fr one = Fr::one(), zero = Fr::zero();
    v.old_root = b.pub(), v.new_root = b.pub();
    v.pk[0] = b.priv(), v.pk[1] = b.priv(), v.receiver_key = b.priv();
    for (SignedTransferWrite &w : v.writes) {
        w.balance = b.priv();
        for (size_t i = 0; i < depth; ++i) w.siblings.push_back(b.priv());
        for (size_t i = 0; i < depth; ++i) w.bits.push_back(b.priv());
    }
    v.amount = b.priv();
    v.R[0] = b.priv(), v.R[1] = b.priv();
    for (size_t i = 0; i < jubjub::kSBits; ++i) v.s_bits.push_back(b.priv());
    const Var amt = b.lin(one, v.amount, zero, kNoVar, zero);
    v.writes[0].new_balance = b.lin(one, v.writes[0].balance, -one, amt, zero);
    v.writes[1].new_balance = b.lin(one, v.writes[1].balance, one, amt, zero);
    b.assert_nonzero(amt);
    b.assert_range(amt, bits);
    b.assert_range(v.writes[0].new_balance, bits);
    b.assert_range(v.writes[1].new_balance, bits);
    const Var keys[2] = {jubjub::hash2_gadget(b, v.pk[0], v.pk[1], p), v.receiver_key};
    for (size_t k = 0; k < 2; ++k) {
        v.writes[k].old_leaf = jubjub::hash2_gadget(b, keys[k], v.writes[k].balance, p);
        v.writes[k].new_leaf = jubjub::hash2_gadget(b, keys[k], v.writes[k].new_balance, p);
    }
    const Var inner = jubjub::hash2_gadget(b, v.receiver_key, amt, p);
    v.m = jubjub::hash2_gadget(b, inner, v.old_root, p);
    for (Var s : v.s_bits) b.assert_bool(s);
    jubjub_schnorr_gadget(b, v.pk, v.m, v.R, v.s_bits, p);
    Var prev = kNoVar;
    for (size_t k = 0; k < 2; ++k) {
        SignedTransferWrite &w = v.writes[k];
        Var old_cur = w.old_leaf, new_cur = w.new_leaf;
        for (size_t i = 0; i < depth; ++i) {
            b.assert_bool(w.bits[i]);
            old_cur = detail::merkle_level(b, old_cur, w.siblings[i], w.bits[i], p);
            new_cur = detail::merkle_level(b, new_cur, w.siblings[i], w.bits[i], p);
        }
        b.assert_equal(old_cur, k == 0 ? v.old_root : prev);
        w.old_out = old_cur, w.new_out = new_cur;
        prev = new_cur;
    }
    b.assert_equal(prev, v.new_root);
    return b.build(layout);
}
inline FrVec jubjub_merkle_signed_transfer_inputs(const CircuitLayout &layout, const SignedTransferVars &v, const Fr &amount, const JjPoint &pk, const Fr &receiver_key,
                                                  const JjSignature &sig, const SignedTransferSide &sender, const SignedTransferSide &receiver) {
    std::vector<std::pair<Var, Fr>> values{{v.amount, amount}, {v.pk[0], pk.x}, {v.pk[1], pk.y}, {v.receiver_key, receiver_key}};
    jubjub::signature_values(values, v.R, v.s_bits, sig);
    const SignedTransferSide *sides[2] = {&sender, &receiver};
    for (size_t k = 0; k < 2; ++k) {
        const SignedTransferWrite &w = v.writes[k];
        const SignedTransferSide &s = *sides[k];
        if (s.siblings.size() != w.siblings.size() || s.bits.size() != w.bits.size()) throw ZkError(ZK_ERR_INVALID, "merkle_signed_transfer_inputs: the path does not have the circuit's depth");
        values.push_back({w.balance, s.balance});
        for (size_t i = 0; i < s.siblings.size(); ++i) values.push_back({w.siblings[i], s.siblings[i]});
        for (size_t i = 0; i < s.bits.size(); ++i) values.push_back({w.bits[i], Fr::from_u64(s.bits[i])});
    }
    return layout.free(values);
}

}  // namespace zkhost
