// Poseidon over BLS12-381 Fr at t = 3 -- the compiled mirror of zkhip/poseidon.py: the instance "zkhip-poseidon-v1", the rule on the host
// (serial, on zkhost's Fr), the device calls through Ctx::poseidon_*, and the permutation / Merkle-path gadgets on CircuitBuilder.
//
// THE RULE (include/zkhip.h).  State (s_0, s_1, s_2), S-box x^5, rf full rounds (rf / 2 first, rf / 2 last) around rp partial rounds, one
// counter k over all rf + rp rounds:
//     full round k      s_i += rc[3k + i] for i = 0, 1, 2;  every s_i <- s_i^5;  s <- M s
//     partial round k   s_i += rc[3k + i] for i = 0, 1, 2;  only  s_0 <- s_0^5;  s <- M s
//     hash2(l, r) = permute(0, l, r)[0];   a Merkle node = hash2(left child, right child);   a tree of n leaves: 2n - 1 elements, root last.
// THE INSTANCE v1: rf = 8, rp = 57;  rc[k] = int_le(SHA-256(tag || u32le(k) || 0x00) || SHA-256(tag || u32le(k) || 0x01)) mod r, k < 195,
// tag = "zkhip-poseidon-v1";  M[i][j] = 1 / (i + j + 3), a Cauchy matrix and hence MDS.  It is SELF-DEFINED: not claimed to equal any other
// library's constants, and the paper's further checks of the matrix (invariant-subspace trails) have NOT been done.  That is why the
// constants are a value (PoseidonConsts) here and a parameter object on the device.
// THE CIRCUIT: a round's constant addition is folded into the qC of the previous linear layer's rows, the first round's constants take
// three lin rows; a full round is 9 rows, a partial round 7, the v1 permutation 474; a Merkle level is 480 rows (zkhip/poseidon.py).
// A TREE KEPT ON THE DEVICE: poseidon_paths_host / poseidon_update_host (the rules), poseidon_update / poseidon_verify_paths over
// Ctx::poseidon_merkle_paths / _roots / _update, and poseidon_merkle_update_circuit: 959 rows per level and write.
#pragma once
#include <algorithm>
#include <cstring>
#include <string>

#include "circuit.hpp"

namespace zkhost {

struct PoseidonConsts {
    int rf = 0, rp = 0;
    FrVec rc, mds;  // 3 (rf + rp) round constants; 9 matrix entries, row-major
};

namespace detail {
// the 512-bit little-endian integer in w[0..63] mod r, as an Fr: Horner over the bytes from the top
inline Fr fr_from_le_bytes_wide(const uint8_t *w, size_t n) {
    const Fr base = Fr::from_u64(256);
    Fr acc = Fr::zero();
    for (size_t i = n; i-- > 0;) acc = acc * base + Fr::from_u64(w[i]);
    return acc;
}
}  // namespace detail

inline const PoseidonConsts &poseidon_v1() {
    static const PoseidonConsts k = [] {
        PoseidonConsts p;
        p.rf = 8, p.rp = 57;
        const char tag[] = "zkhip-poseidon-v1";
        for (uint32_t i = 0; i < 3 * 65; ++i) {
            uint8_t wide[64];
            for (uint8_t half = 0; half < 2; ++half) {
                Sha256 h;
                const uint8_t le[5] = {uint8_t(i), uint8_t(i >> 8), uint8_t(i >> 16), uint8_t(i >> 24), half};
                h.update(tag, sizeof tag - 1);
                h.update(le, 5);
                h.digest(wide + 32 * half);
            }
            p.rc.push_back(detail::fr_from_le_bytes_wide(wide, 64));
        }
        for (uint64_t i = 0; i < 3; ++i)
            for (uint64_t j = 0; j < 3; ++j) p.mds.push_back(Fr::from_u64(i + j + 3).inverse());
        return p;
    }();
    return k;
}

// ---- the rule on the host ----
inline std::array<Fr, 3> poseidon_permute_host(std::array<Fr, 3> s, const PoseidonConsts &p = poseidon_v1()) {
    const size_t half = (size_t)p.rf / 2, rp = (size_t)p.rp;
    auto pow5 = [](const Fr &x) {
        const Fr x2 = x * x;
        return x2 * x2 * x;
    };
    for (size_t k = 0; k < 2 * half + rp; ++k) {
        for (size_t i = 0; i < 3; ++i) s[i] += p.rc[3 * k + i];
        s[0] = pow5(s[0]);
        if (k < half || k >= half + rp) s[1] = pow5(s[1]), s[2] = pow5(s[2]);
        std::array<Fr, 3> t;
        for (size_t i = 0; i < 3; ++i) t[i] = p.mds[3 * i] * s[0] + p.mds[3 * i + 1] * s[1] + p.mds[3 * i + 2] * s[2];
        s = t;
    }
    return s;
}
inline Fr poseidon_hash2_host(const Fr &l, const Fr &r, const PoseidonConsts &p = poseidon_v1()) { return poseidon_permute_host({Fr::zero(), l, r}, p)[0]; }
inline FrVec poseidon_merkle_host(const FrVec &leaves, const PoseidonConsts &p = poseidon_v1()) {
    const size_t n = leaves.size();
    if (n == 0 || (n & (n - 1))) throw ZkError(ZK_ERR_INVALID, "poseidon_merkle_host: the number of leaves must be a power of two");
    FrVec tree = leaves;
    for (size_t lo = 0, cnt = n; cnt > 1; lo += cnt, cnt /= 2)
        for (size_t i = 0; i < cnt / 2; ++i) tree.push_back(poseidon_hash2_host(tree[lo + 2 * i], tree[lo + 2 * i + 1], p));
    return tree;
}
// siblings and bits of leaf `index` from the leaf level up; bit = 1: the running node is the right child
inline void poseidon_merkle_path(const FrVec &tree, size_t n, size_t index, FrVec &siblings, std::vector<uint64_t> &bits) {
    if (index >= n || tree.size() != 2 * n - 1) throw ZkError(ZK_ERR_INVALID, "poseidon_merkle_path: no such leaf");
    siblings.clear(), bits.clear();
    for (size_t lo = 0, cnt = n; cnt > 1; lo += cnt, cnt /= 2, index >>= 1) {
        siblings.push_back(tree[lo + (index ^ 1)]);
        bits.push_back(index & 1);
    }
}


// ---- a tree that is opened and updated: the host rules of zk_poseidon_merkle_paths / _update, with the library's refusals ----
namespace detail {
inline size_t merkle_depth(const FrVec &tree, size_t n) {
    if (n == 0 || (n & (n - 1)) || tree.size() != 2 * n - 1) throw ZkError(ZK_ERR_INVALID, "a tree of n = 2^d leaves has 2n - 1 elements");
    size_t d = 0;
    while ((size_t(1) << d) < n) ++d;
    return d;
}
inline void refuse_not_below(const char *what, const std::vector<uint64_t> &index, uint64_t n) {
    size_t bad = 0, first = 0;
    for (size_t k = index.size(); k-- > 0;)
        if (index[k] >= n) ++bad, first = k;
    if (bad)
        throw ZkError(ZK_ERR_INVALID, std::string(what) + ": " + std::to_string(bad) + " of " + std::to_string(index.size()) + " indices are not below n = " + std::to_string(n) +
                                          "; the first is position " + std::to_string(first));
}
}  // namespace detail
// one vector of d siblings per index, from the leaf level up; the bits of a path are the bits of its index
inline std::vector<FrVec> poseidon_paths_host(const FrVec &tree, size_t n, const std::vector<uint64_t> &index) {
    detail::merkle_depth(tree, n);
    detail::refuse_not_below("zk_poseidon_merkle_paths", index, n);
    std::vector<FrVec> out(index.size());
    std::vector<uint64_t> bits;
    for (size_t k = 0; k < index.size(); ++k) poseidon_merkle_path(tree, n, (size_t)index[k], out[k], bits);
    return out;
}
// a NEW tree: the writes (index, value) applied in order -- any order, repeats allowed, the last write of a leaf wins -- and only the nodes
// above a written leaf hashed again
inline FrVec poseidon_update_host(const FrVec &tree, size_t n, const std::vector<std::pair<uint64_t, Fr>> &writes, const PoseidonConsts &p = poseidon_v1()) {
    const size_t d = detail::merkle_depth(tree, n);
    std::vector<uint64_t> touched;
    for (const auto &w : writes) touched.push_back(w.first);
    detail::refuse_not_below("zk_poseidon_merkle_update", touched, n);
    FrVec out = tree;
    for (const auto &w : writes) out[(size_t)w.first] = w.second;
    std::sort(touched.begin(), touched.end());
    size_t lo = 0;
    for (size_t j = 0; j < d; ++j) {
        for (uint64_t &i : touched) i >>= 1;
        touched.erase(std::unique(touched.begin(), touched.end()), touched.end());
        for (uint64_t q : touched) out[lo + (n >> j) + q] = poseidon_hash2_host(out[lo + 2 * q], out[lo + 2 * q + 1], p);
        lo += n >> j;
    }
    return out;
}

// ---- the device ----
inline std::shared_ptr<PoseidonParams> poseidon_params(Ctx &be, const PoseidonConsts &p = poseidon_v1()) { return be.poseidon_params(p.rf, p.rp, p.rc, p.mds); }
// writes in any order, repeats allowed: sorted by index (stable), the last write of a leaf kept, then Ctx::poseidon_merkle_update.  Asynchronous
inline void poseidon_update(Ctx &be, const PoseidonParams &pp, const DevPtr &tree, size_t n, const std::vector<std::pair<uint64_t, Fr>> &writes) {
    std::vector<size_t> order(writes.size());
    for (size_t k = 0; k < order.size(); ++k) order[k] = k;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return writes[a].first < writes[b].first; });
    std::vector<uint64_t> index;
    FrVec values;
    for (size_t k = 0; k < order.size(); ++k)
        if (k + 1 == order.size() || writes[order[k + 1]].first != writes[order[k]].first) index.push_back(writes[order[k]].first), values.push_back(writes[order[k]].second);
    be.poseidon_merkle_update(pp, tree, n, index, be.to_device(values));
}
// per path: does it reach `root`?  Blocking: the roots are read back
inline std::vector<bool> poseidon_verify_paths(Ctx &be, const PoseidonParams &pp, const Fr &root, const DevPtr &leaves, const std::vector<uint64_t> &index, const DevPtr &siblings,
                                               size_t depth) {
    const FrVec got = be.to_host(be.poseidon_merkle_roots(pp, leaves, index, siblings, depth), index.size());
    std::vector<bool> ok(got.size());
    for (size_t k = 0; k < got.size(); ++k) ok[k] = std::memcmp(got[k].v, root.v, 32) == 0;
    return ok;
}

// ---- the circuit ----
inline std::array<Var, 3> poseidon_permutation_gadget(CircuitBuilder &b, const std::array<Var, 3> &state, const PoseidonConsts &p = poseidon_v1()) {
    const size_t half = (size_t)p.rf / 2, rp = (size_t)p.rp, rounds = 2 * half + rp;
    const Fr one = Fr::one(), zero = Fr::zero();
    std::array<Var, 3> s;
    for (size_t i = 0; i < 3; ++i) s[i] = b.lin(one, state[i], zero, kNoVar, p.rc[i]);
    for (size_t k = 0; k < rounds; ++k) {
        const bool full = k < half || k >= half + rp;
        std::array<Var, 3> u;
        u[0] = b.pow5(s[0]);
        u[1] = full ? b.pow5(s[1]) : s[1];
        u[2] = full ? b.pow5(s[2]) : s[2];
        for (size_t i = 0; i < 3; ++i) {
            const Var t = b.lin(p.mds[3 * i], u[0], p.mds[3 * i + 1], u[1], zero);
            s[i] = b.lin(one, t, p.mds[3 * i + 2], u[2], k + 1 < rounds ? p.rc[3 * (k + 1) + i] : zero);
        }
    }
    return s;
}

struct MerkleCircuitVars {
    Var root = kNoVar, leaf = kNoVar, out = kNoVar;
    std::vector<Var> siblings, bits;
};
// one public input (the root); private: the leaf, `depth` siblings, `depth` bits (zkhip.poseidon.merkle_circuit)
inline PlonkCircuit poseidon_merkle_circuit(size_t depth, CircuitLayout &layout, MerkleCircuitVars &v, const PoseidonConsts &p = poseidon_v1()) {
    if (depth < 1) throw ZkError(ZK_ERR_INVALID, "poseidon_merkle_circuit: depth >= 1 is needed");
    CircuitBuilder b;
    const Fr one = Fr::one(), zero = Fr::zero(), minus = -Fr::one();
    v = MerkleCircuitVars();
    v.root = b.pub();
    v.leaf = b.priv();
    for (size_t i = 0; i < depth; ++i) v.siblings.push_back(b.priv());
    for (size_t i = 0; i < depth; ++i) v.bits.push_back(b.priv());
    Var cur = v.leaf;
    for (size_t i = 0; i < depth; ++i) {
        const Var sib = v.siblings[i], bit = v.bits[i];
        b.assert_bool(bit);
        const Var d = b.lin(one, sib, minus, cur, zero);
        const Var e = b.mul(bit, d);
        const Var left = b.lin(one, cur, one, e, zero), right = b.lin(one, sib, minus, e, zero);
        const Var z = b.lin(zero, kNoVar, zero, kNoVar, zero);
        cur = poseidon_permutation_gadget(b, {z, left, right}, p)[0];
    }
    b.assert_equal(cur, v.root);
    v.out = cur;
    return b.build(layout);
}

// "`count` chained leaf writes take the public old root to the public new root" (zkhip.poseidon.merkle_update_circuit, row for row): two public
// inputs; private, per write: old leaf, new leaf, `depth` siblings, `depth` bits.  Per level ONE assert_bool(bit) row, then the five selection rows
// and the permutation (479 rows) on the old running node and again on the new one, against the same sibling and bit: 959 rows per level,
// 2 + 959 depth count in all.  The first old chain joins the old root's copy class, every later old chain the new chain before it, the last new
// chain the new root's.
struct MerkleUpdateWrite {
    Var old_leaf = kNoVar, new_leaf = kNoVar, old_out = kNoVar, new_out = kNoVar;
    std::vector<Var> siblings, bits;
};
struct MerkleUpdateVars {
    Var old_root = kNoVar, new_root = kNoVar;
    std::vector<MerkleUpdateWrite> writes;
};
struct MerkleUpdateStep {  // one write of a chain, on the tree before it
    Fr old_leaf, new_leaf;
    FrVec siblings;
    std::vector<uint64_t> bits;
};
namespace detail {
inline Var merkle_level(CircuitBuilder &b, Var cur, Var sib, Var bit, const PoseidonConsts &p) {
    const Fr one = Fr::one(), zero = Fr::zero(), minus = -Fr::one();
    const Var d = b.lin(one, sib, minus, cur, zero);
    const Var e = b.mul(bit, d);
    const Var left = b.lin(one, cur, one, e, zero), right = b.lin(one, sib, minus, e, zero);
    const Var z = b.lin(zero, kNoVar, zero, kNoVar, zero);
    return poseidon_permutation_gadget(b, {z, left, right}, p)[0];
}
}  // namespace detail
inline PlonkCircuit poseidon_merkle_update_circuit(size_t depth, size_t count, CircuitLayout &layout, MerkleUpdateVars &v, const PoseidonConsts &p = poseidon_v1()) {
    if (depth < 1 || count < 1) throw ZkError(ZK_ERR_INVALID, "poseidon_merkle_update_circuit: depth >= 1 and count >= 1 are needed");
    CircuitBuilder b;
    v = MerkleUpdateVars();
    v.old_root = b.pub();
    v.new_root = b.pub();
    v.writes.resize(count);
    for (MerkleUpdateWrite &w : v.writes) {
        w.old_leaf = b.priv();
        w.new_leaf = b.priv();
        for (size_t i = 0; i < depth; ++i) w.siblings.push_back(b.priv());
        for (size_t i = 0; i < depth; ++i) w.bits.push_back(b.priv());
    }
    Var prev = kNoVar;
    for (size_t k = 0; k < count; ++k) {
        MerkleUpdateWrite &w = v.writes[k];
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
inline FrVec poseidon_merkle_update_inputs(const CircuitLayout &layout, const MerkleUpdateVars &v, const std::vector<MerkleUpdateStep> &steps) {
    if (steps.size() != v.writes.size()) throw ZkError(ZK_ERR_INVALID, "poseidon_merkle_update_inputs: the chain does not have the circuit's number of writes");
    std::vector<std::pair<Var, Fr>> values;
    for (size_t k = 0; k < steps.size(); ++k) {
        const MerkleUpdateWrite &w = v.writes[k];
        const MerkleUpdateStep &s = steps[k];
        if (s.siblings.size() != w.siblings.size() || s.bits.size() != w.bits.size()) throw ZkError(ZK_ERR_INVALID, "poseidon_merkle_update_inputs: the path does not have the circuit's depth");
        values.push_back({w.old_leaf, s.old_leaf});
        values.push_back({w.new_leaf, s.new_leaf});
        for (size_t i = 0; i < s.siblings.size(); ++i) values.push_back({w.siblings[i], s.siblings[i]});
        for (size_t i = 0; i < s.bits.size(); ++i) values.push_back({w.bits[i], Fr::from_u64(s.bits[i])});
    }
    return layout.free(values);
}
// "the tree with public root R became the tree with public root R' by moving a private non-zero amount from one leaf to another; the amount
// and both new balances lie below 2^bits" (zkhip.poseidon.merkle_transfer_circuit, row for row): the update circuit with count = 2 whose new
// leaves are computed -- amt = amount (a lin copy), new_from = old_from - amt, new_to = old_to + amt, assert_nonzero(amt), assert_range of amt,
// new_from, new_to -- before the two writes' levels.  Every inverse and bit is advice, generated on the device.  v.writes[k].new_leaf names
// the computed row; write 0 is the sender, write 1 the receiver (its path is one of the tree after write 0)
struct MerkleTransferSide {  // one side of a transfer, on the tree before its write
    Fr old_leaf;
    FrVec siblings;
    std::vector<uint64_t> bits;
};
inline PlonkCircuit poseidon_merkle_transfer_circuit(size_t depth, size_t bits, CircuitLayout &layout, MerkleUpdateVars &v, Var &amount, const PoseidonConsts &p = poseidon_v1()) {
    if (depth < 1 || bits < 1 || bits > 253) throw ZkError(ZK_ERR_INVALID, "poseidon_merkle_transfer_circuit: depth >= 1 and 1 <= bits <= 253 are needed");
    CircuitBuilder b;
    v = MerkleUpdateVars();
    v.old_root = b.pub();
    v.new_root = b.pub();
    v.writes.resize(2);
    for (MerkleUpdateWrite &w : v.writes) {
        w.old_leaf = b.priv();
        for (size_t i = 0; i < depth; ++i) w.siblings.push_back(b.priv());
        for (size_t i = 0; i < depth; ++i) w.bits.push_back(b.priv());
    }
    amount = b.priv();
    const Fr one = Fr::one(), zero = Fr::zero();
    const Var amt = b.lin(one, amount, zero, kNoVar, zero);
    v.writes[0].new_leaf = b.lin(one, v.writes[0].old_leaf, -one, amt, zero);
    v.writes[1].new_leaf = b.lin(one, v.writes[1].old_leaf, one, amt, zero);
    b.assert_nonzero(amt);
    b.assert_range(amt, bits);
    b.assert_range(v.writes[0].new_leaf, bits);
    b.assert_range(v.writes[1].new_leaf, bits);
    Var prev = kNoVar;
    for (size_t k = 0; k < 2; ++k) {
        MerkleUpdateWrite &w = v.writes[k];
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
inline FrVec poseidon_merkle_transfer_inputs(const CircuitLayout &layout, const MerkleUpdateVars &v, Var amount, const Fr &amount_value, const MerkleTransferSide &sender,
                                             const MerkleTransferSide &receiver) {
    std::vector<std::pair<Var, Fr>> values{{amount, amount_value}};
    const MerkleTransferSide *sides[2] = {&sender, &receiver};
    for (size_t k = 0; k < 2; ++k) {
        const MerkleUpdateWrite &w = v.writes[k];
        const MerkleTransferSide &s = *sides[k];
        if (s.siblings.size() != w.siblings.size() || s.bits.size() != w.bits.size()) throw ZkError(ZK_ERR_INVALID, "poseidon_merkle_transfer_inputs: the path does not have the circuit's depth");
        values.push_back({w.old_leaf, s.old_leaf});
        for (size_t i = 0; i < s.siblings.size(); ++i) values.push_back({w.siblings[i], s.siblings[i]});
        for (size_t i = 0; i < s.bits.size(); ++i) values.push_back({w.bits[i], Fr::from_u64(s.bits[i])});
    }
    return layout.free(values);
}
inline FrVec poseidon_merkle_witness_inputs(const CircuitLayout &layout, const MerkleCircuitVars &v, const Fr &leaf, const FrVec &siblings, const std::vector<uint64_t> &bits) {
    if (siblings.size() != v.siblings.size() || bits.size() != v.bits.size()) throw ZkError(ZK_ERR_INVALID, "poseidon_merkle_witness_inputs: the path does not have the circuit's depth");
    std::vector<std::pair<Var, Fr>> values{{v.leaf, leaf}};
    for (size_t i = 0; i < siblings.size(); ++i) values.push_back({v.siblings[i], siblings[i]});
    for (size_t i = 0; i < bits.size(); ++i) values.push_back({v.bits[i], Fr::from_u64(bits[i])});
    return layout.free(values);
}

}  // namespace zkhost
