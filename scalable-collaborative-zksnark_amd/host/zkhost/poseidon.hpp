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
#pragma once
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

// ---- the device ----
inline std::shared_ptr<PoseidonParams> poseidon_params(Ctx &be, const PoseidonConsts &p = poseidon_v1()) { return be.poseidon_params(p.rf, p.rp, p.rc, p.mds); }

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
inline FrVec poseidon_merkle_witness_inputs(const CircuitLayout &layout, const MerkleCircuitVars &v, const Fr &leaf, const FrVec &siblings, const std::vector<uint64_t> &bits) {
    if (siblings.size() != v.siblings.size() || bits.size() != v.bits.size()) throw ZkError(ZK_ERR_INVALID, "poseidon_merkle_witness_inputs: the path does not have the circuit's depth");
    std::vector<std::pair<Var, Fr>> values{{v.leaf, leaf}};
    for (size_t i = 0; i < siblings.size(); ++i) values.push_back({v.siblings[i], siblings[i]});
    for (size_t i = 0; i < bits.size(); ++i) values.push_back({v.bits[i], Fr::from_u64(bits[i])});
    return layout.free(values);
}

}  // namespace zkhost
