// Batch opening (HyperPlonk's): K evaluation claims on J polynomials of one size -> ONE degree-2 sumcheck and ONE opening proof -- the
// compiled counterpart of zkhip/batch_open.py, bit for bit.
//
// J tables f_j of N = 2^n Fr with commitments C_j; K claims (j_k, z_k, v_k) meaning f_{j_k}(z_k) = v_k; a_k = alpha^k; challenges rho.
//     E_j(x) = sum_{k : j_k = j} a_k eq(z_k, x)            (zk_eq_table, zk_eq_table_acc)
//     sum_x sum_j E_j(x) f_j(x) = sum_k a_k v_k =: S       one sumcheck, triples as zk_sumcheck_product (zk_sumcheck_multi)
//     e_j = E_j(rho),  g = sum_j e_j f_j                   (zk_fr_lincomb), opened at rho: g(rho) = y, the value the chain ends in
// The verifier: (1) the chain from S, (2) C_g = sum_j e_j C_j (zk_g1_lincomb), (3) one zk_pcs_verify_batch call of one opening.
// alpha and rho are INPUTS: no Fiat-Shamir.  Single party only.  One instance per table size.
#pragma once
#include <array>
#include <vector>

#include "dist_primitive.hpp"
#include "wiring.hpp"
#include "zerocheck.hpp"

namespace zkhost {

struct Claim {
    size_t table;
    FrVec point;
    Fr value;
};
struct BatchOpenProof {
    std::vector<std::array<Fr, 3>> rounds;  // (t0, t1, t2) per round
    G1Vec opening;                          // the opening proof of g at rho
};

inline void check_claims(const std::vector<Claim> &claims, size_t n_tables, size_t n) {
    if (claims.empty()) throw ZkError(ZK_ERR_INVALID, "batch opening: no claims");
    for (const Claim &c : claims) {
        if (c.table >= n_tables) throw ZkError(ZK_ERR_INVALID, "batch opening: a claim's table index is out of range");
        if (c.point.size() != n) throw ZkError(ZK_ERR_INVALID, "batch opening: a claim's point has the wrong number of coordinates");
    }
}
inline FrVec claim_weights(const Fr &alpha, size_t count) {
    FrVec w(count);
    Fr a = Fr::one();
    for (size_t k = 0; k < count; ++k) w[k] = a, a *= alpha;
    return w;
}
inline Fr claimed_sum(const std::vector<Claim> &claims, const Fr &alpha) {
    const FrVec w = claim_weights(alpha, claims.size());
    Fr s = Fr::zero();
    for (size_t k = 0; k < claims.size(); ++k) s += w[k] * claims[k].value;
    return s;
}
// e_j = sum_{k : j_k = j} a_k eq(z_k, rho)
inline FrVec eq_coefficients(size_t n_tables, const std::vector<Claim> &claims, const Fr &alpha, const FrVec &rho) {
    const FrVec w = claim_weights(alpha, claims.size());
    FrVec e(n_tables, Fr::zero());
    for (size_t k = 0; k < claims.size(); ++k) e[claims[k].table] += w[k] * eq_eval(claims[k].point, rho);
    return e;
}

// E_j on the device (a null DevPtr for a table without claims): the first claim on a table is a_k eq(z_k, .), later ones are added in
inline std::vector<DevPtr> combined_eq_tables(Ctx &be, size_t n_tables, size_t n, const std::vector<Claim> &claims, const Fr &alpha) {
    check_claims(claims, n_tables, n);
    const FrVec w = claim_weights(alpha, claims.size());
    std::vector<DevPtr> tabs(n_tables);
    for (size_t k = 0; k < claims.size(); ++k) {
        DevPtr &t = tabs[claims[k].table];
        if (!t) {
            t = be.eq_table(claims[k].point);
            if (w[k] != Fr::one()) t = be.fr_scale(t, w[k], size_t(1) << n);
        } else {
            be.eq_table_acc(claims[k].point, w[k], t);
        }
    }
    return tabs;
}

inline BatchOpenProof batch_open_prove(Ctx &be, const PowersOfG &pg, const std::vector<DevPtr> &tables, size_t N, const std::vector<Claim> &claims,
                                       const Fr &alpha, const FrVec &rho) {
    const size_t n = rho.size();
    if (n < 1 || N != size_t(1) << n) throw ZkError(ZK_ERR_INVALID, "batch_open_prove: rho must hold one element per variable of the tables");
    std::vector<DevPtr> eqs = combined_eq_tables(be, tables.size(), n, claims, alpha), es, fs;
    for (size_t j = 0; j < tables.size(); ++j)
        if (eqs[j]) es.push_back(eqs[j]), fs.push_back(tables[j]);
    FrVec last_e, last_f;
    ScResult r = be.sumcheck_multi(es, fs, N, rho, last_e, last_f);
    DevPtr g = be.fr_lincomb(fs, last_e, N);
    BatchOpenProof p;
    p.rounds.resize(n);
    for (size_t i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) p.rounds[i][k] = r.sums[3 * i + k];
    p.opening = open(be, pg, g, N, rho).proofs;
    return p;
}

// The verifier's field arithmetic (no GPU) -> a bit per failed check (0: all hold; bit 0: a malformed record or statement):
//   1. p_0(0) + p_0(1) == S and p_i(0) + p_i(1) == p_{i-1}(rho_{i-1}), on the nodes 0 .. 2 (round_chain.hpp; dsumcheck.rs:558-588);  y (optional) receives p_{n-1}(rho_{n-1});
//   2. only when finals = the J values f_j(rho) are given: y == sum_j e_j f_j(rho) (the real verifier gets this from the pairing).
inline unsigned failed_checks(size_t n_tables, const std::vector<Claim> &claims, const BatchOpenProof &proof, const Fr &alpha, const FrVec &rho,
                              Fr *y = nullptr, const FrVec *finals = nullptr) {
    const size_t n = rho.size();
    if (n == 0 || proof.rounds.size() != n || proof.opening.size() != n || claims.empty()) return 1u;
    for (const Claim &c : claims)
        if (c.table >= n_tables || c.point.size() != n) return 1u;
    Fr target;
    if (!round_chain(proof.rounds, 3, rho, claimed_sum(claims, alpha), &target)) return 1u << 1;
    if (y) *y = target;
    if (finals) {
        const FrVec e = eq_coefficients(n_tables, claims, alpha, rho);
        Fr s = Fr::zero();
        for (size_t j = 0; j < n_tables && j < finals->size(); ++j) s += e[j] * (*finals)[j];
        if (s != target) return 1u << 2;
    }
    return 0;
}
inline bool verify_rounds(size_t n_tables, const std::vector<Claim> &claims, const BatchOpenProof &proof, const Fr &alpha, const FrVec &rho) {
    return failed_checks(n_tables, claims, proof, alpha, rho) == 0;
}

// C_g = sum_j e_j C_j (zk_g1_lincomb: canonical scalars)
inline G1 combined_commitment(Ctx &be, const G1Vec &commitments, const std::vector<Claim> &claims, const Fr &alpha, const FrVec &rho) {
    FrVec e = eq_coefficients(commitments.size(), claims, alpha, rho);
    for (Fr &x : e) x = x.to_canonical();
    return be.g1_lincomb_batch(commitments, e, 1)[0];
}

// check 3: the single opening (C_g, y, proof, rho) through zk_pcs_verify_batch
inline bool verify_opening(Ctx &be, const PcsVk &vk, const G1Vec &commitments, const std::vector<Claim> &claims, const BatchOpenProof &proof, const Fr &alpha,
                           const FrVec &rho, const Fr &y) {
    return verify(be, vk, combined_commitment(be, commitments, claims, alpha, rho), y, proof.opening, rho);
}
inline bool batch_open_verify(Ctx &be, const PcsVk &vk, const G1Vec &commitments, const std::vector<Claim> &claims, const BatchOpenProof &proof,
                              const Fr &alpha, const FrVec &rho) {
    Fr y;
    if (failed_checks(commitments.size(), claims, proof, alpha, rho, &y)) return false;
    return verify_opening(be, vk, commitments, claims, proof, alpha, rho, y);
}

// what batch_open_verify hands to the pairing, without calling the device: the opening of sum_j e_j C_j at rho with the chain's value y,
// added to `out` as one opening of verify_agg (zkhip.batch_open.opening_claim).  false, and nothing added, when the chain breaks
inline bool opening_claim(const G1Vec &commitments, const std::vector<Claim> &claims, const BatchOpenProof &proof, const Fr &alpha, const FrVec &rho, size_t skip,
                          AggArrays &out) {
    Fr y;
    if (failed_checks(commitments.size(), claims, proof, alpha, rho, &y)) return false;
    out.add(commitments, eq_coefficients(commitments.size(), claims, alpha, rho), y, proof.opening, rho, skip);
    return true;
}

// [(j, z)] -> claims with v = f_j(z) by zk_fold
inline std::vector<Claim> evaluate_claims(Ctx &be, const std::vector<DevPtr> &tables, size_t N, const std::vector<std::pair<size_t, FrVec>> &points) {
    std::vector<Claim> out;
    for (auto &p : points) out.push_back(Claim{p.first, p.second, be.to_host(be.fold(tables[p.first], N, p.second), 1)[0]});
    return out;
}

// ---- users: the gate ZeroCheck and the wiring PermCheck with their openings batched ----
struct GateProofBatched {
    std::vector<std::array<Fr, 5>> rounds;
    G1Vec commitments;  // in the order of kGateOpened
    FrVec values;
    BatchOpenProof batch;
};
inline GateProofBatched gate_zerocheck_prove_batched(Ctx &be, const PowersOfG &pg, const GateTables &t, const FrVec &tau, const FrVec &chal, const Fr &alpha,
                                                     const FrVec &rho) {
    const size_t n = tau.size(), len = size_t(1) << n;
    if (n < 1 || chal.size() != n) throw ZkError(ZK_ERR_INVALID, "gate_zerocheck_prove_batched: tau and chal must hold one element per variable");
    DevPtr eq = be.eq_table(tau);
    FrVec last;
    ScResult sc = be.sumcheck_gate({eq, t.at("q1"), t.at("q2"), t.at("a"), t.at("b"), t.at("c"), t.at("in")}, len, chal, last);
    GateProofBatched p;
    p.rounds.resize(n);
    for (size_t i = 0; i < n; ++i)
        for (int k = 0; k < 5; ++k) p.rounds[i][k] = sc.sums[5 * i + k];
    p.values = {last[3], last[4], last[5], last[6], last[1], last[2]};  // a, b, c, in, q1, q2: the folded-out values ARE f(r)
    std::vector<DevPtr> tabs;
    std::vector<Claim> claims;
    for (size_t k = 0; k < 6; ++k) {
        tabs.push_back(t.at(kGateOpened[k]));
        p.commitments.push_back(commit(be, pg, tabs[k], len));
        claims.push_back(Claim{k, chal, p.values[k]});
    }
    p.batch = batch_open_prove(be, pg, tabs, len, claims, alpha, rho);
    return p;
}
inline bool gate_zerocheck_verify_batched(Ctx &be, const PcsVk &vk, const GateProofBatched &p, const FrVec &tau, const FrVec &chal, const Fr &alpha,
                                          const FrVec &rho) {
    if (p.values.size() != 6 || p.commitments.size() != 6) return false;
    GateProof rec;
    rec.rounds = p.rounds;
    std::vector<Claim> claims;
    for (size_t k = 0; k < 6; ++k) {
        GateOpening o;
        o.commitment = p.commitments[k], o.value = p.values[k];
        rec.openings.push_back(o);
        claims.push_back(Claim{k, chal, p.values[k]});
    }
    return verify_rounds(rec, tau, chal) && batch_open_verify(be, vk, p.commitments, claims, p.batch, alpha, rho);
}

struct WiringProofBatched {
    std::vector<std::array<Fr, 4>> rounds;
    G1Vec commitments;  // w, sid, ssigma
    FrVec values;
    G1 v_commitment;
    FrVec v_values;  // the tree at the five v_points
    BatchOpenProof batch, v_batch;
};
inline WiringProofBatched wiring_prove_batched(Ctx &be, const PowersOfG &pg, const DevPtr &w, const DevPtr &sid, const DevPtr &ssigma, size_t N,
                                               const WiringScalars &sc, const Fr &b_alpha, const FrVec &rho_mu, const FrVec &rho_mu1) {
    const size_t mu = sc.tau.size();
    if (mu < 1 || sc.chal.size() != mu || N != size_t(1) << mu) throw ZkError(ZK_ERR_INVALID, "wiring_prove_batched: tau and chal must hold one element per variable");
    DevPtr num = be.fr_axpb(w, sid, sc.alpha, sc.beta, N), den = be.fr_axpb(w, ssigma, sc.alpha, sc.beta, N);
    DevPtr h = be.fr_batch_div(num, den, N);
    DevPtr tree = be.product_tree(h, N);
    DevPtr eq = be.eq_table(sc.tau);
    FrVec last;
    ScResult r = be.sumcheck_wiring(eq, tree, num, den, N, sc.gamma, sc.chal, last);
    WiringProofBatched p;
    p.rounds.resize(mu);
    for (size_t i = 0; i < mu; ++i)
        for (int k = 0; k < 4; ++k) p.rounds[i][k] = r.sums[4 * i + k];
    const std::vector<DevPtr> tabs = {w, sid, ssigma};
    for (const DevPtr &t : tabs) p.commitments.push_back(commit(be, pg, t, N));
    p.v_commitment = commit(be, pg, tree, 2 * N);
    std::vector<std::pair<size_t, FrVec>> pts = {{0, sc.chal}, {1, sc.chal}, {2, sc.chal}}, vpts;
    for (const FrVec &z : v_points(sc.chal)) vpts.push_back({0, z});
    const std::vector<Claim> claims = evaluate_claims(be, tabs, N, pts), v_claims = evaluate_claims(be, {tree}, 2 * N, vpts);
    for (const Claim &c : claims) p.values.push_back(c.value);
    for (const Claim &c : v_claims) p.v_values.push_back(c.value);
    p.batch = batch_open_prove(be, pg, tabs, N, claims, b_alpha, rho_mu);
    p.v_batch = batch_open_prove(be, pg, {tree}, 2 * N, v_claims, b_alpha, rho_mu1);
    return p;
}
inline bool wiring_verify_batched(Ctx &be, const PcsVk &vk_mu, const PcsVk &vk_mu1, const WiringProofBatched &p, const WiringScalars &sc, const Fr &b_alpha,
                                  const FrVec &rho_mu, const FrVec &rho_mu1) {
    if (p.values.size() != 3 || p.commitments.size() != 3 || p.v_values.size() != 5) return false;
    WiringProof rec;
    rec.rounds = p.rounds;
    std::vector<Claim> claims, v_claims;
    for (size_t k = 0; k < 3; ++k) {
        GateOpening o;
        o.commitment = p.commitments[k], o.value = p.values[k];
        rec.openings.push_back(o);
        claims.push_back(Claim{k, sc.chal, p.values[k]});
    }
    const std::vector<FrVec> vp = v_points(sc.chal);
    for (size_t k = 0; k < 5; ++k) {
        rec.v_openings.push_back(Opening{p.v_values[k], {}});
        v_claims.push_back(Claim{0, vp[k], p.v_values[k]});
    }
    if (failed_checks(rec, sc)) return false;
    return batch_open_verify(be, vk_mu, p.commitments, claims, p.batch, b_alpha, rho_mu) &&
           batch_open_verify(be, vk_mu1, G1Vec{p.v_commitment}, v_claims, p.v_batch, b_alpha, rho_mu1);
}

}  // namespace zkhost
