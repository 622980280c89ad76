// The wiring identity as a PermCheck (HyperPlonk's ProductCheck) a verifier can check end to end -- the compiled counterpart of
// zkhip/wiring.py, bit for bit.
//
// The reference SIMULATES the wiring check: a random `eq` vector, six unrelated committed polynomials, six independent product
// sumchecks and nothing that ties the grand product to 1 (hyperplonk/src/hyperplonk.rs:94-141).  Here, with N = 2^mu wire slots,
//     num = w + alpha sid + beta,  den = w + alpha ssigma + beta,  h = num / den,  v = product_tree(h)   (2N elements)
//     v(0,x) = tree[x] = h,  v(1,x) = tree[N + x],  v(x,0) = tree[2x],  v(x,1) = tree[2x + 1]          (index bit 0 = the TOP bit)
//     sum_x eq(tau, x) [ v(1,x) - v(x,0) v(x,1) + gamma ( den(x) h(x) - num(x) ) ] = 0
// is proved by ONE degree-3 sumcheck (zk_eq_table, zk_sumcheck_wiring), closed by openings of w, sid, ssigma at the sumcheck point r
// and of ONE commitment to the tree at (0,r), (1,r), (r,0), (r,1), (1,..,1,0), and verified with the device pairing: the SRS has
// mu + 1 variables and a mu-variate table uses the last mu of them, so there are two verifying keys and two zk_pcs_verify_batch calls.
//
// alpha, beta, gamma, tau and the challenges are INPUTS, as everywhere in this code base: Fiat-Shamir is out of scope.  Single party only.
#pragma once
#include <array>
#include <chrono>
#include <vector>

#include "dist_primitive.hpp"
#include "zerocheck.hpp"

namespace zkhost {

struct WiringProof {
    std::vector<std::array<Fr, 4>> rounds;  // the round polynomial at t = 0 .. 3
    std::vector<GateOpening> openings;      // w, sid, ssigma at r
    G1 v_commitment;                        // the tree
    std::vector<Opening> v_openings;        // at (0,r), (1,r), (r,0), (r,1), (1,..,1,0)
};
struct WiringScalars {
    Fr alpha, beta, gamma;
    FrVec tau, chal;
};

// the five (mu + 1)-variate points at which the tree is opened
inline std::vector<FrVec> v_points(const FrVec &r) {
    std::vector<FrVec> p(5, r);
    p[0].insert(p[0].begin(), Fr::zero());
    p[1].insert(p[1].begin(), Fr::one());
    p[2].push_back(Fr::zero());
    p[3].push_back(Fr::one());
    p[4].assign(r.size(), Fr::one());
    p[4].push_back(Fr::zero());
    return p;
}

// The verifier's field arithmetic (no GPU) -> a bit per failed check (0: all hold; bit 0: a malformed record):
//   1. p_0(0) + p_0(1) == 0 and p_i(0) + p_i(1) == p_{i-1}(r_{i-1}), on the nodes 0 .. 3 (round_chain.hpp);
//   2. p_{mu-1}(r_{mu-1}) == eq(tau, r) [ v(1,r) - v(r,0) v(r,1) + gamma ((w + alpha ssigma + beta) v(0,r) - (w + alpha sid + beta)) ];
//   3. the opened v(1,..,1,0) == 1.
inline unsigned failed_checks(const WiringProof &proof, const WiringScalars &sc) {
    const size_t mu = proof.rounds.size();
    if (mu == 0 || sc.tau.size() != mu || sc.chal.size() != mu || proof.openings.size() != 3 || proof.v_openings.size() != 5) return 1u;
    unsigned bad = 0;
    Fr target;
    if (!round_chain(proof.rounds, 4, sc.chal, Fr::zero(), &target)) bad |= 1u << 1;
    const Fr &w = proof.openings[0].value, &sid = proof.openings[1].value, &ssigma = proof.openings[2].value;
    const Fr &v0r = proof.v_openings[0].value, &v1r = proof.v_openings[1].value, &vr0 = proof.v_openings[2].value, &vr1 = proof.v_openings[3].value;
    const Fr num = w + sc.alpha * sid + sc.beta, den = w + sc.alpha * ssigma + sc.beta;
    if (!bad && target != eq_eval(sc.tau, sc.chal) * (v1r - vr0 * vr1 + sc.gamma * (den * v0r - num))) bad |= 1u << 2;
    if (proof.v_openings[4].value != Fr::one()) bad |= 1u << 3;
    return bad;
}
inline bool verify_rounds(const WiringProof &proof, const WiringScalars &sc) { return failed_checks(proof, sc) == 0; }

// num, den, h, the tree, the eq table, the wiring sumcheck, the commitments and the eight openings.  pg: a parameter set over mu + 1
// variables.  A zero denominator throws ZkError(ZK_ERR_DIV_ZERO).  seconds (optional): [derived tables, sumcheck]
inline WiringProof wiring_prove(Ctx &be, const PowersOfG &pg, const DevPtr &w, const DevPtr &sid, const DevPtr &ssigma, size_t N, const WiringScalars &sc,
                                double *seconds = nullptr) {
    const size_t mu = sc.tau.size();
    if (mu < 1 || sc.chal.size() != mu || N != size_t(1) << mu) throw ZkError(ZK_ERR_INVALID, "wiring_prove: tau and chal must hold one element per variable");
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t0 = now();
    DevPtr num = be.fr_axpb(w, sid, sc.alpha, sc.beta, N), den = be.fr_axpb(w, ssigma, sc.alpha, sc.beta, N);
    DevPtr h = be.fr_batch_div(num, den, N);
    DevPtr tree = be.product_tree(h, N);
    DevPtr eq = be.eq_table(sc.tau);
    be.sync();
    const double t1 = now();
    FrVec last;
    ScResult r = be.sumcheck_wiring(eq, tree, num, den, N, sc.gamma, sc.chal, last);
    const double t2 = now();
    if (seconds) seconds[0] = t1 - t0, seconds[1] = t2 - t1;
    WiringProof p;
    p.rounds.resize(mu);
    for (size_t i = 0; i < mu; ++i)
        for (int k = 0; k < 4; ++k) p.rounds[i][k] = r.sums[4 * i + k];
    for (const DevPtr *t : {&w, &sid, &ssigma}) {
        GateOpening o;
        o.commitment = commit(be, pg, *t, N);
        Opening op = open(be, pg, *t, N, sc.chal);
        o.value = op.value;
        o.proof = op.proofs;
        p.openings.push_back(o);
    }
    p.v_commitment = commit(be, pg, tree, 2 * N);
    for (const FrVec &pt : v_points(sc.chal)) p.v_openings.push_back(open(be, pg, tree, 2 * N, pt));
    return p;
}

// check 4: w, sid, ssigma at r in one zk_pcs_verify_batch (vk_mu), the tree's five openings in another (vk_mu1)
inline bool verify_openings(Ctx &be, const PcsVk &vk_mu, const PcsVk &vk_mu1, const WiringProof &proof, const FrVec &chal) {
    G1Vec cs;
    FrVec vs;
    std::vector<G1Vec> pfs;
    std::vector<FrVec> pts;
    for (const GateOpening &o : proof.openings) cs.push_back(o.commitment), vs.push_back(o.value), pfs.push_back(o.proof), pts.push_back(chal);
    for (bool ok : verify_batch(be, vk_mu, cs, vs, pfs, pts))
        if (!ok) return false;
    cs.clear(), vs.clear(), pfs.clear();
    pts = v_points(chal);
    for (const Opening &o : proof.v_openings) cs.push_back(proof.v_commitment), vs.push_back(o.value), pfs.push_back(o.proofs);
    for (bool ok : verify_batch(be, vk_mu1, cs, vs, pfs, pts))
        if (!ok) return false;
    return true;
}

inline bool wiring_verify(Ctx &be, const PcsVk &vk_mu, const PcsVk &vk_mu1, const WiringProof &proof, const WiringScalars &sc) {
    return verify_rounds(proof, sc) && verify_openings(be, vk_mu, vk_mu1, proof, sc.chal);
}

}  // namespace zkhost
