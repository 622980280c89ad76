// The gate identity as a ZeroCheck a verifier can check end to end -- the compiled counterpart of zkhip/zerocheck.py, bit for bit.
//
// The reference SIMULATES the gate check with six independent product sumchecks on a random `eq` vector
// (hyperplonk/src/hyperplonk.rs:66-93, dhyperplonk.rs:218-260).  Here
//     sum_x eq(tau, x) [ q1(x) (a(x) + b(x)) + q2(x) a(x) b(x) - c(x) + in(x) ] = 0
// is proved by ONE degree-4 sumcheck (zk_eq_table, zk_sumcheck_gate), closed by openings of a, b, c, in, q1, q2 at the sumcheck
// point (the existing commit / open path) and verified with one batched pairing check (zk_pcs_verify_batch).
//
// tau and the challenges are INPUTS, as everywhere in this code base (dhyperplonk.rs:103-109 pre-samples every challenge):
// Fiat-Shamir is out of scope.  Single party only.
#pragma once
#include <array>
#include <chrono>
#include <map>
#include <string>
#include <vector>

#include "dist_primitive.hpp"
#include "round_chain.hpp"

namespace zkhost {

// order of the six openings in a proof record
static const char *const kGateOpened[6] = {"a", "b", "c", "in", "q1", "q2"};

struct GateOpening {
    G1 commitment;
    Fr value;
    G1Vec proof;
};
struct GateProof {
    std::vector<std::array<Fr, 5>> rounds;  // the round polynomial at t = 0 .. 4
    std::vector<GateOpening> openings;      // in the order of kGateOpened
};
using GateTables = std::map<std::string, DevPtr>;  // "q1", "q2", "a", "b", "c", "in": 2^n Fr each

// eq(tau, r) = prod_i (tau_i r_i + (1 - tau_i)(1 - r_i))
inline Fr eq_eval(const FrVec &tau, const FrVec &r) {
    Fr v = Fr::one();
    for (size_t i = 0; i < tau.size(); ++i) v *= tau[i] * r[i] + (Fr::one() - tau[i]) * (Fr::one() - r[i]);
    return v;
}

// the wide Plonk gate (zk_sumcheck_gate_wide) at one point: eq [ qL a + qR b + qM a b + qH a^5 - qO c + qC + in ]
inline Fr wide_gate_value(const Fr &eq, const Fr &qL, const Fr &qR, const Fr &qM, const Fr &qO, const Fr &qC, const Fr &qH, const Fr &a, const Fr &b, const Fr &c,
                          const Fr &in) {
    const Fr a2 = a * a;
    return eq * (qL * a + qR * b + qM * a * b + qH * a2 * a2 * a - qO * c + qC + in);
}

// The verifier's field arithmetic (no GPU): the round chain from 0 on the nodes 0 .. 4 (round_chain.hpp), and
// p_{n-1}(r_{n-1}) == eq(tau, r) [q1 (a + b) + q2 a b - c + in] on the six opened values.
inline bool verify_rounds(const GateProof &proof, const FrVec &tau, const FrVec &chal) {
    const size_t n = proof.rounds.size();
    if (n == 0 || tau.size() != n || chal.size() != n || proof.openings.size() != 6) return false;
    Fr target;
    if (!round_chain(proof.rounds, 5, chal, Fr::zero(), &target)) return false;
    const Fr &a = proof.openings[0].value, &b = proof.openings[1].value, &c = proof.openings[2].value, &in = proof.openings[3].value,
             &q1 = proof.openings[4].value, &q2 = proof.openings[5].value;
    return target == eq_eval(tau, chal) * (q1 * (a + b) + q2 * a * b - c + in);
}

// eq table, gate sumcheck, commitments (unless given) and openings at r = chal.  seconds (optional): [eq table, sumcheck]
inline GateProof gate_zerocheck_prove(Ctx &be, const PowersOfG &pg, const GateTables &t, const FrVec &tau, const FrVec &chal,
                                      const std::map<std::string, G1> *commitments = nullptr, double *seconds = nullptr) {
    const size_t n = tau.size(), len = size_t(1) << n;
    if (n < 1 || chal.size() != n) throw ZkError(ZK_ERR_INVALID, "gate_zerocheck_prove: tau and chal must hold one element per variable");
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t0 = now();
    DevPtr eq = be.eq_table(tau);
    be.sync();
    const double t1 = now();
    FrVec last;
    ScResult sc = be.sumcheck_gate({eq, t.at("q1"), t.at("q2"), t.at("a"), t.at("b"), t.at("c"), t.at("in")}, len, chal, last);
    const double t2 = now();
    if (seconds) seconds[0] = t1 - t0, seconds[1] = t2 - t1;
    GateProof p;
    p.rounds.resize(n);
    for (size_t i = 0; i < n; ++i)
        for (int k = 0; k < 5; ++k) p.rounds[i][k] = sc.sums[5 * i + k];
    for (const char *name : kGateOpened) {
        GateOpening o;
        const bool have = commitments && commitments->count(name);
        o.commitment = have ? commitments->at(name) : commit(be, pg, t.at(name), len);
        p.openings.push_back(o);
    }
    for (size_t k = 0; k < 6; ++k) {
        Opening op = open(be, pg, t.at(kGateOpened[k]), len, chal);
        p.openings[k].value = op.value;
        p.openings[k].proof = op.proofs;
    }
    return p;
}

// verify_rounds, then the six openings in ONE zk_pcs_verify_batch call
inline bool gate_zerocheck_verify(Ctx &be, const PcsVk &vk, const GateProof &proof, const FrVec &tau, const FrVec &chal) {
    if (!verify_rounds(proof, tau, chal)) return false;
    G1Vec cs;
    FrVec vs;
    std::vector<G1Vec> pfs;
    std::vector<FrVec> pts;
    for (const GateOpening &o : proof.openings) cs.push_back(o.commitment), vs.push_back(o.value), pfs.push_back(o.proof), pts.push_back(chal);
    for (bool ok : verify_batch(be, vk, cs, vs, pfs, pts))
        if (!ok) return false;
    return true;
}

}  // namespace zkhost
