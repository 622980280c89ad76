// Non-interactive gate ZeroCheck and wiring PermCheck -- the compiled counterpart of zkhip/nizk.py, bit for bit: the batched
// arguments of batch_open.hpp with EVERY challenge derived from a Fiat-Shamir transcript (transcript.hpp), so that no challenge is an
// argument of a prover or a verifier.  The prover keeps the transcript on the device (zk_sumcheck_gate_fs / _wiring_fs / _multi_fs draw
// round i's challenge between their kernels); the verifier replays the schedule with HostTranscript from the record alone and then
// runs the EXISTING checks of batch_open.hpp with the derived challenges.
//
// Gate schedule (label "gate"):     absorb n; absorb the six commitments (kGateOpened order); tau <- n challenges; per round absorb its
//     five evaluations, r_i <- challenge; absorb the six claimed values; alpha <- challenge; per round of the batch instance absorb
//     (t0, t1, t2), rho_i <- challenge; the opening at rho.
// Wiring schedule (label "wiring"): absorb mu; absorb the commitments of w, sid, ssigma; alpha, beta <- challenges; absorb the
//     commitment of the product tree; gamma <- challenge; tau <- mu challenges; per round absorb its four evaluations, r_i <- challenge;
//     absorb the three claimed values; absorb the five claimed tree values; b_alpha <- challenge; the rounds of the mu-variate batch
//     instance give rho_mu, then those of the (mu + 1)-variate one give rho_mu1.
#pragma once
#include "batch_open.hpp"
#include "transcript.hpp"

namespace zkhost {

struct GateProofNi {
    size_t n = 0;
    GateProofBatched rec;
};
struct WiringProofNi {
    size_t mu = 0;
    WiringProofBatched rec;
};
struct GateChallenges {
    FrVec tau, chal, rho;
    Fr alpha;
};
struct WiringChallenges {
    WiringScalars sc;  // alpha, beta, gamma, tau, chal
    Fr b_alpha;
    FrVec rho_mu, rho_mu1;
};

namespace detail {
template <size_t K>
inline FrVec replay_rounds(HostTranscript &tr, const std::vector<std::array<Fr, K>> &rounds) {
    FrVec out;
    for (const auto &r : rounds) out.push_back(tr.absorb(r.data(), 32 * K).challenge());
    return out;
}
// batch_open_prove with rho drawn from the transcript
inline BatchOpenProof batch_prove_ni(Ctx &be, const PowersOfG &pg, const std::vector<DevPtr> &tables, size_t N, const std::vector<Claim> &claims, const Fr &alpha,
                                     DeviceTranscript &tr) {
    size_t n = 0;
    while ((size_t(1) << n) < N) ++n;
    std::vector<DevPtr> eqs = combined_eq_tables(be, tables.size(), n, claims, alpha), es, fs;
    for (size_t j = 0; j < tables.size(); ++j)
        if (eqs[j]) es.push_back(eqs[j]), fs.push_back(tables[j]);
    FrVec last_e, last_f, rho;
    ScResult r = be.sumcheck_multi_fs(es, fs, N, tr, last_e, last_f, rho);
    DevPtr g = be.fr_lincomb(fs, last_e, N);
    BatchOpenProof p;
    p.rounds.resize(n);
    for (size_t i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) p.rounds[i][k] = r.sums[3 * i + k];
    p.opening = open(be, pg, g, N, rho).proofs;
    return p;
}
}  // namespace detail

// ---- gate ----
// the verifier's replay of the gate schedule; false on a malformed record
inline bool gate_challenges(const GateProofNi &p, GateChallenges &c, const std::string &label = "gate") {
    const size_t n = p.n;
    if (n < 1 || p.rec.rounds.size() != n || p.rec.batch.rounds.size() != n || p.rec.commitments.size() != 6 || p.rec.values.size() != 6) return false;
    HostTranscript tr(label);
    tr.absorb_u64(n).absorb(p.rec.commitments.data(), 144 * 6);
    c.tau = tr.challenges(n);
    c.chal = detail::replay_rounds(tr, p.rec.rounds);
    c.alpha = tr.absorb(p.rec.values).challenge();
    c.rho = detail::replay_rounds(tr, p.rec.batch.rounds);
    return true;
}

inline GateProofNi gate_prove_ni(Ctx &be, const PowersOfG &pg, const GateTables &t, size_t n) {
    if (n < 1) throw ZkError(ZK_ERR_INVALID, "gate_prove_ni: n >= 1");
    const size_t len = size_t(1) << n;
    GateProofNi p;
    p.n = n;
    std::vector<DevPtr> tabs;
    for (size_t k = 0; k < 6; ++k) tabs.push_back(t.at(kGateOpened[k])), p.rec.commitments.push_back(commit(be, pg, tabs[k], len));
    std::shared_ptr<DeviceTranscript> tr = be.transcript("gate");
    const uint64_t n64 = n;
    be.absorb(*tr, &n64, 8);
    be.absorb(*tr, p.rec.commitments.data(), 144 * 6);
    const FrVec tau = be.challenges(*tr, n);
    DevPtr eq = be.eq_table(tau);
    FrVec last, chal;
    ScResult sc = be.sumcheck_gate_fs({eq, t.at("q1"), t.at("q2"), t.at("a"), t.at("b"), t.at("c"), t.at("in")}, len, *tr, last, chal);
    p.rec.rounds.resize(n);
    for (size_t i = 0; i < n; ++i)
        for (int k = 0; k < 5; ++k) p.rec.rounds[i][k] = sc.sums[5 * i + k];
    p.rec.values = {last[3], last[4], last[5], last[6], last[1], last[2]};  // a, b, c, in, q1, q2: the folded-out values ARE f(r)
    be.absorb(*tr, p.rec.values.data(), 32 * 6);
    const Fr alpha = be.challenges(*tr, 1)[0];
    std::vector<Claim> claims;
    for (size_t k = 0; k < 6; ++k) claims.push_back(Claim{k, chal, p.rec.values[k]});
    p.rec.batch = detail::batch_prove_ni(be, pg, tabs, len, claims, alpha, *tr);
    return p;
}

inline bool gate_verify_ni(Ctx &be, const PcsVk &vk, const GateProofNi &p) {
    GateChallenges c;
    if (!gate_challenges(p, c)) return false;
    return gate_zerocheck_verify_batched(be, vk, p.rec, c.tau, c.chal, c.alpha, c.rho);
}

// ---- wiring ----
inline bool wiring_challenges(const WiringProofNi &p, WiringChallenges &c, const std::string &label = "wiring") {
    const size_t mu = p.mu;
    const WiringProofBatched &r = p.rec;
    if (mu < 1 || r.rounds.size() != mu || r.batch.rounds.size() != mu || r.v_batch.rounds.size() != mu + 1 || r.commitments.size() != 3 || r.values.size() != 3 ||
        r.v_values.size() != 5)
        return false;
    HostTranscript tr(label);
    tr.absorb_u64(mu).absorb(r.commitments.data(), 144 * 3);
    c.sc.alpha = tr.challenge(), c.sc.beta = tr.challenge();
    c.sc.gamma = tr.absorb(r.v_commitment.data(), 144).challenge();
    c.sc.tau = tr.challenges(mu);
    c.sc.chal = detail::replay_rounds(tr, r.rounds);
    c.b_alpha = tr.absorb(r.values).absorb(r.v_values).challenge();
    c.rho_mu = detail::replay_rounds(tr, r.batch.rounds);
    c.rho_mu1 = detail::replay_rounds(tr, r.v_batch.rounds);
    return true;
}

// pg: the levels of a PolynomialCommitment over mu + 1 variables
inline WiringProofNi wiring_prove_ni(Ctx &be, const PowersOfG &pg, const DevPtr &w, const DevPtr &sid, const DevPtr &ssigma, size_t N) {
    size_t mu = 0;
    while ((size_t(1) << mu) < N) ++mu;
    if (mu < 1 || N != size_t(1) << mu) throw ZkError(ZK_ERR_INVALID, "wiring_prove_ni: N must be 2^mu, mu >= 1");
    WiringProofNi p;
    p.mu = mu;
    WiringProofBatched &r = p.rec;
    const std::vector<DevPtr> tabs = {w, sid, ssigma};
    for (const DevPtr &t : tabs) r.commitments.push_back(commit(be, pg, t, N));
    std::shared_ptr<DeviceTranscript> tr = be.transcript("wiring");
    const uint64_t mu64 = mu;
    be.absorb(*tr, &mu64, 8);
    be.absorb(*tr, r.commitments.data(), 144 * 3);
    const FrVec ab = be.challenges(*tr, 2);
    DevPtr num = be.fr_axpb(w, sid, ab[0], ab[1], N), den = be.fr_axpb(w, ssigma, ab[0], ab[1], N);
    DevPtr h = be.fr_batch_div(num, den, N);
    DevPtr tree = be.product_tree(h, N);
    r.v_commitment = commit(be, pg, tree, 2 * N);
    be.absorb(*tr, r.v_commitment.data(), 144);
    const Fr gamma = be.challenges(*tr, 1)[0];
    const FrVec tau = be.challenges(*tr, mu);
    DevPtr eq = be.eq_table(tau);
    FrVec last, chal;
    ScResult sc = be.sumcheck_wiring_fs(eq, tree, num, den, N, gamma, *tr, last, chal);
    r.rounds.resize(mu);
    for (size_t i = 0; i < mu; ++i)
        for (int k = 0; k < 4; ++k) r.rounds[i][k] = sc.sums[4 * i + k];
    std::vector<std::pair<size_t, FrVec>> pts = {{0, chal}, {1, chal}, {2, chal}}, vpts;
    for (const FrVec &z : v_points(chal)) vpts.push_back({0, z});
    const std::vector<Claim> claims = evaluate_claims(be, tabs, N, pts), v_claims = evaluate_claims(be, {tree}, 2 * N, vpts);
    for (const Claim &c : claims) r.values.push_back(c.value);
    for (const Claim &c : v_claims) r.v_values.push_back(c.value);
    be.absorb(*tr, r.values.data(), 32 * 3);
    be.absorb(*tr, r.v_values.data(), 32 * 5);
    const Fr b_alpha = be.challenges(*tr, 1)[0];
    r.batch = detail::batch_prove_ni(be, pg, tabs, N, claims, b_alpha, *tr);
    r.v_batch = detail::batch_prove_ni(be, pg, {tree}, 2 * N, v_claims, b_alpha, *tr);
    return p;
}

inline bool wiring_verify_ni(Ctx &be, const PcsVk &vk_mu, const PcsVk &vk_mu1, const WiringProofNi &p) {
    WiringChallenges c;
    if (!wiring_challenges(p, c)) return false;
    return wiring_verify_batched(be, vk_mu, vk_mu1, p.rec, c.sc, c.b_alpha, c.rho_mu, c.rho_mu1);
}

// zkhip.nizk.proof_digest: the record's words in the order of the schedule
namespace detail {
inline void digest_batch(Sha256 &h, const BatchOpenProof &b) {
    for (auto &r : b.rounds) h.update(r.data(), 3 * 32);
    h.update(b.opening.data(), 144 * b.opening.size());
}
}  // namespace detail
inline std::string proof_digest(const GateProofNi &p) {
    Sha256 h;
    const uint64_t n = p.n;
    h.update(&n, 8);
    h.update(p.rec.commitments.data(), 144 * p.rec.commitments.size());
    for (auto &r : p.rec.rounds) h.update(r.data(), 5 * 32);
    h.update(p.rec.values.data(), 32 * p.rec.values.size());
    detail::digest_batch(h, p.rec.batch);
    return h.hex();
}
inline std::string proof_digest(const WiringProofNi &p) {
    Sha256 h;
    const uint64_t mu = p.mu;
    h.update(&mu, 8);
    h.update(p.rec.commitments.data(), 144 * p.rec.commitments.size());
    h.update(p.rec.v_commitment.data(), 144);
    for (auto &r : p.rec.rounds) h.update(r.data(), 4 * 32);
    h.update(p.rec.values.data(), 32 * p.rec.values.size());
    h.update(p.rec.v_values.data(), 32 * p.rec.v_values.size());
    detail::digest_batch(h, p.rec.batch);
    detail::digest_batch(h, p.rec.v_batch);
    return h.hex();
}

}  // namespace zkhost
