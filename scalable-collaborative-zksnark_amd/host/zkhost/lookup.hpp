// The lookup argument (LogUp) as a stand-alone non-interactive proof -- the compiled counterpart of zkhip/lookup.py, function by
// function and bit for bit: every value of a column f lies in a table t, both of N = 2^n Fr.  The caller supplies the row-to-table
// indices idx (u32[N], f[x] = t[idx[x]]); m[y] = #{x : idx[x] = y} (zk_lookup_multiplicities, which checks every row on the way).
//
//     df = beta + f,   dt = beta + t,   hf = 1 / df,   ht = m / dt
//     sum_x  hf(x) - ht(x)  +  E(x) [ hf(x) df(x) - 1  +  gamma ( ht(x) dt(x) - m(x) ) ]  =  0,        E = lambda eq(tau, .)
//
// Schedule (label "lookup"): absorb n; absorb the commitment of t; absorb the commitments of f and m; beta <- challenge; absorb the
//     commitments of hf and ht; gamma, lambda <- challenges; tau <- n challenges; per round absorb its four evaluations, r_i <- challenge;
//     absorb the five claimed values f, t, m, hf, ht at r (the folded-out last values of the sumcheck: f(r) = df(r) - beta,
//     t(r) = dt(r) - beta); b_alpha <- challenge; per round of the n-variate batch instance (five claims, one point) absorb
//     (t0, t1, t2), rho_i <- challenge; the opening at rho.
#pragma once
#include "hyperplonk.hpp"
#include "nizk.hpp"
#include "sha256.hpp"

namespace zkhost {

struct LookupProof {
    size_t n = 0;
    G1Vec commitments;                      // f, m, hf, ht
    std::vector<std::array<Fr, 4>> rounds;  // p(0) .. p(3) per round
    FrVec values;                           // f, t, m, hf, ht at r
    BatchOpenProof batch;
};
struct LookupPk {
    size_t n = 0;
    DevPtr t;
    G1 commitment;
};
struct LookupVk {
    size_t n = 0;
    G1 commitment;
};
struct LookupChallenges {
    Fr beta, gamma, lambda, b_alpha;
    FrVec tau, chal, rho;
};

// hf - ht + E [ hf (beta + f) - 1 + gamma ( ht (beta + t) - m ) ]
inline Fr lookup_value(const Fr &E, const Fr &f, const Fr &t, const Fr &m, const Fr &hf, const Fr &ht, const Fr &beta, const Fr &gamma) {
    return hf - ht + E * (hf * (beta + f) - Fr::one() + gamma * (ht * (beta + t) - m));
}

// t: the table, N = 2^n Fr on the device; pg: the levels of a PolynomialCommitment over n variables
inline std::pair<LookupPk, LookupVk> lookup_preprocess(Ctx &be, const PowersOfG &pg, const DevPtr &t, size_t N) {
    size_t n = 0;
    while ((size_t(1) << n) < N) ++n;
    if (n < 1 || N != size_t(1) << n) throw ZkError(ZK_ERR_INVALID, "lookup_preprocess: the table must hold 2^n elements, n >= 1");
    const G1 c = commit(be, pg, t, N);
    return {LookupPk{n, t, c}, LookupVk{n, c}};
}

namespace detail {
inline LookupProof lookup_prove_with(Ctx &be, const PowersOfG &pg, const LookupPk &pk, const DevPtr &f, const DevPtr &m) {
    const size_t n = pk.n, N = size_t(1) << n;
    LookupProof p;
    p.n = n;
    std::shared_ptr<DeviceTranscript> tr = be.transcript("lookup");
    const uint64_t n64 = n;
    be.absorb(*tr, &n64, 8);
    be.absorb(*tr, pk.commitment.data(), 144);
    p.commitments = {commit(be, pg, f, N), commit(be, pg, m, N)};
    be.absorb(*tr, p.commitments.data(), 144 * 2);
    const Fr beta = be.challenges(*tr, 1)[0];
    DevPtr zero = be.fr_sub(f, f, N);
    DevPtr df = be.fr_axpb(f, zero, Fr::zero(), beta, N), dt = be.fr_axpb(pk.t, zero, Fr::zero(), beta, N);
    DevPtr hf = be.fr_batch_div(be.fr_axpb(zero, zero, Fr::zero(), Fr::one(), N), df, N), ht = be.fr_batch_div(m, dt, N);
    p.commitments.push_back(commit(be, pg, hf, N)), p.commitments.push_back(commit(be, pg, ht, N));
    be.absorb(*tr, p.commitments.data() + 2, 144 * 2);
    const FrVec gl = be.challenges(*tr, 2);
    const FrVec tau = be.challenges(*tr, n);
    be.eq_table_acc(tau, gl[1], zero);  // E = lambda eq(tau, .) on the zeroed table
    FrVec last, chal;
    ScResult sc = be.sumcheck_lookup_fs({zero, df, dt, m, hf, ht}, N, gl[0], *tr, last, chal);
    p.rounds.resize(n);
    for (size_t i = 0; i < n; ++i)
        for (int k = 0; k < 4; ++k) p.rounds[i][k] = sc.sums[4 * i + k];
    p.values = {last[1] - beta, last[2] - beta, last[3], last[4], last[5]};
    be.absorb(*tr, p.values.data(), 32 * 5);
    const Fr b_alpha = be.challenges(*tr, 1)[0];
    std::vector<Claim> claims;
    for (size_t j = 0; j < 5; ++j) claims.push_back(Claim{j, chal, p.values[j]});
    p.batch = detail::batch_prove_ni(be, pg, {f, pk.t, m, hf, ht}, N, claims, b_alpha, *tr);
    return p;
}
}  // namespace detail

// f: N Fr, idx: N u32, both on the device.  A row whose value is not the table entry it names: ZkError(ZK_ERR_INVALID); a zero
// denominator: ZkError(ZK_ERR_DIV_ZERO)
inline LookupProof lookup_prove(Ctx &be, const PowersOfG &pg, const LookupPk &pk, const DevPtr &f, const DevPtr &idx) {
    return detail::lookup_prove_with(be, pg, pk, f, be.lookup_multiplicities(f, pk.t, idx, size_t(1) << pk.n));
}
// the find mode: no idx; a row whose value is no entry of the table: ZkError(ZK_ERR_INVALID).  The record is the one of lookup_prove with the
// indices of the first occurrences
inline LookupProof lookup_prove(Ctx &be, const PowersOfG &pg, const LookupPk &pk, const DevPtr &f, FindIndices) {
    return detail::lookup_prove_with(be, pg, pk, f, be.lookup_find(f, pk.t, size_t(1) << pk.n).second);
}

// the verifier's replay of the schedule; false on a malformed record
inline bool lookup_challenges(const LookupVk &vk, const LookupProof &p, LookupChallenges &c, const std::string &label = "lookup") {
    const size_t n = p.n;
    if (n < 1 || n != vk.n || p.rounds.size() != n || p.batch.rounds.size() != n || p.commitments.size() != 4 || p.values.size() != 5) return false;
    HostTranscript tr(label);
    tr.absorb_u64(n).absorb(vk.commitment.data(), 144);
    c.beta = tr.absorb(p.commitments.data(), 144 * 2).challenge();
    tr.absorb(p.commitments.data() + 2, 144 * 2);
    c.gamma = tr.challenge(), c.lambda = tr.challenge();
    c.tau = tr.challenges(n);
    c.chal = detail::replay_rounds(tr, p.rounds);
    c.b_alpha = tr.absorb(p.values).challenge();
    c.rho = detail::replay_rounds(tr, p.batch.rounds);
    return true;
}

namespace detail {
inline std::vector<Claim> lookup_claims(const LookupChallenges &c, const LookupProof &p) {
    std::vector<Claim> claims;
    for (size_t j = 0; j < 5; ++j) claims.push_back(Claim{j, c.chal, p.values[j]});
    return claims;
}
}  // namespace detail

// The verifier's field arithmetic (no GPU) -> 0 when all checks hold, bit 0 for a malformed record, else bit k of the FIRST check that
// fails (whatever breaks one check also changes every challenge drawn after it):
//   1. p_0(0) + p_0(1) == 0 and p_i(0) + p_i(1) == p_{i-1}(r_{i-1}), by interpolation on the nodes 0 .. 3;
//   2. p_{n-1}(r_{n-1}) == hf - ht + lambda eq(tau, r) [ hf (beta + f) - 1 + gamma ( ht (beta + t) - m ) ] on the claimed values;
//   3. the round chain of the batch instance (batch_open.hpp failed_checks; with finals = the five f_j(rho) also its last value).
inline unsigned lookup_failed_checks(const LookupVk &vk, const LookupProof &p, const FrVec *finals = nullptr, Fr *y = nullptr) {
    LookupChallenges c;
    if (!lookup_challenges(vk, p, c) || p.batch.opening.size() != p.n) return 1u;
    Fr target;
    if (!round_chain(p.rounds, 4, c.chal, Fr::zero(), &target)) return 1u << 1;
    const FrVec &v = p.values;
    if (target != lookup_value(c.lambda * eq_eval(c.tau, c.chal), v[0], v[1], v[2], v[3], v[4], c.beta, c.gamma)) return 1u << 2;
    if (failed_checks(5, detail::lookup_claims(c, p), p.batch, c.b_alpha, c.rho, y, finals)) return 1u << 3;
    return 0;
}
inline bool lookup_field_checks(const LookupVk &vk, const LookupProof &p, const FrVec *finals = nullptr) { return lookup_failed_checks(vk, p, finals) == 0; }

// the replay, checks 1-3, and ONE zk_pcs_verify_batch call: the opening of sum_j e_j C_j at rho
inline bool lookup_verify(Ctx &be, const PcsVk &pcs_vk, const LookupVk &vk, const LookupProof &p) {
    LookupChallenges c;
    Fr y;
    if (lookup_failed_checks(vk, p, nullptr, &y) || !lookup_challenges(vk, p, c)) return false;
    const G1Vec all5 = {p.commitments[0], vk.commitment, p.commitments[1], p.commitments[2], p.commitments[3]};  // f, t, m, hf, ht
    try {
        return verify_opening(be, pcs_vk, all5, detail::lookup_claims(c, p), p.batch, c.b_alpha, c.rho, y);
    } catch (const ZkError &e) {  // a point of the record that is not on the curve is refused by the pairing call: a record to reject
        if (e.status != ZK_ERR_INVALID) throw;
        return false;
    }
}

// zkhip.lookup.proof_digest: the record's words in the order of the schedule
inline std::string proof_digest(const LookupProof &p) {
    Sha256 h;
    const uint64_t n = p.n;
    h.update(&n, 8);
    h.update(p.commitments.data(), 144 * p.commitments.size());
    for (auto &r : p.rounds) h.update(r.data(), 4 * 32);
    h.update(p.values.data(), 32 * p.values.size());
    detail::digest_batch(h, p.batch);
    return h.hex();
}

// ---- the sample both hosts prove (zkhip.lookup.sample_lookup: one seed = one digest) ----
static const uint64_t kLookupSampleSeed = 0x10C00000;  // stream k of seed S is SplitMix64(kLookupSampleSeed + 1000 S + k)

struct LookupSample {
    FrVec t, f;
    std::vector<uint32_t> idx;
};
// a table of `distinct` different entries (stream 10; 0: N / 2, at least 1) padded to N = 2^n by repeating the last one, and a column
// drawn from it: idx[x] = (limb 0 of element x of stream 11) mod distinct, f[x] = t[idx[x]]
inline LookupSample sample_lookup(size_t n, uint64_t seed, size_t distinct = 0) {
    const size_t N = size_t(1) << n;
    if (distinct == 0) distinct = N / 2 ? N / 2 : 1;
    if (distinct > N) throw ZkError(ZK_ERR_INVALID, "sample_lookup: 1 <= distinct <= N is needed");
    const uint64_t base = kLookupSampleSeed + 1000 * seed;
    LookupSample s;
    s.t = SplitMix64(base + 10).fr_vec(distinct);
    s.t.resize(N, s.t[distinct - 1]);
    const FrVec draw = SplitMix64(base + 11).fr_vec(N);
    s.idx.resize(N), s.f.resize(N);
    for (size_t x = 0; x < N; ++x) s.idx[x] = (uint32_t)(draw[x].v[0] % distinct), s.f[x] = s.t[s.idx[x]];
    return s;
}
// the trapdoor of the sample's SRS: n Fr of stream 3
inline FrVec sample_lookup_srs(size_t n, uint64_t seed) { return SplitMix64(kLookupSampleSeed + 1000 * seed + 3).fr_vec(n); }
// SHA-256 over t | f | idx (u32), little-endian
inline std::string sample_digest(const LookupSample &s) {
    Sha256 h;
    h.update(s.t.data(), 32 * s.t.size());
    h.update(s.f.data(), 32 * s.f.size());
    h.update(s.idx.data(), 4 * s.idx.size());
    return h.hex();
}

}  // namespace zkhost
