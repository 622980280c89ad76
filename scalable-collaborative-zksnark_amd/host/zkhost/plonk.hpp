// HyperPlonk for ONE circuit -- the compiled counterpart of zkhip/plonk.py, bit for bit: the gate ZeroCheck and the wiring PermCheck
// over the three wire columns on the SAME committed wires, under one Fiat-Shamir transcript, closed by two opening proofs.
//
// N = 2^mu rows with selectors q1, q2 and wires a, b, c (columns 0, 1, 2; slot j N + x = wire j of row x), a permutation sigma of the 3N
// slots, ssigma_j(x) = sigma(j N + x), l = 2^k <= N / 2 public inputs in rows 0 .. l - 1 of `in`.
//     n_j = w_j + alpha (j N + x) + beta,  d_j = w_j + alpha ssigma_j + beta,  h = n_0 n_1 n_2 / (d_0 d_1 d_2),  v = product_tree(h)
//
// Schedule (label "plonk"):
//   1. absorb mu, l (one u64 each), the five vk commitments (q1, q2, ssigma_0..2), the l public inputs;
//   2. absorb the commitments of a, b, c;  alpha, beta <- challenges;
//   3. the derived tables and the tree; absorb the tree's commitment;  gamma <- challenge;
//   4. tau_p <- mu challenges; zk_sumcheck_perm3_fs: per round absorb its six evaluations, r_p[i] <- challenge;
//   5. tau_g <- mu challenges; zk_sumcheck_gate_fs on (eq, q1, q2, a, b, c, in): per round absorb its five evaluations, r_g[i] <- challenge;
//   6. absorb q1, q2, a, b, c at r_g; a, b, c, ssigma_0..2 at r_p; the tree at the five v_points of r_p;  b_alpha <- challenge;
//   7. the mu-variate batch instance (eleven claims on q1, q2, a, b, c, ssigma_0..2), then the (mu + 1)-variate one (five claims on the
//      tree): per round absorb (t0, t1, t2), rho[i] <- challenge.  Two opening proofs.
// The SRS has mu + 1 variables; the mu-variate tables use the last mu of them.  Single party only.
//
// A SECOND arithmetisation beside this one (GateKind::wide): the selectors qL, qR, qM, qO, qC, qH in the place of q1, q2 and the gate
//     qL a + qR b + qM a b + qH a^5 - qO c + qC + in = 0
// under the label "plonk-wide": nine vk commitments, zk_sumcheck_gate_wide_fs with EIGHT evaluations per round, nine values at r_g, a
// mu-variate batch instance of twelve tables and fifteen claims.  The schedule, the permutation half and the (mu + 1)-variate instance are
// the same code: a gate kind is described by gate_desc (label, selector count, evaluations per round), gate_sumcheck_fs (the device
// sumcheck) and gate_closed_form (the verifier's closed form).  GateKind::basic behaves exactly as before.
//
// LOOKUPS (zkhip/plonk.py, module text): a circuit may carry a selector qk (0 or 1) and a table of N triples (t0, t1, t2); row x with
// qk(x) = 1 claims (a, b, c)(x) = (t0, t1, t2)(idx[x]).  With f = a + zeta b + zeta^2 c, t = t0 + zeta t1 + zeta^2 t2, df = beta_l + f,
// dt = beta_l + t, hf = qk / df, ht = m / dt one degree-3 sumcheck over E, df, dt, m, hf, ht, qk (zk_sumcheck_lookup_sel_fs) proves
//     sum_x hf - ht + E [ hf df - qk + gamma_l ( ht dt - m ) ] = 0,      E = lambda eq(tau_l, .)
// The label is the gate's + "-lookup"; the vk commitments are the gate's followed by qk, t0, t1, t2.  Insertions into the schedule:
//   2L. after alpha, beta: m; absorb its commitment;  zeta, beta_l <- challenges;
//   3L. after gamma: df, dt, hf, ht; absorb the commitments of hf, ht;  gamma_l, lambda <- challenges;
//   5L. after the gate sumcheck: tau_l <- mu challenges; the lookup sumcheck: per round absorb four evaluations, r_l[i] <- challenge;
//   6.  after v_values absorb l_values = a, b, c, qk, t0, t1, t2, m, hf, ht at r_l;
//   7.  the mu-variate instance gains three claims (a, b, c at r_l); after the (mu + 1)-variate instance a THIRD one: qk, t0, t1, t2, m,
//       hf, ht with seven claims at r_l.  Three opening proofs.
// A circuit, key or record without a lookup behaves exactly as before.
#pragma once
#include <chrono>

#include "nizk.hpp"

namespace zkhost {

enum class GateKind { basic, wide };
struct GateDesc {
    const char *label;
    size_t selectors;  // basic: q1, q2;  wide: qL, qR, qM, qO, qC, qH
    size_t evals;      // evaluations per round of the gate sumcheck
};
inline const GateDesc &gate_desc(GateKind k) {
    static const GateDesc d[2] = {{"plonk", 2, 5}, {"plonk-wide", 6, 8}};
    return d[k == GateKind::wide ? 1 : 0];
}

struct PlonkCircuit {
    GateKind gate = GateKind::basic;
    size_t mu = 0, l = 0;
    std::vector<FrVec> sel;             // the selectors in the order of gate_desc
    FrVec a, b, c, public_inputs, s;    // s: the SRS trapdoor, mu + 1 elements
    std::vector<uint64_t> sigma;        // 3N slot numbers
    bool lookup = false;
    FrVec qk, t0, t1, t2;               // with a lookup: the selector and the table, N elements each
    std::vector<uint32_t> idx;          // with a lookup: the prover's row-to-table indices
    std::vector<uint32_t> advice;       // the advice codes, N of them (empty: none): prover-side only, read by witness_plan alone
    FrVec free;                         // sample_circuit_lookup_fn only: the free values at their slots (3N elements, 0 elsewhere); not in the digest
};
struct PlonkVk {
    GateKind gate = GateKind::basic;
    size_t mu = 0, l = 0;
    G1Vec commitments;  // the selectors, ssigma_0, ssigma_1, ssigma_2; with a lookup then qk, t0, t1, t2
    bool lookup = false;
    std::vector<G2Rec> g2;  // the mu + 2 raw keys [g2, s_0 g2, .., s_mu g2] when the caller has set them (pcs_vk.hpp powers_of_g2); read by vk_io.hpp only
};
struct PlonkPk {
    GateKind gate = GateKind::basic;
    size_t mu = 0, l = 0;
    std::vector<DevPtr> sel;
    std::array<DevPtr, 3> ssigma;
    G1Vec commitments;
    bool lookup = false;
    DevPtr qk;
    std::array<DevPtr, 3> table;  // t0, t1, t2
};
struct PlonkProof {
    GateKind gate = GateKind::basic;
    size_t mu = 0, l = 0;
    G1Vec commitments;  // a, b, c
    G1 v_commitment;
    std::vector<std::array<Fr, 6>> p_rounds;
    std::vector<FrVec> g_rounds;         // gate_desc(gate).evals per round
    FrVec g_values, p_values, v_values;  // selectors + 3, 6, 5
    BatchOpenProof batch, v_batch;
    bool lookup = false;
    G1Vec l_commitments;                     // m, hf, ht
    std::vector<std::array<Fr, 4>> l_rounds;
    FrVec l_values;                          // a, b, c, qk, t0, t1, t2, m, hf, ht at r_l
    BatchOpenProof l_batch;
};
inline std::string plonk_label(GateKind k, bool lookup) { return std::string(gate_desc(k).label) + (lookup ? "-lookup" : ""); }
// hf - ht + E [ hf (beta + a + zeta b + zeta^2 c) - qk + gamma ( ht (beta + t0 + zeta t1 + zeta^2 t2) - m ) ];  v: the ten l_values
inline Fr lookup3_value(const Fr &E, const FrVec &v, const Fr &zeta, const Fr &beta, const Fr &gamma) {
    const Fr df = beta + v[0] + zeta * v[1] + zeta * zeta * v[2], dt = beta + v[4] + zeta * v[5] + zeta * zeta * v[6];
    return v[8] - v[9] + E * (v[8] * df - v[3] + gamma * (v[9] * dt - v[7]));
}

// the device sumcheck of a gate kind; tabs: eq, the selectors, a, b, c, in
inline ScResult gate_sumcheck_fs(Ctx &be, GateKind k, const std::vector<DevPtr> &tabs, size_t N, DeviceTranscript &tr, FrVec &last, FrVec &chal) {
    if (tabs.size() != gate_desc(k).selectors + 5) throw ZkError(ZK_ERR_INVALID, "gate_sumcheck_fs: eq, the selectors, a, b, c, in are needed");
    if (k == GateKind::wide) {
        std::array<DevPtr, 11> t;
        for (size_t i = 0; i < 11; ++i) t[i] = tabs[i];
        return be.sumcheck_gate_wide_fs(t, N, tr, last, chal);
    }
    std::array<DevPtr, 7> t;
    for (size_t i = 0; i < 7; ++i) t[i] = tabs[i];
    return be.sumcheck_gate_fs(t, N, tr, last, chal);
}
// the verifier's closed form of a gate kind; g: the selectors, a, b, c at r_g
inline Fr gate_closed_form(GateKind k, const Fr &eq, const FrVec &g, const Fr &in) {
    if (k == GateKind::wide) return wide_gate_value(eq, g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], g[8], in);
    return eq * (g[0] * (g[2] + g[3]) + g[1] * g[2] * g[3] - g[4] + in);
}

// ---- witness (zkhip.plonk.witness_plan / witness / check_witness; the rules: include/zkhip.h) ----
// the plan of a circuit: built once, on the host inside the library; the wide gate's output selector qO is sel[3].  lookup: the plan of
// the circuit WITH its lookup (required then; the key table of (t0, t1) is built on the device) -- plonk_witness / plonk_check_witness
// dispatch on the plan.  The default ignores a lookup the circuit may carry.  advice: -1 uses the circuit's advice codes when it has
// them (Ctx::witness_plan_advice), 0 ignores them, 1 requires them
inline std::shared_ptr<WitnessPlan> witness_plan(Ctx &be, const PlonkCircuit &c, bool lookup = false, int advice = -1) {
    const size_t N = size_t(1) << c.mu;
    DevPtr qo;
    if (c.gate == GateKind::wide) qo = be.to_device(c.sel[3]);
    const DevPtr *out_sel = c.gate == GateKind::wide ? &qo : nullptr;
    if (advice > 0 && c.advice.empty()) throw ZkError(ZK_ERR_INVALID, "witness_plan: an advice plan needs a circuit with advice codes");
    const bool adv = advice != 0 && !c.advice.empty();
    if (!lookup) return adv ? be.witness_plan_advice(c.sigma, N, out_sel, c.advice) : be.witness_plan(c.sigma, N, out_sel);
    if (!c.lookup) throw ZkError(ZK_ERR_INVALID, "witness_plan: a lookup plan needs a circuit with a lookup");
    if (adv) {
        const DevPtr qk = be.to_device(c.qk);
        const std::array<DevPtr, 3> t = {be.to_device(c.t0), be.to_device(c.t1), be.to_device(c.t2)};
        return be.witness_plan_advice(c.sigma, N, out_sel, c.advice, &qk, &t);
    }
    return be.witness_plan_lookup(c.sigma, N, out_sel, be.to_device(c.qk), {be.to_device(c.t0), be.to_device(c.t1), be.to_device(c.t2)});
}
inline void witness_need(bool ok, const char *what) {
    if (!ok) throw ZkError(ZK_ERR_INVALID, what);
}
inline void witness_args(const PlonkPk &pk, const WitnessPlan &plan, const FrVec &public_inputs) {
    witness_need(public_inputs.size() == pk.l, "plonk witness: the public-input count differs from the key's");
    witness_need(plan.N == size_t(1) << pk.mu && plan.wide == (pk.gate == GateKind::wide), "plonk witness: the plan is not one of this key's circuit");
    witness_need(!plan.lookup || pk.lookup, "plonk witness: a lookup plan needs a key with the lookup's tables");
}
// the wires of pk's circuit from its public inputs and the values of its free classes (free: 3N elements read at the smallest slot of every
// free class, or null: zeros) -> a, b, c on the device, which go straight into plonk_prove.  A broken gate or copy: ZkError(ZK_ERR_INVALID)
inline std::array<DevPtr, 3> plonk_witness(Ctx &be, const PlonkPk &pk, const WitnessPlan &plan, const FrVec &public_inputs, const FrVec *free = nullptr) {
    witness_args(pk, plan, public_inputs);
    DevPtr f;
    if (free) {
        witness_need(free->size() == 3 * plan.N, "plonk witness: free must hold 3N elements");
        f = be.to_device(*free);
    }
    if (plan.lookup) return be.plonk_witness_lookup(plan, pk.sel, pk.qk, pk.table, public_inputs, free ? &f : nullptr);
    return be.plonk_witness(plan, pk.sel, public_inputs, free ? &f : nullptr);
}
inline WitnessReport plonk_check_witness(Ctx &be, const PlonkPk &pk, const WitnessPlan &plan, const DevPtr &a, const DevPtr &b, const DevPtr &c, const FrVec &public_inputs) {
    witness_args(pk, plan, public_inputs);
    if (plan.lookup) return be.plonk_witness_check_lookup(plan, pk.sel, pk.qk, pk.table, public_inputs, a, b, c);
    return be.plonk_witness_check(plan, pk.sel, public_inputs, a, b, c);
}

namespace detail {
// sigma: one cycle per value -- the c slot of row y, then the a / b slots that copy it in ascending slot order
// fixed (optional, N flags): rows whose a and b slots copy nothing and stay fixed points (the lookup rows)
inline std::vector<uint64_t> copy_sigma(const std::vector<size_t> &ia, const std::vector<size_t> &ib, size_t l, size_t N, const std::vector<char> *fixed = nullptr) {
    std::vector<std::vector<uint64_t>> users(N);
    for (size_t x = l; x < N; ++x)
        if (!fixed || !(*fixed)[x]) users[ia[x]].push_back(x);
    for (size_t x = l; x < N; ++x)
        if (!fixed || !(*fixed)[x]) users[ib[x]].push_back(N + x);
    std::vector<uint64_t> sigma(3 * N);
    for (size_t i = 0; i < 3 * N; ++i) sigma[i] = i;
    for (size_t y = 0; y < N; ++y) {
        uint64_t prev = 2 * N + y;
        for (uint64_t u : users[y]) sigma[prev] = u, prev = u;
        sigma[prev] = 2 * N + y;
    }
    return sigma;
}
// seconds the last sample_circuit / sample_circuit_wide call spent in its ROW LOOP -- the loop over the rows l .. N - 1 that copies a and
// b and computes c (the wide one also places the row's selectors), without the SplitMix64 draws, the allocations, sigma and the
// trapdoor: the CPU baseline of tools/witness_time.py
inline double &sample_loop_seconds() {
    static double s = 0;
    return s;
}
}  // namespace detail
// the lookup rows that sample_circuit_lookup hands to the two generators: row x with mask[x] takes a = u[y[x]], b = v[y[x]] in the place
// of copies and a product gate (c = a b); row brk (-1: none) gets a + 1 before its c is computed
// (u, v are Fr here for both gate kinds; Python's _lookup_rows carries them as integers in the domain its generator builds rows in)
struct LookupRows {
    std::vector<char> mask;
    std::vector<size_t> y;
    FrVec u, v;
    long long brk = -1;
};
struct PlonkChallenges {
    Fr alpha, beta, gamma, b_alpha;
    FrVec tau_p, r_p, tau_g, r_g, rho_mu, rho_mu1;
    Fr zeta, beta_l, gamma_l, lambda;  // with a lookup
    FrVec tau_l, r_l, rho_l;
};

// The test circuit of zkhip.plonk.sample_circuit (the same SplitMix64 streams: 1 public inputs, 2 q1, 3 q2, 4 picks, 5 trapdoor).
// break_gate K adds 1 to c[K] after the fact; break_wire K (K >= l) adds 1 to a[K] and recomputes c[K].  -1: none.
inline PlonkCircuit sample_circuit(size_t mu, uint64_t seed, long long break_gate = -1, long long break_wire = -1, const LookupRows *lk = nullptr) {
    if (mu < 2) throw ZkError(ZK_ERR_INVALID, "sample_circuit: mu >= 2");
    PlonkCircuit c;
    const size_t N = size_t(1) << mu, l = N / 2 < 4 ? N / 2 : 4;
    const uint64_t base = 0x91A70000ull + 1000 * seed;
    c.mu = mu, c.l = l;
    c.public_inputs = SplitMix64(base + 1).fr_vec(l);
    c.sel = {SplitMix64(base + 2).fr_vec(N), SplitMix64(base + 3).fr_vec(N)};
    FrVec &q1 = c.sel[0], &q2 = c.sel[1];
    const FrVec pick = SplitMix64(base + 4).fr_vec(N);
    c.a.assign(N, Fr::zero()), c.b.assign(N, Fr::zero()), c.c.assign(N, Fr::zero());
    for (size_t x = 0; x < l; ++x) q1[x] = Fr::zero(), q2[x] = Fr::zero(), c.c[x] = c.public_inputs[x];
    for (size_t x = l; lk && x < N; ++x)  // a lookup row is a product row: q1 = 0, q2 = 1
        if (lk->mask[x]) q1[x] = Fr::zero(), q2[x] = Fr::one();
    std::vector<size_t> ia(N, 0), ib(N, 0);
    auto gate = [&](size_t x) { return q1[x] * (c.a[x] + c.b[x]) + q2[x] * c.a[x] * c.b[x]; };
    const auto loop_start = std::chrono::steady_clock::now();
    for (size_t x = l; x < N; ++x) {
        ia[x] = pick[x].v[0] % x, ib[x] = pick[x].v[1] % x;
        if (lk && lk->mask[x]) {
            c.a[x] = lk->u[lk->y[x]], c.b[x] = lk->v[lk->y[x]];
            if ((long long)x == lk->brk) c.a[x] += Fr::one();
        } else {
            c.a[x] = c.c[ia[x]], c.b[x] = c.c[ib[x]];
        }
        c.c[x] = gate(x);
    }
    detail::sample_loop_seconds() = std::chrono::duration<double>(std::chrono::steady_clock::now() - loop_start).count();
    if (break_wire >= 0) {
        if ((size_t)break_wire < l || (size_t)break_wire >= N) throw ZkError(ZK_ERR_INVALID, "sample_circuit: break_wire must name a row past the input rows");
        c.a[break_wire] += Fr::one();
        c.c[break_wire] = gate(break_wire);
    }
    if (break_gate >= 0) c.c[break_gate] += Fr::one();
    c.sigma = detail::copy_sigma(ia, ib, l, N, lk ? &lk->mask : nullptr);
    c.s = SplitMix64(base + 5).fr_vec(mu + 1);
    return c;
}

// The test circuit of zkhip.plonk.sample_circuit_wide, bit for bit: streams 1 public inputs, 4 picks, 5 trapdoor as above and 6 .. 11 =
// qL, qR, qM, qO, qC, qH.  Input rows: qO = 1, every other selector 0, c = the public input.  Row x >= l copies a, b from earlier c
// values; its kind is limb 2 of pick x mod 4: 0 linear (qL, qR, qC drawn, qO = 1), 1 product (qM, qC drawn, qO = 1), 2 S-box (qH = 1, qC
// drawn, qO = 1), 3 full (all six drawn; a zero qO is replaced by 1); a selector the kind does not name is 0 and
// c = (qL a + qR b + qM a b + qH a^5 + qC) / qO.  break_gate / break_wire as in sample_circuit.
inline PlonkCircuit sample_circuit_wide(size_t mu, uint64_t seed, long long break_gate = -1, long long break_wire = -1, const LookupRows *lk = nullptr) {
    if (mu < 2) throw ZkError(ZK_ERR_INVALID, "sample_circuit_wide: mu >= 2");
    PlonkCircuit c;
    const size_t N = size_t(1) << mu, l = N / 2 < 4 ? N / 2 : 4;
    const uint64_t base = 0x91A70000ull + 1000 * seed;
    enum { qL, qR, qM, qO, qC, qH };
    c.gate = GateKind::wide, c.mu = mu, c.l = l;
    c.public_inputs = SplitMix64(base + 1).fr_vec(l);
    const FrVec pick = SplitMix64(base + 4).fr_vec(N);
    std::vector<FrVec> drawn;
    for (uint64_t k = 0; k < 6; ++k) drawn.push_back(SplitMix64(base + 6 + k).fr_vec(N));
    c.sel.assign(6, FrVec(N, Fr::zero()));
    c.sel[qO].assign(N, Fr::one());
    c.a.assign(N, Fr::zero()), c.b.assign(N, Fr::zero()), c.c.assign(N, Fr::zero());
    for (size_t x = 0; x < l; ++x) c.c[x] = c.public_inputs[x];
    static const std::vector<std::vector<int>> named = {{qL, qR, qC}, {qM, qC}, {qC}, {qL, qR, qM, qO, qC, qH}};
    std::vector<size_t> ia(N, 0), ib(N, 0);
    auto out = [&](size_t x) {  // the c that satisfies row x
        const Fr &a = c.a[x], a2 = a * a;
        const Fr s = c.sel[qL][x] * a + c.sel[qR][x] * c.b[x] + c.sel[qM][x] * a * c.b[x] + c.sel[qH][x] * a2 * a2 * a + c.sel[qC][x];
        return c.sel[qO][x] == Fr::one() ? s : s * c.sel[qO][x].inverse();
    };
    const auto loop_start = std::chrono::steady_clock::now();
    for (size_t x = l; x < N; ++x) {
        const unsigned kind = pick[x].v[2] % 4;
        for (int k : named[kind]) c.sel[k][x] = drawn[k][x];
        if (kind == 2) c.sel[qH][x] = Fr::one();
        if (kind == 3 && c.sel[qO][x].is_zero()) c.sel[qO][x] = Fr::one();
        ia[x] = pick[x].v[0] % x, ib[x] = pick[x].v[1] % x;
        if (lk && lk->mask[x]) {  // a lookup row is a pure product row: qM = qO = 1, every other selector 0
            for (int k = 0; k < 6; ++k) c.sel[k][x] = (k == qM || k == qO) ? Fr::one() : Fr::zero();
            c.a[x] = lk->u[lk->y[x]], c.b[x] = lk->v[lk->y[x]];
            if ((long long)x == lk->brk) c.a[x] += Fr::one();
        } else {
            c.a[x] = c.c[ia[x]], c.b[x] = c.c[ib[x]];
        }
        c.c[x] = out(x);
    }
    detail::sample_loop_seconds() = std::chrono::duration<double>(std::chrono::steady_clock::now() - loop_start).count();
    if (break_wire >= 0) {
        if ((size_t)break_wire < l || (size_t)break_wire >= N) throw ZkError(ZK_ERR_INVALID, "sample_circuit_wide: break_wire must name a row past the input rows");
        c.a[break_wire] += Fr::one();
        c.c[break_wire] = out(break_wire);
    }
    if (break_gate >= 0) c.c[break_gate] += Fr::one();
    c.sigma = detail::copy_sigma(ia, ib, l, N, lk ? &lk->mask : nullptr);
    c.s = SplitMix64(base + 5).fr_vec(mu + 1);
    return c;
}

// The test circuit of zkhip.plonk.sample_circuit_lookup, bit for bit: sample_circuit (wide: sample_circuit_wide) plus lookup rows against
// a fixed multiplication table.  mu >= 3; streams 12 = u, 13 = v (D = N / 4 elements each); entry y < D is (u_y, v_y, u_y v_y), padded to
// N by repeating entry D - 1.  Row x >= l whose pick (stream 4) has an odd limb 3 is a lookup row: y = (limb 3 >> 1) mod D, a = u_y,
// b = v_y, c = a b, qk = 1, idx = y; its a and b slots are fixed points of sigma.  Every other row: qk = 0, idx = 0.  break_lookup K (a
// lookup row): a[K] + 1 and c[K] recomputed -- gate and wiring still hold and the triple is outside the table.
inline PlonkCircuit sample_circuit_lookup(size_t mu, uint64_t seed, bool wide = false, long long break_lookup = -1) {
    if (mu < 3) throw ZkError(ZK_ERR_INVALID, "sample_circuit_lookup: mu >= 3");
    const size_t N = size_t(1) << mu, l = 4, D = N / 4;
    const uint64_t base = 0x91A70000ull + 1000 * seed;
    const FrVec pick = SplitMix64(base + 4).fr_vec(N);
    LookupRows lk;
    lk.mask.assign(N, 0), lk.y.assign(N, 0), lk.brk = break_lookup;
    for (size_t x = 0; x < N; ++x) lk.mask[x] = x >= l && (pick[x].v[3] & 1), lk.y[x] = (pick[x].v[3] >> 1) % D;
    if (break_lookup >= 0 && !((size_t)break_lookup < N && lk.mask[break_lookup])) throw ZkError(ZK_ERR_INVALID, "sample_circuit_lookup: break_lookup must name a lookup row");
    lk.u = SplitMix64(base + 12).fr_vec(D), lk.v = SplitMix64(base + 13).fr_vec(D);
    PlonkCircuit c = (wide ? sample_circuit_wide : sample_circuit)(mu, seed, -1, -1, &lk);
    c.lookup = true;
    c.t0 = lk.u, c.t1 = lk.v, c.t2.resize(D);
    for (size_t y = 0; y < D; ++y) c.t2[y] = lk.u[y] * lk.v[y];
    for (FrVec *t : {&c.t0, &c.t1, &c.t2}) t->resize(N, (*t)[D - 1]);
    c.qk.assign(N, Fr::zero()), c.idx.assign(N, 0);
    for (size_t x = 0; x < N; ++x)
        if (lk.mask[x]) c.qk[x] = Fr::one(), c.idx[x] = (uint32_t)lk.y[x];
    return c;
}
// The test circuit of zkhip.plonk.sample_circuit_lookup_fn, bit for bit: the wide gate, lookup rows with the gate switched off against the
// XOR table on k = min(4, mu / 2) bits (entry y < 4^k is (y >> k, y & (2^k - 1), their XOR), padded to N by repeating the last entry).
// Streams 1 public inputs, 5 trapdoor, 14 picks.  Row x >= l by limb 2 of pick x mod 8: 0 .. 5 a LOOKUP row (every gate selector 0, qk = 1,
// c = a XOR b; a copies the c of the (limb 0 mod E)-th of the E earlier lookup rows when bits 3 .. 5 of limb 2 are 0 and E > 0, and is
// otherwise free -- a fixed point of sigma holding limb 3 & (2^k - 1); b likewise with bits 6 .. 8, limb 1, (limb 3 >> 8) & (2^k - 1)),
// 6 linear (qL = qR = qO = 1, c = a + b), 7 product (qM = qO = 1, c = a b), both on a = c[limb 0 mod x], b = c[limb 1 mod x].
// break_row K (a lookup row with a free a): that free value + 2^k, so the pair is in no entry; c[K] = 0 as the generator leaves it, idx[K] = 0.
inline PlonkCircuit sample_circuit_lookup_fn(size_t mu, uint64_t seed, long long break_row = -1) {
    if (mu < 3) throw ZkError(ZK_ERR_INVALID, "sample_circuit_lookup_fn: mu >= 3");
    PlonkCircuit c;
    const size_t N = size_t(1) << mu, l = 4, k = mu / 2 < 4 ? mu / 2 : 4, D = size_t(1) << (2 * k);
    const uint64_t base = 0x91A70000ull + 1000 * seed, low = (uint64_t(1) << k) - 1;
    enum { qL, qR, qM, qO, qC, qH };
    c.gate = GateKind::wide, c.mu = mu, c.l = l, c.lookup = true;
    c.public_inputs = SplitMix64(base + 1).fr_vec(l);
    const FrVec pick = SplitMix64(base + 14).fr_vec(N);
    c.sel.assign(6, FrVec(N, Fr::zero()));
    for (FrVec *t : {&c.a, &c.b, &c.c, &c.qk}) t->assign(N, Fr::zero());
    c.free.assign(3 * N, Fr::zero()), c.idx.assign(N, 0);
    std::vector<std::vector<uint64_t>> users(N);  // row y -> the slots that copy c[y]
    std::vector<size_t> lookups;                  // the lookup rows so far
    std::vector<uint64_t> small(N, 0);            // the c of a lookup row as an integer
    for (size_t x = 0; x < l; ++x) c.sel[qO][x] = Fr::one(), c.c[x] = c.public_inputs[x];
    bool broke = false;
    for (size_t x = l; x < N; ++x) {
        const uint64_t *p = pick[x].v;
        const unsigned kind = p[2] % 8;
        if (kind < 6) {
            c.qk[x] = Fr::one();
            uint64_t w[2];
            for (size_t j = 0; j < 2; ++j) {
                const uint64_t bits = (p[2] >> (3 + 3 * j)) & 7;
                if (bits == 0 && !lookups.empty()) {
                    const size_t y = lookups[p[j] % lookups.size()];
                    w[j] = small[y];
                    users[y].push_back(j * N + x);
                } else {
                    w[j] = (j == 0 ? p[3] : p[3] >> 8) & low;
                    if (j == 0 && (long long)x == break_row) w[j] += uint64_t(1) << k, broke = true;
                    c.free[j * N + x] = Fr::from_u64(w[j]);
                }
            }
            const bool hit = w[0] <= low && w[1] <= low;
            small[x] = hit ? w[0] ^ w[1] : 0;
            c.a[x] = Fr::from_u64(w[0]), c.b[x] = Fr::from_u64(w[1]), c.c[x] = Fr::from_u64(small[x]);
            c.idx[x] = hit ? (uint32_t)((w[0] << k) | w[1]) : 0;
            lookups.push_back(x);
        } else {
            const size_t ya = p[0] % x, yb = p[1] % x;
            c.a[x] = c.c[ya], c.b[x] = c.c[yb];
            users[ya].push_back(x), users[yb].push_back(N + x);
            c.sel[qO][x] = Fr::one();
            if (kind == 6) c.sel[qL][x] = c.sel[qR][x] = Fr::one(), c.c[x] = c.a[x] + c.b[x];
            else c.sel[qM][x] = Fr::one(), c.c[x] = c.a[x] * c.b[x];
        }
    }
    if (break_row >= 0 && !broke) throw ZkError(ZK_ERR_INVALID, "sample_circuit_lookup_fn: break_row must name a lookup row with a free a");
    c.sigma.resize(3 * N);
    for (size_t i = 0; i < 3 * N; ++i) c.sigma[i] = i;
    for (size_t y = 0; y < N; ++y) {
        if (users[y].empty()) continue;
        std::sort(users[y].begin(), users[y].end());
        uint64_t prev = 2 * N + y;
        for (uint64_t u : users[y]) c.sigma[prev] = u, prev = u;
        c.sigma[prev] = 2 * N + y;
    }
    c.t0.resize(N), c.t1.resize(N), c.t2.resize(N);
    for (size_t i = 0; i < N; ++i) {
        const uint64_t y = i < D ? i : D - 1;
        c.t0[i] = Fr::from_u64(y >> k), c.t1[i] = Fr::from_u64(y & low), c.t2[i] = Fr::from_u64((y >> k) ^ (y & low));
    }
    c.s = SplitMix64(base + 5).fr_vec(mu + 1);
    return c;
}
// SHA-256 of a sampled circuit's tables: the selectors, a, b, c, the public inputs, the trapdoor, sigma (u64) and, with a lookup, qk, t0,
// t1, t2 and idx (u32), little-endian in that order (zkhip.plonk.circuit_digest)
inline std::string circuit_digest(const PlonkCircuit &c) {
    Sha256 h;
    for (const FrVec &q : c.sel) h.update(q.data(), 32 * q.size());
    for (const FrVec *t : {&c.a, &c.b, &c.c, &c.public_inputs, &c.s}) h.update(t->data(), 32 * t->size());
    h.update(c.sigma.data(), 8 * c.sigma.size());
    if (c.lookup) {
        for (const FrVec *t : {&c.qk, &c.t0, &c.t1, &c.t2}) h.update(t->data(), 32 * t->size());
        h.update(c.idx.data(), 4 * c.idx.size());
    }
    return h.hex();
}

// ---- the verifier's closed forms ----
// in(r): prod_{i < mu - k} (1 - r_i) * sum_y pi[y] eq(y, r_{mu-k..}), index bit 0 the TOP bit
inline Fr in_eval(const FrVec &pi, const FrVec &r) {
    size_t k = 0;
    while ((size_t(1) << k) < pi.size()) ++k;
    const size_t mu = r.size();
    Fr head = Fr::one();
    for (size_t i = 0; i + k < mu; ++i) head *= Fr::one() - r[i];
    const FrVec tail(r.begin() + (mu - k), r.end());
    Fr acc = Fr::zero();
    for (size_t y = 0; y < pi.size(); ++y) {
        FrVec bits(k);
        for (size_t i = 0; i < k; ++i) bits[i] = ((y >> (k - 1 - i)) & 1) ? Fr::one() : Fr::zero();
        acc += pi[y] * eq_eval(bits, tail);
    }
    return head * acc;
}
// the multilinear extension of x -> x at r
inline Fr slot_eval(const FrVec &r) {
    Fr acc = Fr::zero();
    for (const Fr &x : r) acc = acc + acc + x;
    return acc;
}

// ---- keys ----
inline PlonkPk preprocess(Ctx &be, const PowersOfG &pg, const PlonkCircuit &c, PlonkVk &vk) {
    const size_t N = size_t(1) << c.mu;
    bool ok = c.mu >= 1 && c.l >= 1 && !(c.l & (c.l - 1)) && 2 * c.l <= N && c.sigma.size() == 3 * N && c.sel.size() == gate_desc(c.gate).selectors;
    for (const FrVec &q : c.sel) ok = ok && q.size() == N;
    if (!ok) throw ZkError(ZK_ERR_INVALID, "preprocess: mu >= 1, l = 2^k <= N / 2, the gate kind's selectors of N and sigma of 3N elements are needed");
    PlonkPk pk;
    pk.gate = vk.gate = c.gate;
    pk.mu = vk.mu = c.mu, pk.l = vk.l = c.l;
    for (const FrVec &q : c.sel) pk.sel.push_back(be.to_device(q));
    for (size_t j = 0; j < 3; ++j) {
        FrVec col(N);
        for (size_t x = 0; x < N; ++x) col[x] = Fr::from_u64(c.sigma[j * N + x]);
        pk.ssigma[j] = be.to_device(col);
    }
    for (const DevPtr &t : pk.sel) pk.commitments.push_back(commit(be, pg, t, N));
    for (const DevPtr &t : pk.ssigma) pk.commitments.push_back(commit(be, pg, t, N));
    pk.lookup = vk.lookup = c.lookup;
    if (c.lookup) {
        bool lok = c.qk.size() == N && c.t0.size() == N && c.t1.size() == N && c.t2.size() == N;
        for (size_t x = 0; lok && x < N; ++x) lok = c.qk[x].is_zero() || c.qk[x] == Fr::one();
        if (!lok) throw ZkError(ZK_ERR_INVALID, "preprocess: the lookup needs qk, t0, t1, t2 of N elements and every entry of qk 0 or 1");
        pk.qk = be.to_device(c.qk), pk.table = {be.to_device(c.t0), be.to_device(c.t1), be.to_device(c.t2)};
        pk.commitments.push_back(commit(be, pg, pk.qk, N));
        for (const DevPtr &t : pk.table) pk.commitments.push_back(commit(be, pg, t, N));
    }
    vk.commitments = pk.commitments;
    return pk;
}

namespace detail {
inline void plonk_claims(const PlonkProof &p, const FrVec &r_g, const FrVec &r_p, std::vector<Claim> &claims, std::vector<Claim> &v_claims) {
    // tables of the mu-variate instance: the selectors, a, b, c, ssigma_0..2
    const size_t ns = gate_desc(p.gate).selectors;
    for (size_t k = 0; k < ns + 3; ++k) claims.push_back(Claim{k, r_g, p.g_values[k]});
    for (size_t k = 0; k < 6; ++k) claims.push_back(Claim{ns + k, r_p, p.p_values[k]});
    const std::vector<FrVec> vp = v_points(r_p);
    for (size_t k = 0; k < 5; ++k) v_claims.push_back(Claim{0, vp[k], p.v_values[k]});
}
// with a lookup: the three claims a, b, c at r_l that the mu-variate instance gains, and the seven of the third instance (qk, t0, t1, t2, m, hf, ht)
inline void lookup_claims(const PlonkProof &p, const FrVec &r_l, std::vector<Claim> &claims, std::vector<Claim> &l_claims) {
    const size_t ns = gate_desc(p.gate).selectors;
    for (size_t k = 0; k < 3; ++k) claims.push_back(Claim{ns + k, r_l, p.l_values[k]});
    for (size_t j = 0; j < 7; ++j) l_claims.push_back(Claim{j, r_l, p.l_values[3 + j]});
}
inline FrVec replay_rounds(HostTranscript &tr, const std::vector<FrVec> &rounds) {
    FrVec out;
    for (const FrVec &r : rounds) out.push_back(tr.absorb(r).challenge());
    return out;
}
}  // namespace detail

// ---- prover ----  (pg: the levels of a PolynomialCommitment over mu + 1 variables; a zero alpha, of probability 2^-254, is refused)
namespace detail {
// find: the device finds the indices (zk_lookup3_find) and idx is not looked at
inline PlonkProof plonk_prove_with(Ctx &be, const PowersOfG &pg, const PlonkPk &pk, const DevPtr &a, const DevPtr &b, const DevPtr &c, const FrVec &public_inputs,
                                   const DevPtr &idx, bool find) {
    const size_t mu = pk.mu, l = pk.l, N = size_t(1) << mu;
    if (public_inputs.size() != l) throw ZkError(ZK_ERR_INVALID, "plonk_prove: l public inputs are needed");
    if (pk.lookup != (find || idx.get() != nullptr)) throw ZkError(ZK_ERR_INVALID, "plonk_prove: idx is needed exactly when the key has a lookup");
    const GateDesc &gd = gate_desc(pk.gate);
    const size_t ns = gd.selectors;
    PlonkProof p;
    p.gate = pk.gate, p.mu = mu, p.l = l, p.lookup = pk.lookup;
    const std::array<DevPtr, 3> w = {a, b, c};
    for (const DevPtr &t : w) p.commitments.push_back(commit(be, pg, t, N));
    std::shared_ptr<DeviceTranscript> tr = be.transcript(plonk_label(pk.gate, pk.lookup));
    const uint64_t mu64 = mu, l64 = l;
    be.absorb(*tr, &mu64, 8);
    be.absorb(*tr, &l64, 8);
    be.absorb(*tr, pk.commitments.data(), 144 * pk.commitments.size());
    be.absorb(*tr, public_inputs.data(), 32 * l);
    be.absorb(*tr, p.commitments.data(), 144 * 3);
    const FrVec ab = be.challenges(*tr, 2);
    const Fr alpha = ab[0], beta = ab[1];
    if (alpha.is_zero()) throw ZkError(ZK_ERR_INVALID, "plonk_prove: the challenge alpha is zero");
    DevPtr m, df, dt, hf, ht;
    Fr zeta, beta_l, gamma_l, lambda;
    if (pk.lookup) {  // 2L
        m = find ? be.lookup3_find(w, pk.table, pk.qk, N).second : be.lookup3_multiplicities(w, pk.table, pk.qk, idx, N);
        p.l_commitments.push_back(commit(be, pg, m, N));
        be.absorb(*tr, p.l_commitments.data(), 144);
        const FrVec zb = be.challenges(*tr, 2);
        zeta = zb[0], beta_l = zb[1];
    }
    Ctx::Perm3Terms t = be.perm3_terms(w, pk.ssigma, N, alpha, beta);
    DevPtr tree = be.product_tree(be.fr_batch_div(t.P, t.Q, N), N);
    p.v_commitment = commit(be, pg, tree, 2 * N);
    be.absorb(*tr, p.v_commitment.data(), 144);
    const Fr gamma = be.challenges(*tr, 1)[0];
    if (pk.lookup) {  // 3L
        std::tie(df, dt) = be.lookup3_terms(w, pk.table, N, zeta, beta_l);
        hf = be.fr_batch_div(pk.qk, df, N), ht = be.fr_batch_div(m, dt, N);
        p.l_commitments.push_back(commit(be, pg, hf, N)), p.l_commitments.push_back(commit(be, pg, ht, N));
        be.absorb(*tr, p.l_commitments.data() + 1, 144 * 2);
        const FrVec gl = be.challenges(*tr, 2);
        gamma_l = gl[0], lambda = gl[1];
    }
    FrVec p_last, r_p, g_last, r_g, r_l;
    {
        DevPtr eq = be.eq_table(be.challenges(*tr, mu));
        ScResult sc = be.sumcheck_perm3_fs(eq, tree, t.num, t.den, N, gamma, *tr, p_last, r_p);
        p.p_rounds.resize(mu);
        for (size_t i = 0; i < mu; ++i)
            for (int k = 0; k < 6; ++k) p.p_rounds[i][k] = sc.sums[6 * i + k];
    }
    {
        DevPtr eq = be.eq_table(be.challenges(*tr, mu));
        FrVec inp(N, Fr::zero());
        for (size_t y = 0; y < l; ++y) inp[y] = public_inputs[y];
        std::vector<DevPtr> tabs = {eq};
        tabs.insert(tabs.end(), pk.sel.begin(), pk.sel.end());
        tabs.insert(tabs.end(), {a, b, c, be.to_device(inp)});
        ScResult sc = gate_sumcheck_fs(be, pk.gate, tabs, N, *tr, g_last, r_g);
        for (size_t i = 0; i < mu; ++i) p.g_rounds.emplace_back(sc.sums.begin() + gd.evals * i, sc.sums.begin() + gd.evals * (i + 1));
    }
    if (pk.lookup) {  // 5L
        DevPtr E = be.fr_scale(be.eq_table(be.challenges(*tr, mu)), lambda, N);
        FrVec l_last;
        ScResult sc = be.sumcheck_lookup_sel_fs({E, df, dt, m, hf, ht, pk.qk}, N, gamma_l, *tr, l_last, r_l);
        p.l_rounds.resize(mu);
        for (size_t i = 0; i < mu; ++i)
            for (int k = 0; k < 4; ++k) p.l_rounds[i][k] = sc.sums[4 * i + k];
        // a, b, c, t0, t1, t2 at r_l: six folds in one batch, into one buffer; qk, m, hf, ht are the folded-out last values
        DevPtr at = be.alloc_fr(6);
        std::vector<ScRequest> folds;
        const DevPtr six[6] = {a, b, c, pk.table[0], pk.table[1], pk.table[2]};
        for (size_t j = 0; j < 6; ++j) folds.push_back(ScRequest{ScRequest::Fold, six[j], DevPtr(), N, r_l, at.fr(j)});
        be.sumcheck_batch(folds);
        const FrVec v = be.to_host(at, 6);
        p.l_values = {v[0], v[1], v[2], l_last[6], v[3], v[4], v[5], l_last[3], l_last[4], l_last[5]};
    }
    p.g_values.assign(g_last.begin() + 1, g_last.begin() + 1 + ns + 3);  // the folded-out values ARE the selectors and a, b, c at r_g
    // the folded-out n_j, d_j at r_p give the wires and the permutation columns there: both are linear in them
    const Fr ids = slot_eval(r_p), ainv = alpha.inverse();
    FrVec w_r(3), s_r(3);
    for (size_t j = 0; j < 3; ++j) {
        w_r[j] = p_last[5 + j] - alpha * (Fr::from_u64(j * N) + ids) - beta;
        s_r[j] = (p_last[8 + j] - w_r[j] - beta) * ainv;
    }
    p.p_values = {w_r[0], w_r[1], w_r[2], s_r[0], s_r[1], s_r[2]};
    Fr prod;  // the tree at (0,r) = h, (1,r) = v1x, (r,0) = vx0, (r,1) = vx1 are folded-out values too; (1,..,1,0) is tree[2N - 2]
    be.check(zk_memcpy_d2h(be.handle(), prod.v, (const char *)tree.get() + 32 * (2 * N - 2), 32));
    p.v_values = {p_last[4], p_last[1], p_last[2], p_last[3], prod};
    be.absorb(*tr, p.g_values.data(), 32 * (ns + 3));
    be.absorb(*tr, p.p_values.data(), 32 * 6);
    be.absorb(*tr, p.v_values.data(), 32 * 5);
    if (pk.lookup) be.absorb(*tr, p.l_values.data(), 32 * 10);
    const Fr b_alpha = be.challenges(*tr, 1)[0];
    std::vector<Claim> claims, v_claims, l_claims;
    detail::plonk_claims(p, r_g, r_p, claims, v_claims);
    if (pk.lookup) detail::lookup_claims(p, r_l, claims, l_claims);
    std::vector<DevPtr> batch_tables = pk.sel;
    batch_tables.insert(batch_tables.end(), {a, b, c, pk.ssigma[0], pk.ssigma[1], pk.ssigma[2]});
    p.batch = detail::batch_prove_ni(be, pg, batch_tables, N, claims, b_alpha, *tr);
    p.v_batch = detail::batch_prove_ni(be, pg, {tree}, 2 * N, v_claims, b_alpha, *tr);
    if (pk.lookup) p.l_batch = detail::batch_prove_ni(be, pg, {pk.qk, pk.table[0], pk.table[1], pk.table[2], m, hf, ht}, N, l_claims, b_alpha, *tr);
    return p;
}
}  // namespace detail

// idx: the N row-to-table indices (u32 on the device), needed exactly when the key has a lookup; a selected row whose triple is not the table
// entry it names: ZkError(ZK_ERR_INVALID)
inline PlonkProof plonk_prove(Ctx &be, const PowersOfG &pg, const PlonkPk &pk, const DevPtr &a, const DevPtr &b, const DevPtr &c, const FrVec &public_inputs,
                              const DevPtr &idx = DevPtr()) {
    return detail::plonk_prove_with(be, pg, pk, a, b, c, public_inputs, idx, false);
}
// the find mode (zkhip.plonk.FIND): no idx, the key must have a lookup; a selected row whose triple is no entry of the table:
// ZkError(ZK_ERR_INVALID).  The record is the one of plonk_prove with the indices of the first occurrences
inline PlonkProof plonk_prove(Ctx &be, const PowersOfG &pg, const PlonkPk &pk, const DevPtr &a, const DevPtr &b, const DevPtr &c, const FrVec &public_inputs,
                              FindIndices) {
    return detail::plonk_prove_with(be, pg, pk, a, b, c, public_inputs, DevPtr(), true);
}

// ---- verifier ----
// the replay of the schedule on the host transcript; false on a malformed record or statement (a record of another gate kind than the key's among them)
inline bool plonk_challenges(const PlonkVk &vk, const FrVec &pi, const PlonkProof &p, PlonkChallenges &c) {
    const size_t mu = vk.mu;
    const GateDesc &gd = gate_desc(vk.gate);
    const size_t ns = gd.selectors;
    const bool lk = vk.lookup;
    if (p.lookup != lk) return false;  // a record / key pair that disagrees on having a lookup is malformed
    if (lk && (p.l_commitments.size() != 3 || p.l_rounds.size() != mu || p.l_values.size() != 10 || p.l_batch.rounds.size() != mu || p.l_batch.opening.size() != mu))
        return false;
    if (p.gate != vk.gate || mu < 1 || p.mu != mu || p.l != vk.l || pi.size() != vk.l || vk.commitments.size() != ns + 3 + (lk ? 4 : 0) || p.commitments.size() != 3 ||
        p.p_rounds.size() != mu || p.g_rounds.size() != mu || p.batch.rounds.size() != mu || p.v_batch.rounds.size() != mu + 1 || p.g_values.size() != ns + 3 ||
        p.p_values.size() != 6 || p.v_values.size() != 5)
        return false;
    for (const FrVec &r : p.g_rounds)
        if (r.size() != gd.evals) return false;
    HostTranscript tr(plonk_label(vk.gate, lk));
    tr.absorb_u64(mu).absorb_u64(vk.l).absorb(vk.commitments.data(), 144 * vk.commitments.size()).absorb(pi);
    tr.absorb(p.commitments.data(), 144 * 3);
    c.alpha = tr.challenge(), c.beta = tr.challenge();
    if (lk) tr.absorb(p.l_commitments.data(), 144), c.zeta = tr.challenge(), c.beta_l = tr.challenge();
    c.gamma = tr.absorb(p.v_commitment.data(), 144).challenge();
    if (lk) tr.absorb(p.l_commitments.data() + 1, 144 * 2), c.gamma_l = tr.challenge(), c.lambda = tr.challenge();
    c.tau_p = tr.challenges(mu);
    c.r_p = detail::replay_rounds(tr, p.p_rounds);
    c.tau_g = tr.challenges(mu);
    c.r_g = detail::replay_rounds(tr, p.g_rounds);
    if (lk) {
        c.tau_l = tr.challenges(mu);
        for (const std::array<Fr, 4> &r : p.l_rounds) c.r_l.push_back(tr.absorb(r.data(), 32 * 4).challenge());
    }
    tr.absorb(p.g_values).absorb(p.p_values).absorb(p.v_values);
    if (lk) tr.absorb(p.l_values);
    c.b_alpha = tr.challenge();
    c.rho_mu = detail::replay_rounds(tr, p.batch.rounds);
    c.rho_mu1 = detail::replay_rounds(tr, p.v_batch.rounds);
    if (lk) c.rho_l = detail::replay_rounds(tr, p.l_batch.rounds);
    return true;
}

// The verifier's field arithmetic (no GPU, no pairing) -> a bit per failed check (0: all hold; bit 0: malformed): 1 the wiring chain,
// 2 the gate chain (on the gate kind's nodes), 3 the gate's last value (gate_closed_form) with in(r_g) formed here, 4 the wiring's last value with n_j formed here, 5 v(1,..,1,0) == 1,
// 6 the chains of the two batch instances; with a lookup 7 the lookup chain (nodes 0 .. 3), 8 its last value (lookup3_value on the ten l_values with
// E = lambda eq(tau_l, r_l)), 9 the third batch instance's chain (zkhip.plonk.failed_checks).
inline unsigned plonk_failed_checks(const PlonkVk &vk, const FrVec &pi, const PlonkProof &p, const PlonkChallenges &c) {
    const size_t mu = vk.mu, N = size_t(1) << mu, ns = gate_desc(vk.gate).selectors;
    if (p.gate != vk.gate || p.lookup != vk.lookup) return 1u;
    unsigned bad = 0;
    Fr p_target, g_target;
    if (!round_chain(p.p_rounds, 6, c.r_p, Fr::zero(), &p_target)) bad |= 1u << 1;
    if (!round_chain(p.g_rounds, gate_desc(vk.gate).evals, c.r_g, Fr::zero(), &g_target)) bad |= 1u << 2;
    const FrVec &g = p.g_values, &v = p.p_values, &t = p.v_values;  // g: the selectors, a, b, c;  t: v(0,r), v(1,r), v(r,0), v(r,1), v(1,..,1,0)
    if (!(bad & (1u << 2)) && g_target != gate_closed_form(vk.gate, eq_eval(c.tau_g, c.r_g), g, in_eval(pi, c.r_g))) bad |= 1u << 3;
    const Fr ids = slot_eval(c.r_p);
    Fr nn = Fr::one(), dd = Fr::one();
    for (size_t j = 0; j < 3; ++j) {
        nn *= v[j] + c.alpha * (Fr::from_u64(j * N) + ids) + c.beta;
        dd *= v[j] + c.alpha * v[3 + j] + c.beta;
    }
    if (!(bad & (1u << 1)) && p_target != eq_eval(c.tau_p, c.r_p) * (t[1] - t[2] * t[3] + c.gamma * (t[0] * dd - nn))) bad |= 1u << 4;
    if (t[4] != Fr::one()) bad |= 1u << 5;
    std::vector<Claim> claims, v_claims, l_claims;
    detail::plonk_claims(p, c.r_g, c.r_p, claims, v_claims);
    if (vk.lookup) detail::lookup_claims(p, c.r_l, claims, l_claims);
    if (failed_checks(ns + 6, claims, p.batch, c.b_alpha, c.rho_mu) || failed_checks(1, v_claims, p.v_batch, c.b_alpha, c.rho_mu1)) bad |= 1u << 6;
    if (vk.lookup) {
        Fr target;
        if (!round_chain(p.l_rounds, 4, c.r_l, Fr::zero(), &target)) bad |= 1u << 7;
        if (!(bad & (1u << 7)) && target != lookup3_value(c.lambda * eq_eval(c.tau_l, c.r_l), p.l_values, c.zeta, c.beta_l, c.gamma_l)) bad |= 1u << 8;
        if (failed_checks(7, l_claims, p.l_batch, c.b_alpha, c.rho_l)) bad |= 1u << 9;
    }
    return bad;
}

inline bool plonk_verify(Ctx &be, const PcsVk &vk_mu, const PcsVk &vk_mu1, const PlonkVk &vk, const FrVec &pi, const PlonkProof &p) {
    PlonkChallenges c;
    if (!plonk_challenges(vk, pi, p, c) || plonk_failed_checks(vk, pi, p, c)) return false;
    std::vector<Claim> claims, v_claims, l_claims;
    detail::plonk_claims(p, c.r_g, c.r_p, claims, v_claims);
    if (vk.lookup) detail::lookup_claims(p, c.r_l, claims, l_claims);
    const size_t ns = gate_desc(vk.gate).selectors;  // the tables of the mu-variate instance: the selectors, a, b, c, ssigma_0..2
    G1Vec comms(vk.commitments.begin(), vk.commitments.begin() + ns);
    comms.insert(comms.end(), p.commitments.begin(), p.commitments.end());
    comms.insert(comms.end(), vk.commitments.begin() + ns, vk.commitments.begin() + ns + 3);
    try {
        if (!batch_open_verify(be, vk_mu, comms, claims, p.batch, c.b_alpha, c.rho_mu) ||
            !batch_open_verify(be, vk_mu1, G1Vec{p.v_commitment}, v_claims, p.v_batch, c.b_alpha, c.rho_mu1))
            return false;
        if (!vk.lookup) return true;
        G1Vec l_comms(vk.commitments.begin() + ns + 3, vk.commitments.end());  // the third instance: qk, t0, t1, t2, m, hf, ht
        l_comms.insert(l_comms.end(), p.l_commitments.begin(), p.l_commitments.end());
        return batch_open_verify(be, vk_mu, l_comms, l_claims, p.l_batch, c.b_alpha, c.rho_l);
    } catch (const ZkError &e) {  // a point of the record that is not on the curve is refused by the pairing call: a record to reject
        if (e.status != ZK_ERR_INVALID) throw;
        return false;
    }
}

// ---- aggregated verification: many proofs, one pairing check (zkhip.plonk.agg_openings / verify_many / verify_agg) ----
struct PlonkItem {
    FrVec public_inputs;
    PlonkProof proof;
};
// the replay and the checks of plonk_failed_checks for every item; the batch instances of the survivors -- two each, with a lookup three --
// as openings over the FULL key: skip = 1 for the mu-variate instances, 0 for the tree's.  alive: the indices of the survivors
inline AggArrays plonk_agg_openings(const PlonkVk &vk, const std::vector<PlonkItem> &items, std::vector<size_t> &alive) {
    AggArrays all;
    alive.clear();
    const size_t ns = gate_desc(vk.gate).selectors;
    for (size_t n = 0; n < items.size(); ++n) {
        const PlonkProof &p = items[n].proof;
        PlonkChallenges c;
        if (!plonk_challenges(vk, items[n].public_inputs, p, c) || plonk_failed_checks(vk, items[n].public_inputs, p, c)) continue;
        std::vector<Claim> claims, v_claims, l_claims;
        detail::plonk_claims(p, c.r_g, c.r_p, claims, v_claims);
        if (vk.lookup) detail::lookup_claims(p, c.r_l, claims, l_claims);
        G1Vec comms(vk.commitments.begin(), vk.commitments.begin() + ns);  // batch_tables order
        comms.insert(comms.end(), p.commitments.begin(), p.commitments.end());
        comms.insert(comms.end(), vk.commitments.begin() + ns, vk.commitments.begin() + ns + 3);
        AggArrays mine;
        bool ok = opening_claim(comms, claims, p.batch, c.b_alpha, c.rho_mu, 1, mine) &&
                  opening_claim(G1Vec{p.v_commitment}, v_claims, p.v_batch, c.b_alpha, c.rho_mu1, 0, mine);
        if (ok && vk.lookup) {
            G1Vec l_comms(vk.commitments.begin() + ns + 3, vk.commitments.end());
            l_comms.insert(l_comms.end(), p.l_commitments.begin(), p.l_commitments.end());
            ok = opening_claim(l_comms, l_claims, p.l_batch, c.b_alpha, c.rho_l, 1, mine);
        }
        if (!ok) continue;
        alive.push_back(n);
        all.append(mine);
    }
    return all;
}
// plonk_verify for a list: ONE zk_pcs_verify_agg call for the batch instances of all surviving proofs.  When the aggregate accepts every
// survivor is true; when it rejects -- or refuses a point that is not on the curve -- the survivors go one by one through plonk_verify,
// so the bad one is named.  weights (optional): what zk_pcs_agg_weights derives from the aggregate's input arrays, count x 2 u64 --
// computed here on the host for the caller, not read back from the call, which derives the same bits again
inline std::vector<bool> plonk_verify_many(Ctx &be, const PcsVk &vk_mu, const PcsVk &vk_mu1, const PlonkVk &vk, const std::vector<PlonkItem> &items,
                                           std::vector<uint64_t> *weights = nullptr) {
    std::vector<size_t> alive;
    const AggArrays openings = plonk_agg_openings(vk, items, alive);
    if (weights) *weights = pcs_agg_weights(openings);
    bool ok = true;
    if (!alive.empty()) {
        try {
            ok = verify_agg(be, vk_mu1, openings);
        } catch (const ZkError &e) {
            if (e.status != ZK_ERR_INVALID) throw;
            ok = false;
        }
    }
    std::vector<bool> out(items.size(), false);
    for (size_t n : alive) out[n] = ok || plonk_verify(be, vk_mu, vk_mu1, vk, items[n].public_inputs, items[n].proof);
    return out;
}
// plonk_verify with ONE pairing call instead of two or three: plonk_verify_many of one proof
inline bool plonk_verify_agg(Ctx &be, const PcsVk &vk_mu, const PcsVk &vk_mu1, const PlonkVk &vk, const FrVec &pi, const PlonkProof &p) {
    return plonk_verify_many(be, vk_mu, vk_mu1, vk, {PlonkItem{pi, p}})[0];
}

// zkhip.plonk.proof_digest: the record's words in the order of the schedule
inline std::string proof_digest(const PlonkProof &p) {
    Sha256 h;
    const uint64_t mu = p.mu, l = p.l;
    h.update(&mu, 8);
    h.update(&l, 8);
    h.update(p.commitments.data(), 144 * p.commitments.size());
    h.update(p.v_commitment.data(), 144);
    for (auto &r : p.p_rounds) h.update(r.data(), 6 * 32);
    for (auto &r : p.g_rounds) h.update(r.data(), 32 * r.size());
    h.update(p.g_values.data(), 32 * p.g_values.size());
    h.update(p.p_values.data(), 32 * p.p_values.size());
    h.update(p.v_values.data(), 32 * p.v_values.size());
    detail::digest_batch(h, p.batch);
    detail::digest_batch(h, p.v_batch);
    if (p.lookup) {
        h.update(p.l_commitments.data(), 144 * p.l_commitments.size());
        for (auto &r : p.l_rounds) h.update(r.data(), 4 * 32);
        h.update(p.l_values.data(), 32 * p.l_values.size());
        detail::digest_batch(h, p.l_batch);
    }
    return h.hex();
}

}  // namespace zkhost
