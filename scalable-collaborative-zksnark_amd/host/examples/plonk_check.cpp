// plonk_check -- one HyperPlonk proof of one circuit on the compiled host (zkhost/plonk.hpp): the test circuit of
// zkhip.plonk.sample_circuit (the same SplitMix64 streams, so the same tables for one seed), preprocessed, proved with every challenge
// drawn from the device transcript and verified by replaying the schedule on the host transcript.  One digest for one seed across the
// two hosts (zkhip.plonk.proof_digest).
//
//     bin/plonk_check --mu M [--seed S] [--gate wide] [--break-gate K | --break-wire K | --bad-input] [--circuit-only]
//
// --gate wide proves the test circuit of the wide gate (zkhip.plonk.sample_circuit_wide: six selectors and a fifth-power term) instead.
// --break-gate K adds 1 to c[K]; --break-wire K (K past the input rows) changes a[K] and recomputes c[K], so that only the copy
// constraint fails; --bad-input hands the verifier a public input the prover did not use.  The verifier rejects each.  Prints the proof
// digest and accept / reject; exit 0 on accept, 1 on reject, 2 on error (arguments are checked before any device is touched).
// Without a GPU it refuses (no CPU fallback) -- but for --circuit-only, which builds the test circuit, prints the SHA-256 of its tables (the
// selectors, a, b, c, the public inputs, the trapdoor, sigma: little-endian words in that order) and exits 0 without touching a device.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "zkhost/hyperplonk.hpp"
#include "zkhost/pcs_vk.hpp"
#include "zkhost/plonk.hpp"

using namespace zkhost;

static bool number(const char *s, long long &out) {
    char *end = nullptr;
    out = std::strtoll(s, &end, 10);
    return *s && end && !*end && out >= 0;
}

static int circuit_only(size_t mu, uint64_t seed, bool wide, long long break_gate, long long break_wire) {
    const PlonkCircuit c = (wide ? sample_circuit_wide : sample_circuit)(mu, seed, break_gate, break_wire);
    Sha256 h;
    for (const FrVec &q : c.sel) h.update(q.data(), 32 * q.size());
    for (const FrVec *t : {&c.a, &c.b, &c.c, &c.public_inputs, &c.s}) h.update(t->data(), 32 * t->size());
    h.update(c.sigma.data(), 8 * c.sigma.size());
    std::printf("circuit sha256 %s\n", h.hex().c_str());
    return 0;
}

static int run(size_t mu, uint64_t seed, bool wide, long long break_gate, long long break_wire, bool bad_input) {
    Ctx be(0);
    const size_t N = size_t(1) << mu;
    const auto sample = wide ? sample_circuit_wide : sample_circuit;
    const PlonkCircuit good = sample(mu, seed, -1, -1), c = sample(mu, seed, break_gate, break_wire);
    PolynomialCommitmentCub cub = PolynomialCommitmentCub::make(be, good.s);
    // level mu of the parameter set uses s_1 .. s_mu: its openings verify against [g2, s_1 g2, .., s_mu g2]
    std::shared_ptr<PcsVk> vk_mu1 = make_pcs_vk(be, good.s), vk_mu = make_pcs_vk(be, FrVec(good.s.begin() + 1, good.s.end()));
    PlonkVk vk;
    const PlonkPk pk = preprocess(be, cub.mature(), good, vk);
    const PlonkProof proof = plonk_prove(be, cub.mature(), pk, be.to_device(c.a), be.to_device(c.b), be.to_device(c.c), good.public_inputs);
    FrVec pi = good.public_inputs;
    if (bad_input) pi[1] += Fr::one();
    const bool ok = plonk_verify(be, *vk_mu, *vk_mu1, vk, pi, proof);
    std::printf("proof sha256 %s\n", proof_digest(proof).c_str());
    std::printf("plonk_check mu=%zu N=%zu l=%zu seed=%llu%s: %s\n", mu, N, good.l, (unsigned long long)seed, wide ? " gate=wide" : "", ok ? "accept" : "reject");
    return ok ? 0 : 1;
}

int main(int argc, char **argv) {
    long long mu = -1, seed = 7, break_gate = -1, break_wire = -1;
    bool bad_input = false, wide = false, only_circuit = false, usage = argc < 2;
    for (int i = 1; i < argc && !usage; ++i) {
        const std::string k = argv[i];
        if (k == "--bad-input") bad_input = true;
        else if (k == "--circuit-only") only_circuit = true;
        else if (i + 1 < argc && k == "--gate") usage = std::strcmp(argv[++i], "wide") != 0, wide = true;
        else if (i + 1 < argc && k == "--mu") usage = !number(argv[++i], mu);
        else if (i + 1 < argc && k == "--seed") usage = !number(argv[++i], seed);
        else if (i + 1 < argc && k == "--break-gate") usage = !number(argv[++i], break_gate);
        else if (i + 1 < argc && k == "--break-wire") usage = !number(argv[++i], break_wire);
        else usage = true;
    }
    if (usage || mu < 0 || (break_gate >= 0) + (break_wire >= 0) + (bad_input ? 1 : 0) > 1) {
        std::fprintf(stderr, "usage: plonk_check --mu M [--seed S] [--gate wide] [--break-gate K | --break-wire K | --bad-input] [--circuit-only]\n");
        return 2;
    }
    if (mu < 2 || mu > 24) {
        std::fprintf(stderr, "plonk_check: --mu must be in [2, 24]\n");
        return 2;
    }
    const long long N = 1ll << mu, l = N / 2 < 4 ? N / 2 : 4;
    if (break_gate >= N || break_wire >= N || (break_wire >= 0 && break_wire < l)) {
        std::fprintf(stderr, "plonk_check: --break-gate must be below 2^mu, --break-wire in [l, 2^mu) with l = %lld input rows\n", l);
        return 2;
    }
    if (only_circuit) return circuit_only((size_t)mu, (uint64_t)seed, wide, break_gate, break_wire);
    int ngpu = zk_device_count();
    if (ngpu <= 0) {
        std::fprintf(stderr, "plonk_check: no GPU visible -- this host has no CPU fallback (zk_device_count = %d)\n", ngpu);
        return 2;
    }
    try {
        return run((size_t)mu, (uint64_t)seed, wide, break_gate, break_wire, bad_input);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "plonk_check: %s\n", e.what());
        return 2;
    }
}
