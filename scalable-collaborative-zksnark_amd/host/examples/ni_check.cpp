// ni_check -- the non-interactive gate ZeroCheck and wiring PermCheck on the compiled host (zkhost/nizk.hpp): the circuits of
// gate_check / wiring_check (the same SplitMix64 streams, so the same tables as zkhip.zerocheck.satisfied_circuit and
// zkhip.wiring.permuted_circuit for one seed), proved with every challenge drawn from the device transcript and verified by replaying
// the schedule on the host transcript.  One digest for one seed across the two hosts (zkhip.nizk.proof_digest).
//
//     bin/ni_check --which gate|wiring [--n N] [--seed S] [--break K]
//     bin/ni_check --vectors
//
// --break K adds 1 to c[K] (gate) or to w[K] (wiring) before proving: the verifier rejects.  Prints the proof digest and accept /
// reject; exit 0 on accept, 1 on reject, 2 on error.  Without a GPU it refuses (no CPU fallback).
// --vectors needs no GPU: the transcript test vectors tests/test_fs.py compares with zkhip.transcript.HostTranscript, line by line --
// for the labels "", "gate" and "wiring" the state after init, then for absorbs of 0, 1, 22, 23, 54, 55, 56, 63, 64, 119 and 120 bytes
// (the padding boundaries after the 33-byte prefix; byte i of an absorb is (7 i + 3 + |label|) mod 256) the state and two challenges
// as four u64 limbs in Montgomery form.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "zkhost/hyperplonk.hpp"
#include "zkhost/nizk.hpp"
#include "zkhost/pcs_vk.hpp"

using namespace zkhost;

static int vectors() {
    const size_t lengths[] = {0, 1, 22, 23, 54, 55, 56, 63, 64, 119, 120};
    for (const std::string label : {"", "gate", "wiring"}) {
        HostTranscript tr(label);
        std::printf("init %s %s\n", label.empty() ? "-" : label.c_str(), tr.state_hex().c_str());
        for (size_t n : lengths) {
            std::vector<uint8_t> data(n);
            for (size_t i = 0; i < n; ++i) data[i] = (uint8_t)(7 * i + 3 + label.size());
            tr.absorb(data.data(), n);
            std::printf("absorb %zu %s\n", n, tr.state_hex().c_str());
            for (const Fr &c : tr.challenges(2))
                std::printf("challenge %016llx%016llx%016llx%016llx\n", (unsigned long long)c.v[0], (unsigned long long)c.v[1], (unsigned long long)c.v[2],
                            (unsigned long long)c.v[3]);
        }
    }
    return 0;
}

static int gate(size_t n, uint64_t seed, long long brk) {
    Ctx be(0);
    const size_t len = size_t(1) << n;
    const uint64_t base = 0x6A7E0000 + 1000 * seed;  // zkhip/zerocheck.py CIRCUIT_SEED
    GateTables t;
    const char *drawn[5] = {"a", "b", "q1", "q2", "in"};
    for (int k = 0; k < 5; ++k) t[drawn[k]] = be.to_device(SplitMix64(base + 1 + k).fr_vec(len));
    DevPtr lin = be.fr_mul(t["q1"], be.fr_add(t["a"], t["b"], len), len);
    t["c"] = be.fr_add(be.fr_add(lin, be.fr_mul(be.fr_mul(t["q2"], t["a"], len), t["b"], len), len), t["in"], len);
    if (brk >= 0) {
        Fr v;
        be.check(zk_memcpy_d2h(be.handle(), v.v, (const char *)t["c"].get() + 32 * (size_t)brk, 32));
        v += Fr::one();
        be.check(zk_memcpy_h2d(be.handle(), (char *)t["c"].get() + 32 * (size_t)brk, v.v, 32));
    }
    const FrVec s = SplitMix64(base + 8).fr_vec(n);
    PolynomialCommitmentCub cub = PolynomialCommitmentCub::make(be, s);
    std::shared_ptr<PcsVk> vk = make_pcs_vk(be, s);
    const GateProofNi proof = gate_prove_ni(be, cub.mature(), t, n);
    const bool ok = gate_verify_ni(be, *vk, proof);
    std::printf("proof sha256 %s\n", proof_digest(proof).c_str());
    std::printf("ni_check gate n=%zu seed=%llu: %s\n", n, (unsigned long long)seed, ok ? "accept" : "reject");
    return ok ? 0 : 1;
}

static int wiring(size_t mu, uint64_t seed, long long brk) {
    Ctx be(0);
    const size_t N = size_t(1) << mu, blk = N < 8 ? N : 8;
    const uint64_t base = 0x3B1E0000 + 1000 * seed, b = (2 * seed + 1) & 7;  // zkhip/wiring.py CIRCUIT_SEED, block_permutation
    const FrVec val = SplitMix64(base + 1).fr_vec(N >> 3 ? N >> 3 : 1);
    FrVec wv(N), idv(N), sgv(N);
    for (size_t i = 0; i < N; ++i) {
        const size_t low = i & (blk - 1);
        wv[i] = val[i >> 3];
        idv[i] = Fr::from_u64(i);
        sgv[i] = Fr::from_u64((i - low) + ((5 * low + b) & (blk - 1)));
    }
    if (brk >= 0) wv[(size_t)brk] += Fr::one();
    DevPtr w = be.to_device(wv), sid = be.to_device(idv), ssigma = be.to_device(sgv);
    const FrVec s = SplitMix64(base + 7).fr_vec(mu + 1);
    PolynomialCommitmentCub cub = PolynomialCommitmentCub::make(be, s);
    // level mu of the parameter set uses s_1 .. s_mu: its openings verify against [g2, s_1 g2, .., s_mu g2]
    std::shared_ptr<PcsVk> vk_mu1 = make_pcs_vk(be, s), vk_mu = make_pcs_vk(be, FrVec(s.begin() + 1, s.end()));
    const WiringProofNi proof = wiring_prove_ni(be, cub.mature(), w, sid, ssigma, N);
    const bool ok = wiring_verify_ni(be, *vk_mu, *vk_mu1, proof);
    std::printf("proof sha256 %s\n", proof_digest(proof).c_str());
    std::printf("ni_check wiring n=%zu seed=%llu: %s\n", mu, (unsigned long long)seed, ok ? "accept" : "reject");
    return ok ? 0 : 1;
}

int main(int argc, char **argv) {
    size_t n = 12;
    uint64_t seed = 7;
    long long brk = -1;
    std::string which;
    for (int i = 1; i < argc; ++i) {
        std::string k = argv[i];
        if (k == "--vectors") return vectors();
        else if (i + 1 < argc && k == "--which") which = argv[++i];
        else if (i + 1 < argc && k == "--n") n = std::strtoull(argv[++i], nullptr, 10);
        else if (i + 1 < argc && k == "--seed") seed = std::strtoull(argv[++i], nullptr, 10);
        else if (i + 1 < argc && k == "--break") brk = std::strtoll(argv[++i], nullptr, 10);
        else which = "?";
    }
    if (which != "gate" && which != "wiring") {
        std::fprintf(stderr, "usage: ni_check --which gate|wiring [--n N] [--seed S] [--break K]   |   ni_check --vectors\n");
        return 2;
    }
    int ngpu = zk_device_count();
    if (ngpu <= 0) {
        std::fprintf(stderr, "ni_check: no GPU visible -- this host has no CPU fallback (zk_device_count = %d)\n", ngpu);
        return 2;
    }
    if (n < 1 || n > 24 || (brk >= 0 && (size_t)brk >= (size_t(1) << n))) {
        std::fprintf(stderr, "ni_check: --n must be in [1, 24], --break below 2^n\n");
        return 2;
    }
    try {
        return which == "gate" ? gate(n, seed, brk) : wiring(n, seed, brk);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "ni_check: %s\n", e.what());
        return 2;
    }
}
