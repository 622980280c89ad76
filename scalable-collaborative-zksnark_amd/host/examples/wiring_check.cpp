// wiring_check -- the wiring identity proved and verified end to end on the compiled host (zkhost/wiring.hpp): a satisfied
// copy-constraint system from SplitMix64 (sigma = i -> 5 i + b mod 8 inside aligned blocks of 8, one 8-cycle per block; w constant on
// every block; sid[i] = i, ssigma[i] = sigma(i)), a structured parameter set over mu + 1 variables with its powers_of_g2, the
// fractions, the product tree, the eq table and the degree-3 wiring sumcheck (zk_sumcheck_wiring -- what hyperplonk.rs:94-141
// simulates), eight openings, and the verifier with two zk_pcs_verify_batch calls.  The same circuit, proof record and digest as
// zkhip/wiring.py (tools/wiring_time.py --digest).
//
//     bin/wiring_check [--n MU] [--seed S] [--break-wire K] [--break-opening J] [--digest]
//
// --break-wire K adds 1 to w[K] (the grand product is no longer 1: check 3 fails); --break-opening J replaces one point of an opening
// proof by another curve point AFTER proving (J = 0 .. 2: w, sid, ssigma; 3 .. 7: the tree at (0,r), (1,r), (r,0), (r,1), (1,..,1,0)):
// the field checks pass, the pairing of zk_pcs_verify_batch rejects.  Prints the verdict of every check, accept / reject and the times;
// exit 0 on accept, 1 on reject, 2 on error.  Without a GPU it refuses (no CPU fallback).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "sha256.hpp"
#include "zkhost/hyperplonk.hpp"
#include "zkhost/pcs_vk.hpp"
#include "zkhost/wiring.hpp"

using namespace zkhost;

static const uint64_t kCircuitSeed = 0x3B1E0000;  // zkhip/wiring.py CIRCUIT_SEED

// zkhip.wiring.proof_digest
static std::string proof_digest(const WiringProof &p) {
    Sha256 h;
    for (auto &r : p.rounds) h.update(r.data(), 4 * 32);
    for (auto &o : p.openings) h.update(o.commitment.data(), 144), h.update(o.value.v, 32), h.update(o.proof.data(), 144 * o.proof.size());
    h.update(p.v_commitment.data(), 144);
    for (auto &o : p.v_openings) h.update(o.value.v, 32), h.update(o.proofs.data(), 144 * o.proofs.size());
    return h.hex();
}

int main(int argc, char **argv) {
    size_t mu = 12;
    uint64_t seed = 7;
    long long brk = -1, brk_open = -1;
    bool digest = false;
    for (int i = 1; i < argc; ++i) {
        std::string k = argv[i];
        if (k == "--digest") digest = true;
        else if (i + 1 < argc && k == "--n") mu = std::strtoull(argv[++i], nullptr, 10);
        else if (i + 1 < argc && k == "--seed") seed = std::strtoull(argv[++i], nullptr, 10);
        else if (i + 1 < argc && k == "--break-wire") brk = std::strtoll(argv[++i], nullptr, 10);
        else if (i + 1 < argc && k == "--break-opening") brk_open = std::strtoll(argv[++i], nullptr, 10);
        else {
            std::fprintf(stderr, "usage: wiring_check [--n MU] [--seed S] [--break-wire K] [--break-opening J] [--digest]\n");
            return 2;
        }
    }
    int ngpu = zk_device_count();
    if (ngpu <= 0) {
        std::fprintf(stderr, "wiring_check: no GPU visible -- this host has no CPU fallback (zk_device_count = %d)\n", ngpu);
        return 2;
    }
    if (mu < 1 || mu > 24 || (brk >= 0 && (size_t)brk >= (size_t(1) << mu)) || brk_open > 7) {
        std::fprintf(stderr, "wiring_check: --n must be in [1, 24], --break-wire below 2^n, --break-opening in [0, 7]\n");
        return 2;
    }
    try {
        Ctx be(0);
        const size_t N = size_t(1) << mu, blk = N < 8 ? N : 8;
        const uint64_t base = kCircuitSeed + 1000 * seed, b = (2 * seed + 1) & 7;
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
        WiringScalars sc;
        sc.alpha = SplitMix64(base + 2).fr_vec(1)[0], sc.beta = SplitMix64(base + 3).fr_vec(1)[0], sc.gamma = SplitMix64(base + 4).fr_vec(1)[0];
        sc.tau = SplitMix64(base + 5).fr_vec(mu), sc.chal = SplitMix64(base + 6).fr_vec(mu);
        const FrVec s = SplitMix64(base + 7).fr_vec(mu + 1);
        PolynomialCommitmentCub cub = PolynomialCommitmentCub::make(be, s);
        // level mu of the parameter set uses s_1 .. s_mu: its openings verify against [g2, s_1 g2, .., s_mu g2]
        std::shared_ptr<PcsVk> vk_mu1 = make_pcs_vk(be, s), vk_mu = make_pcs_vk(be, FrVec(s.begin() + 1, s.end()));

        double sec[2] = {0, 0};
        WiringProof proof = wiring_prove(be, cub.mature(), w, sid, ssigma, N, sc, sec);
        if (brk_open >= 0) {  // one proof point of that opening + g1: still on the curve and in the subgroup
            uint64_t g1a[12];
            be.check(zk_srs_download(be.handle(), cub.mature()[0]->handle(), g1a));
            G1 g1{};
            std::memcpy(g1.data(), g1a, 96);
            std::memcpy(g1.data() + 12, Fq::one().v, 48);
            G1 &pt = brk_open < 3 ? proof.openings[(size_t)brk_open].proof[mu / 2] : proof.v_openings[(size_t)brk_open - 3].proofs[mu / 2];
            pt = be.g1_lincomb_batch(G1Vec{pt, g1}, FrVec{Fr{{1, 0, 0, 0}}, Fr{{1, 0, 0, 0}}}, 1)[0];
        }
        auto t0 = std::chrono::steady_clock::now();
        const unsigned bad = failed_checks(proof, sc);
        const bool open_ok = verify_openings(be, *vk_mu, *vk_mu1, proof, sc.chal);
        const double tv = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        const bool ok = bad == 0 && open_ok;
        if (bad & 1u) std::printf("malformed proof record\n");
        std::printf("check 1 (round chain): %s\n", bad & 2u ? "failed" : "ok");
        std::printf("check 2 (final identity): %s\n", bad & 4u ? "failed" : (bad & 2u ? "not reached" : "ok"));
        std::printf("check 3 (grand product = 1): %s\n", bad & 8u ? "failed" : "ok");
        std::printf("check 4 (eight openings, device pairing): %s\n", open_ok ? "ok" : "failed");
        std::printf("wiring_check n=%zu seed=%llu: %s\n", mu, (unsigned long long)seed, ok ? "accept" : "reject");
        std::printf("tables %.3f ms  sumcheck_wiring %.3f ms  verify %.3f ms\n", sec[0] * 1e3, sec[1] * 1e3, tv * 1e3);
        if (digest) std::printf("proof sha256 %s\n", proof_digest(proof).c_str());
        return ok ? 0 : 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "wiring_check: %s\n", e.what());
        return 2;
    }
}
