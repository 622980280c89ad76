// batch_open_check -- one batch-opening instance proved and verified end to end on the compiled host (zkhost/batch_open.hpp): J random
// tables of 2^n elements from SplitMix64, K claims at random, repeated and boolean points (the last one (1,..,1,0)), the values by
// zk_fold, a structured parameter set with its powers_of_g2, the combined eq tables, the fused degree-2 sumcheck (zk_sumcheck_multi),
// ONE opening of sum_j e_j f_j, and the verifier: round chain, C_g by zk_g1_lincomb, one zk_pcs_verify_batch call.  The same instance,
// proof record and digest as zkhip/batch_open.py (random_instance; tools/batch_open_time.py --digest).
//
//     bin/batch_open_check [--n N] [--seed S] [--tables J] [--claims K] [--break-value K] [--break-opening] [--digest]
//
// --break-value K adds 1 to the claimed value v_K AFTER proving (the round chain no longer starts at S: check 1 fails);
// --break-opening replaces point n/2 of the opening proof by another curve point AFTER proving: the field checks pass, the pairing of
// zk_pcs_verify_batch rejects.  Prints the verdict of every check, accept / reject and the times; exit 0 on accept, 1 on reject, 2 on
// error.  Without a GPU it refuses (no CPU fallback).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "sha256.hpp"
#include "zkhost/batch_open.hpp"
#include "zkhost/hyperplonk.hpp"
#include "zkhost/pcs_vk.hpp"

using namespace zkhost;

static const uint64_t kInstanceSeed = 0x0BA70000;  // zkhip/batch_open.py INSTANCE_SEED

// zkhip.batch_open.proof_digest
static std::string proof_digest(const BatchOpenProof &p) {
    Sha256 h;
    for (auto &r : p.rounds) h.update(r.data(), 3 * 32);
    h.update(p.opening.data(), 144 * p.opening.size());
    return h.hex();
}

int main(int argc, char **argv) {
    size_t n = 10, J = 4, K = 9;
    uint64_t seed = 7;
    long long brk = -1;
    bool brk_open = false, digest = false;
    for (int i = 1; i < argc; ++i) {
        std::string k = argv[i];
        if (k == "--digest") digest = true;
        else if (k == "--break-opening") brk_open = true;
        else if (i + 1 < argc && k == "--n") n = std::strtoull(argv[++i], nullptr, 10);
        else if (i + 1 < argc && k == "--seed") seed = std::strtoull(argv[++i], nullptr, 10);
        else if (i + 1 < argc && k == "--tables") J = std::strtoull(argv[++i], nullptr, 10);
        else if (i + 1 < argc && k == "--claims") K = std::strtoull(argv[++i], nullptr, 10);
        else if (i + 1 < argc && k == "--break-value") brk = std::strtoll(argv[++i], nullptr, 10);
        else {
            std::fprintf(stderr, "usage: batch_open_check [--n N] [--seed S] [--tables J] [--claims K] [--break-value K] [--break-opening] [--digest]\n");
            return 2;
        }
    }
    int ngpu = zk_device_count();
    if (ngpu <= 0) {
        std::fprintf(stderr, "batch_open_check: no GPU visible -- this host has no CPU fallback (zk_device_count = %d)\n", ngpu);
        return 2;
    }
    if (n < 1 || n > 24 || J < 1 || J > 16 || K < 1 || K > 64 || (brk >= 0 && (size_t)brk >= K)) {
        std::fprintf(stderr, "batch_open_check: --n in [1, 24], --tables in [1, 16], --claims in [1, 64], --break-value below the number of claims\n");
        return 2;
    }
    try {
        Ctx be(0);
        const size_t N = size_t(1) << n;
        const uint64_t base = kInstanceSeed + 1000 * seed;
        std::vector<DevPtr> tables;
        for (size_t j = 0; j < J; ++j) tables.push_back(be.to_device(SplitMix64(base + 10 + j).fr_vec(N)));
        std::vector<std::pair<size_t, FrVec>> pts;
        for (size_t k = 0; k < K; ++k) {
            FrVec z;
            if (k % 3 == 0) z = SplitMix64(base + 100 + k).fr_vec(n);
            else if (k % 3 == 1) z = pts.back().second;
            else if (k == K - 1) z.assign(n - 1, Fr::one()), z.push_back(Fr::zero());
            else
                for (size_t i = 0; i < n; ++i) z.push_back(((k + i) & 1) ? Fr::one() : Fr::zero());
            pts.push_back({k % J, z});
        }
        const Fr alpha = SplitMix64(base + 1).fr_vec(1)[0];
        const FrVec rho = SplitMix64(base + 2).fr_vec(n), s = SplitMix64(base + 3).fr_vec(n);
        PolynomialCommitmentCub cub = PolynomialCommitmentCub::make(be, s);
        std::shared_ptr<PcsVk> vk = make_pcs_vk(be, s);
        G1Vec comms;
        for (const DevPtr &t : tables) comms.push_back(commit(be, cub.mature(), t, N));
        std::vector<Claim> claims = evaluate_claims(be, tables, N, pts);

        auto t0 = std::chrono::steady_clock::now();
        BatchOpenProof proof = batch_open_prove(be, cub.mature(), tables, N, claims, alpha, rho);
        const double tp = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        const std::string dg = proof_digest(proof);
        if (brk >= 0) claims[(size_t)brk].value += Fr::one();
        if (brk_open) {  // proof point n/2 + g1: still on the curve and in the subgroup
            uint64_t g1a[12];
            be.check(zk_srs_download(be.handle(), cub.mature()[0]->handle(), g1a));
            G1 g1{};
            std::memcpy(g1.data(), g1a, 96);
            std::memcpy(g1.data() + 12, Fq::one().v, 48);
            G1 &pt = proof.opening[n / 2];
            pt = be.g1_lincomb_batch(G1Vec{pt, g1}, FrVec{Fr{{1, 0, 0, 0}}, Fr{{1, 0, 0, 0}}}, 1)[0];
        }
        t0 = std::chrono::steady_clock::now();
        Fr y = Fr::zero();
        const unsigned bad = failed_checks(J, claims, proof, alpha, rho, &y);
        const bool open_ok = bad == 0 && verify_opening(be, *vk, comms, claims, proof, alpha, rho, y);
        const double tv = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        const bool ok = bad == 0 && open_ok;
        if (bad & 1u) std::printf("malformed proof record\n");
        std::printf("check 1 (round chain from S): %s\n", bad ? "failed" : "ok");
        std::printf("check 2+3 (C_g, one opening, device pairing): %s\n", bad ? "not reached" : (open_ok ? "ok" : "failed"));
        std::printf("batch_open_check n=%zu seed=%llu tables=%zu claims=%zu: %s\n", n, (unsigned long long)seed, J, K, ok ? "accept" : "reject");
        std::printf("prove %.3f ms  verify %.3f ms\n", tp * 1e3, tv * 1e3);
        if (digest) std::printf("proof sha256 %s\n", dg.c_str());
        return ok ? 0 : 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "batch_open_check: %s\n", e.what());
        return 2;
    }
}
