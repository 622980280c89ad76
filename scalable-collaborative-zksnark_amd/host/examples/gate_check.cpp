// gate_check -- the gate identity proved and verified end to end on the compiled host (zkhost/zerocheck.hpp): a satisfied circuit
// from SplitMix64 (a, b, q1, q2, in uniform, c = q1 (a + b) + q2 a b + in by the element-wise kernels), a structured parameter
// set (PolynomialCommitmentCub::new, dpoly_comm.rs:37-67) with its powers_of_g2, the eq table and the degree-4 gate sumcheck
// (zk_eq_table, zk_sumcheck_gate -- the virtual circuit hyperplonk.rs:66-93 simulates), six openings, and the verifier with ONE
// zk_pcs_verify_batch call.  The same circuit, proof record and digest as zkhip/zerocheck.py (tools/gate_time.py --digest).
//
//     bin/gate_check [--n N] [--seed S] [--break-gate K] [--break-opening J] [--digest]
//
// --break-gate K adds 1 to c[K] (the field checks reject: the claimed sum is eq(tau, K) != 0); --break-opening J replaces one point of
// the opening proof of table J (0 .. 5: a, b, c, in, q1, q2) by another curve point AFTER proving (the field checks pass, the
// pairing of zk_pcs_verify_batch rejects).  Prints the verdict of the field checks, accept / reject and the three times; exit 0 on accept, 1 on reject, 2 on error.  Without a GPU it refuses (no CPU fallback).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "sha256.hpp"
#include "zkhost/hyperplonk.hpp"
#include "zkhost/pcs_vk.hpp"
#include "zkhost/zerocheck.hpp"

using namespace zkhost;

static const uint64_t kCircuitSeed = 0x6A7E0000;  // zkhip/zerocheck.py CIRCUIT_SEED

// SHA-256 over the record's words: rounds, then per opening commitment | value | opening proof (zkhip.zerocheck.proof_digest)
static std::string proof_digest(const GateProof &p) {
    Sha256 h;
    for (auto &r : p.rounds) h.update(r.data(), 5 * 32);
    for (auto &o : p.openings) h.update(o.commitment.data(), 144), h.update(o.value.v, 32), h.update(o.proof.data(), 144 * o.proof.size());
    return h.hex();
}

int main(int argc, char **argv) {
    size_t n = 12;
    uint64_t seed = 7;
    long long brk = -1, brk_open = -1;
    bool digest = false;
    for (int i = 1; i < argc; ++i) {
        std::string k = argv[i];
        if (k == "--digest") digest = true;
        else if (i + 1 < argc && k == "--n") n = std::strtoull(argv[++i], nullptr, 10);
        else if (i + 1 < argc && k == "--seed") seed = std::strtoull(argv[++i], nullptr, 10);
        else if (i + 1 < argc && k == "--break-gate") brk = std::strtoll(argv[++i], nullptr, 10);
        else if (i + 1 < argc && k == "--break-opening") brk_open = std::strtoll(argv[++i], nullptr, 10);
        else {
            std::fprintf(stderr, "usage: gate_check [--n N] [--seed S] [--break-gate K] [--break-opening J] [--digest]\n");
            return 2;
        }
    }
    int ngpu = zk_device_count();
    if (ngpu <= 0) {
        std::fprintf(stderr, "gate_check: no GPU visible -- this host has no CPU fallback (zk_device_count = %d)\n", ngpu);
        return 2;
    }
    if (n < 1 || n > 26 || (brk >= 0 && (size_t)brk >= (size_t(1) << n)) || brk_open > 5) {
        std::fprintf(stderr, "gate_check: --n must be in [1, 26], --break-gate below 2^n, --break-opening in [0, 5]\n");
        return 2;
    }
    try {
        Ctx be(0);
        const size_t len = size_t(1) << n;
        const uint64_t base = kCircuitSeed + 1000 * seed;
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
        const FrVec tau = SplitMix64(base + 6).fr_vec(n), chal = SplitMix64(base + 7).fr_vec(n), s = SplitMix64(base + 8).fr_vec(n);
        PolynomialCommitmentCub cub = PolynomialCommitmentCub::make(be, s);

        std::shared_ptr<PcsVk> vk = make_pcs_vk(be, s);  // powers_of_g2 = [g2, s_0 g2, ..., s_{n-1} g2] (dpoly_comm.rs:59-62)

        double sec[2] = {0, 0};
        GateProof proof = gate_zerocheck_prove(be, cub.mature(), t, tau, chal, nullptr, sec);
        if (brk_open >= 0) {  // proof point n/2 of that opening + g1: still on the curve and in the subgroup
            uint64_t g1a[12];
            be.check(zk_srs_download(be.handle(), cub.mature()[0]->handle(), g1a));
            G1 g1{};
            std::memcpy(g1.data(), g1a, 96);
            std::memcpy(g1.data() + 12, Fq::one().v, 48);
            G1 &pt = proof.openings[(size_t)brk_open].proof[n / 2];
            pt = be.g1_lincomb_batch(G1Vec{pt, g1}, FrVec{Fr{{1, 0, 0, 0}}, Fr{{1, 0, 0, 0}}}, 1)[0];
        }
        std::printf("field checks (rounds, final identity): %s\n", verify_rounds(proof, tau, chal) ? "ok" : "failed");
        auto t0 = std::chrono::steady_clock::now();
        const bool ok = gate_zerocheck_verify(be, *vk, proof, tau, chal);
        const double tv = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        std::printf("gate_check n=%zu seed=%llu: %s\n", n, (unsigned long long)seed, ok ? "accept" : "reject");
        std::printf("eq_table %.3f ms  sumcheck_gate %.3f ms  verify %.3f ms\n", sec[0] * 1e3, sec[1] * 1e3, tv * 1e3);
        if (digest) std::printf("proof sha256 %s\n", proof_digest(proof).c_str());
        return ok ? 0 : 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "gate_check: %s\n", e.what());
        return 2;
    }
}
