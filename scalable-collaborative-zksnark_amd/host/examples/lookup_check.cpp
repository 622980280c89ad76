// lookup_check -- the stand-alone lookup argument on the compiled host (zkhost/lookup.hpp): the sample of zkhip.lookup.sample_lookup
// (the same SplitMix64 streams, so the same table, column and indices for one seed), proved with every challenge drawn from the
// device transcript and verified by replaying the schedule on the host transcript.  One digest for one seed across the two hosts
// (zkhip.lookup.proof_digest).
//
//     bin/lookup_check --n N [--seed S] [--distinct D] [--find] [--break K | --outside] [--sample-only]
//
// --find proves without the sample's indices: the device finds them (lookup_prove(.., kFind)); the sampler only ever names first occurrences,
// so the digest is the one without --find.
// --break K flips the lowest bit of one limb of record field K after proving (0: commitments, 1: rounds, 2: values, 3: the batch
// instance's rounds, 4: its opening proof): the verifier rejects.  --outside changes one value of f so that it is not the table entry
// its index names: the prover refuses.  Prints the proof digest and accept / reject / refused; exit 0 on accept, 1 on reject or
// refusal, 2 on error (arguments are checked before any device is touched).
// Without a GPU it refuses (no CPU fallback) -- but for --sample-only, which prints the SHA-256 of the sample (t, f, idx: little-endian
// words in that order) and exits 0 without touching a device.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "zkhost/lookup.hpp"
#include "zkhost/pcs_vk.hpp"

using namespace zkhost;

static bool number(const char *s, long long &out) {
    char *end = nullptr;
    out = std::strtoll(s, &end, 10);
    return end != s && *end == 0 && out >= 0;
}

static int run(size_t n, uint64_t seed, size_t distinct, long long brk, bool outside, bool find) {
    Ctx be(0);
    const size_t N = size_t(1) << n;
    LookupSample s = sample_lookup(n, seed, distinct);
    if (outside) s.f[N - 1].v[0] ^= 1;
    const FrVec trap = sample_lookup_srs(n, seed);
    PolynomialCommitmentCub cub = PolynomialCommitmentCub::make(be, trap);
    std::shared_ptr<PcsVk> pcs_vk = make_pcs_vk(be, trap);
    const auto keys = lookup_preprocess(be, cub.mature(), be.to_device(s.t), N);
    DevPtr idx;
    if (!find) {
        idx = be.alloc(4 * N);
        be.upload(idx, s.idx.data(), 4 * N);
    }
    LookupProof proof;
    try {
        proof = find ? lookup_prove(be, cub.mature(), keys.first, be.to_device(s.f), kFind) : lookup_prove(be, cub.mature(), keys.first, be.to_device(s.f), idx);
    } catch (const ZkError &e) {
        if (e.status != ZK_ERR_INVALID) throw;
        std::printf("lookup_check n=%zu seed=%llu: refused (%s)\n", n, (unsigned long long)seed, e.what());
        return 1;
    }
    std::printf("proof sha256 %s\n", proof_digest(proof).c_str());
    switch (brk) {
    case 0: proof.commitments[2][5] ^= 1; break;
    case 1: proof.rounds[0][1].v[0] ^= 1; break;
    case 2: proof.values[4].v[0] ^= 1; break;
    case 3: proof.batch.rounds[n - 1][2].v[0] ^= 1; break;  // t2 of the last round: only the value the chain ends in moves -- the pairing sees it
    case 4: proof.batch.opening[0][3] ^= 1; break;
    default: break;
    }
    const bool ok = lookup_verify(be, *pcs_vk, keys.second, proof);
    std::printf("lookup_check n=%zu seed=%llu: %s\n", n, (unsigned long long)seed, ok ? "accept" : "reject");
    return ok ? 0 : 1;
}

int main(int argc, char **argv) {
    long long n = -1, seed = 7, distinct = 0, brk = -1;
    bool outside = false, only_sample = false, usage = false, find = false;
    for (int i = 1; i < argc && !usage; ++i) {
        const std::string k = argv[i];
        if (k == "--outside") outside = true;
        else if (k == "--sample-only") only_sample = true;
        else if (k == "--find") find = true;
        else if (i + 1 < argc && k == "--n") usage = !number(argv[++i], n);
        else if (i + 1 < argc && k == "--seed") usage = !number(argv[++i], seed);
        else if (i + 1 < argc && k == "--distinct") usage = !number(argv[++i], distinct);
        else if (i + 1 < argc && k == "--break") usage = !number(argv[++i], brk);
        else usage = true;
    }
    if (usage || n < 0 || (brk >= 0 && outside)) {
        std::fprintf(stderr, "usage: lookup_check --n N [--seed S] [--distinct D] [--find] [--break K | --outside] [--sample-only]\n");
        return 2;
    }
    if (n < 1 || n > 24 || brk > 4 || distinct > (1ll << n)) {
        std::fprintf(stderr, "lookup_check: --n must be in [1, 24], --break in [0, 4], --distinct at most 2^n\n");
        return 2;
    }
    try {
        if (only_sample) {
            std::printf("sample sha256 %s\n", sample_digest(sample_lookup((size_t)n, (uint64_t)seed, (size_t)distinct)).c_str());
            return 0;
        }
        const int ngpu = zk_device_count();
        if (ngpu <= 0) {
            std::fprintf(stderr, "lookup_check: no GPU visible -- this host has no CPU fallback (zk_device_count = %d)\n", ngpu);
            return 2;
        }
        return run((size_t)n, (uint64_t)seed, (size_t)distinct, brk, outside, find);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "lookup_check: %s\n", e.what());
        return 2;
    }
}
