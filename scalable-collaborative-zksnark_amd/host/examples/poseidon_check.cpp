// "I know a leaf and a path to this public root", end to end in the compiled host -- the mirror of tools/poseidon_merkle.py, flag for flag and
// line for line:
//     bin/poseidon_check --depth D [--seed S] [--break bit|sibling|root] [--sample-only]
// A tree of 2^D SplitMix64(S) leaves on the device (zk_poseidon_merkle), the path of leaf S mod 2^D, poseidon_merkle_circuit(D), then
// witness_plan -> plonk_witness -> preprocess -> plonk_prove -> proof bytes -> verify_bytes.  Prints
//     circuit sha256 <built_circuit_digest>
//     root <64 hex digits of the canonical integer>
//     proof sha256 <proof_digest>
//     verdict accept | reject             (or:  refused: <the library's message>  when the witness generator refuses the path; exit 1)
// The SRS trapdoor is SplitMix64(S + 1), mu + 1 elements.  --sample-only: the circuit digest and the root by the host rule
// (poseidon_merkle_host), without a device.  --time-host K: the serial host rule alone on K states / a tree of K leaves, milliseconds
// (the CPU column of tools/poseidon_time.py).
// --update COUNT: the state transition instead -- COUNT writes (leaf (S + 5k) mod 2^D takes SplitMix64(S + 2)[k]) applied one after another to the
// device tree (poseidon_update), each path by Ctx::poseidon_merkle_paths, then poseidon_merkle_update_circuit(D, COUNT); prints circuit sha256 /
// old root / new root / proof sha256 / verdict; --break leaf alters the first write's old leaf; --sample-only: the first three lines by the host rules.
// --transfer [--bits B --amount A]: a proved transfer instead -- the leaves are BALANCES, leaf k holds 2^(B-2) + (13 S + 41 k) mod 2^(B-2) (4 <= B <= 64);
// leaf S mod 2^D pays A (default 5) to leaf (S + 1) mod 2^D: two writes one after another on the device tree, each path taken from the tree before its
// write, then poseidon_merkle_transfer_circuit(D, B), whose inverses and bits the witness generator makes on the device.  Prints circuit sha256 /
// roots <old> <new> / proof sha256 / verdict; --break sibling alters the sender's leaf-level sibling; --sample-only: the first two lines by the host rules.
// --schnorr: "I know a signature under this public key on this public message" -- sk = S + 1, m = S + 1000, jubjub_sign_host, the native check on the
// device (Ctx::schnorr_verify must say 0), then jubjub_schnorr_circuit through the pipeline.  Prints circuit sha256 / signature sha256 (of
// R.x || R.y || s) / proof sha256 / verdict; --sample-only: the first two lines, without a device.
// --signed-transfer [--bits B --amount A --forge]: the transfer on leaves hash2(hash2(PK.x, PK.y), balance) -- leaf k belongs to the secret key
// S + 1 + k, balances as for --transfer; the sender signs m = hash2(hash2(receiver key hash, A), old root); --forge signs with the RECEIVER's key.
// Prints circuit sha256 / signature sha256 / roots <old> <new> / proof sha256 / verdict; --sample-only: the first three lines by the host rules.
// --time-schnorr K: jubjub_verify_host on K signatures, serial, milliseconds (the CPU column of tools/jubjub_time.py).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "zkhost/hyperplonk.hpp"
#include "zkhost/jubjub.hpp"
#include "zkhost/pcs_vk.hpp"
#include "zkhost/poseidon.hpp"
#include "zkhost/proof_io.hpp"

using namespace zkhost;

static std::string hex_of(const Fr &x) {
    const Fr c = x.to_canonical();
    char buf[65];
    for (int i = 0; i < 4; ++i) std::snprintf(buf + 16 * i, 17, "%016llx", (unsigned long long)c.v[3 - i]);
    return buf;
}

static int time_host(size_t k) {
    const FrVec in = SplitMix64(1).fr_vec(3 * k);
    auto t0 = std::chrono::steady_clock::now();
    Fr acc = Fr::zero();
    for (size_t i = 0; i < k; ++i) acc += poseidon_permute_host({in[3 * i], in[3 * i + 1], in[3 * i + 2]})[0];
    auto t1 = std::chrono::steady_clock::now();
    std::printf("host permute n=%zu ms %.3f (check %016llx)\n", k, std::chrono::duration<double, std::milli>(t1 - t0).count(), (unsigned long long)acc.v[0]);
    if (!(k & (k - 1))) {
        const FrVec leaves(in.begin(), in.begin() + k);
        t0 = std::chrono::steady_clock::now();
        const FrVec tree = poseidon_merkle_host(leaves);
        t1 = std::chrono::steady_clock::now();
        std::printf("host merkle n=%zu ms %.3f (root %s)\n", k, std::chrono::duration<double, std::milli>(t1 - t0).count(), hex_of(tree.back()).c_str());
    }
    return 0;
}

// --update COUNT: COUNT writes one after another on the device tree, each path taken from the tree before its write, then
// poseidon_merkle_update_circuit(D, COUNT) through the pipeline (tools/poseidon_merkle.py `update`, line for line)
static int update_check(size_t depth, uint64_t seed, size_t count, const std::string &brk, bool sample_only) {
    const size_t n = size_t(1) << depth;
    CircuitLayout layout;
    MerkleUpdateVars v;
    const PlonkCircuit circuit = poseidon_merkle_update_circuit(depth, count, layout, v);
    const FrVec leaves = SplitMix64(seed).fr_vec(n), fresh = SplitMix64(seed + 2).fr_vec(count);
    std::vector<std::pair<uint64_t, Fr>> writes;
    for (size_t k = 0; k < count; ++k) writes.push_back({(seed + 5 * k) % n, fresh[k]});
    std::printf("circuit sha256 %s\n", built_circuit_digest(circuit).c_str());
    if (sample_only) {
        FrVec tree = poseidon_merkle_host(leaves);
        std::printf("old root %s\n", hex_of(tree.back()).c_str());
        for (const auto &w : writes) tree = poseidon_update_host(tree, n, {w});
        std::printf("new root %s\n", hex_of(tree.back()).c_str());
        return 0;
    }
    Ctx be(0);
    const std::shared_ptr<PoseidonParams> pp = poseidon_params(be);
    const DevPtr tree = be.poseidon_merkle(*pp, be.to_device(leaves), n);
    const Fr old_root = be.to_host(tree.fr(2 * n - 2), 1)[0];
    std::printf("old root %s\n", hex_of(old_root).c_str());
    std::vector<MerkleUpdateStep> steps;
    for (const auto &w : writes) {
        MerkleUpdateStep s;
        s.old_leaf = be.to_host(tree.fr((size_t)w.first), 1)[0];
        s.new_leaf = w.second;
        s.siblings = be.to_host(be.poseidon_merkle_paths(tree, n, {w.first}), depth);
        for (size_t j = 0; j < depth; ++j) s.bits.push_back((w.first >> j) & 1);
        steps.push_back(s);
        poseidon_update(be, *pp, tree, n, {w});
    }
    const Fr new_root = be.to_host(tree.fr(2 * n - 2), 1)[0];
    std::printf("new root %s\n", hex_of(new_root).c_str());
    if (brk == "leaf") steps[0].old_leaf += Fr::one();
    if (brk == "bit") steps[0].bits[0] ^= 1;
    if (brk == "sibling") steps[0].siblings[0] += Fr::one();
    const FrVec pi{old_root, brk == "root" ? new_root + Fr::one() : new_root};
    const FrVec s = SplitMix64(seed + 1).fr_vec(circuit.mu + 1);
    const PolynomialCommitmentCub cub = PolynomialCommitmentCub::make(be, s);
    const std::vector<uint64_t> pg2 = powers_of_g2(be, s);
    std::vector<G2Rec> keys(pg2.size() / 24);
    std::memcpy(keys.data(), pg2.data(), 8 * pg2.size());
    std::vector<G2Rec> keys_mu{keys[0]};
    keys_mu.insert(keys_mu.end(), keys.begin() + 2, keys.end());
    std::shared_ptr<PcsVk> vk_mu1 = be.pcs_vk(nullptr, keys[0].data(), 192, keys.size()), vk_mu = be.pcs_vk(nullptr, keys_mu[0].data(), 192, keys_mu.size());
    PlonkVk vk;
    const PlonkPk pk = preprocess(be, cub.mature(), circuit, vk);
    const std::shared_ptr<WitnessPlan> plan = witness_plan(be, circuit);
    const FrVec free = poseidon_merkle_update_inputs(layout, v, steps);
    std::array<DevPtr, 3> w;
    try {
        w = plonk_witness(be, pk, *plan, pi, &free);
    } catch (const ZkError &e) {
        if (e.status != ZK_ERR_INVALID) throw;
        const char *msg = std::strstr(e.what(), ": ");  // past ZkError's "zkhip error -1: "
        std::printf("refused: %s\n", msg ? msg + 2 : e.what());
        return 1;
    }
    const PlonkProof proof = plonk_prove(be, cub.mature(), pk, w[0], w[1], w[2], pi, DevPtr());
    std::printf("proof sha256 %s\n", proof_digest(proof).c_str());
    const bool ok = verify_bytes(be, *vk_mu, *vk_mu1, vk, pi, proof_to_bytes(proof));
    std::printf("verdict %s\n", ok ? "accept" : "reject");
    return ok ? 0 : 1;
}

// --transfer: tools/poseidon_merkle.py `transfer`, line for line
static int transfer_check(size_t depth, uint64_t seed, size_t bits, uint64_t amount, const std::string &brk, bool sample_only) {
    const size_t n = size_t(1) << depth;
    CircuitLayout layout;
    MerkleUpdateVars v;
    Var amount_var = kNoVar;
    const PlonkCircuit circuit = poseidon_merkle_transfer_circuit(depth, bits, layout, v, amount_var);
    const uint64_t quarter = uint64_t(1) << (bits - 2);
    FrVec leaves;
    for (size_t k = 0; k < n; ++k) leaves.push_back(Fr::from_u64(quarter + (13 * seed + 41 * k) % quarter));
    const uint64_t from = seed % n, to = (seed + 1) % n;
    const Fr amt = Fr::from_u64(amount);
    std::printf("circuit sha256 %s\n", built_circuit_digest(circuit).c_str());
    if (sample_only) {
        FrVec tree = poseidon_merkle_host(leaves);
        const Fr old_root = tree.back();
        tree = poseidon_update_host(tree, n, {{from, leaves[from] - amt}});
        tree = poseidon_update_host(tree, n, {{to, leaves[to] + amt}});
        std::printf("roots %s %s\n", hex_of(old_root).c_str(), hex_of(tree.back()).c_str());
        return 0;
    }
    Ctx be(0);
    const std::shared_ptr<PoseidonParams> pp = poseidon_params(be);
    const DevPtr tree = be.poseidon_merkle(*pp, be.to_device(leaves), n);
    const Fr old_root = be.to_host(tree.fr(2 * n - 2), 1)[0];
    MerkleTransferSide side[2];
    const std::pair<uint64_t, Fr> writes[2] = {{from, leaves[from] - amt}, {to, leaves[to] + amt}};
    for (size_t k = 0; k < 2; ++k) {
        side[k].old_leaf = be.to_host(tree.fr((size_t)writes[k].first), 1)[0];
        side[k].siblings = be.to_host(be.poseidon_merkle_paths(tree, n, {writes[k].first}), depth);
        for (size_t j = 0; j < depth; ++j) side[k].bits.push_back((writes[k].first >> j) & 1);
        poseidon_update(be, *pp, tree, n, {writes[k]});
    }
    const Fr new_root = be.to_host(tree.fr(2 * n - 2), 1)[0];
    std::printf("roots %s %s\n", hex_of(old_root).c_str(), hex_of(new_root).c_str());
    if (brk == "sibling") side[0].siblings[0] += Fr::one();
    const FrVec pi{old_root, new_root};
    const FrVec s = SplitMix64(seed + 1).fr_vec(circuit.mu + 1);
    const PolynomialCommitmentCub cub = PolynomialCommitmentCub::make(be, s);
    const std::vector<uint64_t> pg2 = powers_of_g2(be, s);
    std::vector<G2Rec> keys(pg2.size() / 24);
    std::memcpy(keys.data(), pg2.data(), 8 * pg2.size());
    std::vector<G2Rec> keys_mu{keys[0]};
    keys_mu.insert(keys_mu.end(), keys.begin() + 2, keys.end());
    std::shared_ptr<PcsVk> vk_mu1 = be.pcs_vk(nullptr, keys[0].data(), 192, keys.size()), vk_mu = be.pcs_vk(nullptr, keys_mu[0].data(), 192, keys_mu.size());
    PlonkVk vk;
    const PlonkPk pk = preprocess(be, cub.mature(), circuit, vk);
    const std::shared_ptr<WitnessPlan> plan = witness_plan(be, circuit);
    const FrVec free = poseidon_merkle_transfer_inputs(layout, v, amount_var, amt, side[0], side[1]);
    std::array<DevPtr, 3> w;
    try {
        w = plonk_witness(be, pk, *plan, pi, &free);
    } catch (const ZkError &e) {
        if (e.status != ZK_ERR_INVALID) throw;
        const char *msg = std::strstr(e.what(), ": ");  // past ZkError's "zkhip error -1: "
        std::printf("refused: %s\n", msg ? msg + 2 : e.what());
        return 1;
    }
    const PlonkProof proof = plonk_prove(be, cub.mature(), pk, w[0], w[1], w[2], pi, DevPtr());
    std::printf("proof sha256 %s\n", proof_digest(proof).c_str());
    const bool ok = verify_bytes(be, *vk_mu, *vk_mu1, vk, pi, proof_to_bytes(proof));
    std::printf("verdict %s\n", ok ? "accept" : "reject");
    return ok ? 0 : 1;
}

// witness_plan -> plonk_witness -> preprocess -> plonk_prove -> proof bytes -> verify_bytes, with the two lines (or the refusal) they print
static int prove_and_verify(Ctx &be, const PlonkCircuit &circuit, const FrVec &pi, const FrVec &free, uint64_t seed) {
    const FrVec s = SplitMix64(seed + 1).fr_vec(circuit.mu + 1);
    const PolynomialCommitmentCub cub = PolynomialCommitmentCub::make(be, s);
    const std::vector<uint64_t> pg2 = powers_of_g2(be, s);
    std::vector<G2Rec> keys(pg2.size() / 24);
    std::memcpy(keys.data(), pg2.data(), 8 * pg2.size());
    std::vector<G2Rec> keys_mu{keys[0]};
    keys_mu.insert(keys_mu.end(), keys.begin() + 2, keys.end());
    std::shared_ptr<PcsVk> vk_mu1 = be.pcs_vk(nullptr, keys[0].data(), 192, keys.size()), vk_mu = be.pcs_vk(nullptr, keys_mu[0].data(), 192, keys_mu.size());
    PlonkVk vk;
    const PlonkPk pk = preprocess(be, cub.mature(), circuit, vk);
    const std::shared_ptr<WitnessPlan> plan = witness_plan(be, circuit);
    std::array<DevPtr, 3> w;
    try {
        w = plonk_witness(be, pk, *plan, pi, &free);
    } catch (const ZkError &e) {
        if (e.status != ZK_ERR_INVALID) throw;
        const char *msg = std::strstr(e.what(), ": ");  // past ZkError's "zkhip error -1: "
        std::printf("refused: %s\n", msg ? msg + 2 : e.what());
        return 1;
    }
    const PlonkProof proof = plonk_prove(be, cub.mature(), pk, w[0], w[1], w[2], pi, DevPtr());
    std::printf("proof sha256 %s\n", proof_digest(proof).c_str());
    const bool ok = verify_bytes(be, *vk_mu, *vk_mu1, vk, pi, proof_to_bytes(proof));
    std::printf("verdict %s\n", ok ? "accept" : "reject");
    return ok ? 0 : 1;
}

static int time_schnorr(size_t k) {
    std::vector<JjPoint> pks;
    std::vector<JjSignature> sigs;
    for (size_t i = 0; i < 4; ++i) {
        pks.push_back(jubjub_keygen_host({3 + i, 0, 0, 0}));
        sigs.push_back(jubjub_sign_host({3 + i, 0, 0, 0}, Fr::from_u64(1000 + i)));
    }
    const auto t0 = std::chrono::steady_clock::now();
    int bad = 0;
    for (size_t i = 0; i < k; ++i) bad += jubjub_verify_host(pks[i % 4], Fr::from_u64(1000 + i % 4), sigs[i % 4]);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    std::printf("host schnorr verify n=%zu ms %.3f (%.4f ms per signature, %d refused)\n", k, ms, ms / (double)k, bad);
    return bad ? 1 : 0;
}

// --schnorr: tools/poseidon_merkle.py `schnorr`, line for line
static int schnorr_check(uint64_t seed, bool sample_only) {
    CircuitLayout layout;
    SchnorrVars v;
    const PlonkCircuit circuit = jubjub_schnorr_circuit(layout, v);
    const JjScalar sk = {seed + 1, 0, 0, 0};
    const Fr m = Fr::from_u64(seed + 1000);
    const JjPoint pk = jubjub_keygen_host(sk);
    const JjSignature sig = jubjub_sign_host(sk, m);
    std::printf("circuit sha256 %s\n", built_circuit_digest(circuit).c_str());
    std::printf("signature sha256 %s\n", jubjub_signature_digest(sig).c_str());
    if (sample_only) return jubjub_verify_host(pk, m, sig) == 0 ? 0 : 1;
    Ctx be(0);
    const std::shared_ptr<PoseidonParams> pp = poseidon_params(be);
    Fr s_raw;
    for (size_t i = 0; i < 4; ++i) s_raw.v[i] = sig.s[i];
    const std::vector<uint32_t> st = be.schnorr_verify(*pp, be.to_device(FrVec{pk.x, pk.y}), be.to_device(FrVec{m}), be.to_device(FrVec{sig.R.x, sig.R.y, s_raw}), 1);
    if (st[0] != 0) {
        std::printf("refused: zk_schnorr_verify: status %u\n", st[0]);
        return 1;
    }
    return prove_and_verify(be, circuit, FrVec{pk.x, pk.y, m, Fr::zero()}, jubjub_schnorr_inputs(layout, v, sig), seed);
}

// --signed-transfer: tools/poseidon_merkle.py `signed_transfer`, line for line
static int signed_transfer_check(size_t depth, uint64_t seed, size_t bits, uint64_t amount, bool forge, bool sample_only) {
    const size_t n = size_t(1) << depth;
    CircuitLayout layout;
    SignedTransferVars v;
    const PlonkCircuit circuit = jubjub_merkle_signed_transfer_circuit(depth, bits, layout, v);
    const uint64_t quarter = uint64_t(1) << (bits - 2);
    std::vector<uint64_t> balances;
    std::vector<JjPoint> pks;
    FrVec keys, leaves;
    for (size_t k = 0; k < n; ++k) {
        balances.push_back(quarter + (13 * seed + 41 * k) % quarter);
        pks.push_back(jubjub_keygen_host({seed + 1 + k, 0, 0, 0}));
        keys.push_back(poseidon_hash2_host(pks[k].x, pks[k].y));
        leaves.push_back(poseidon_hash2_host(keys[k], Fr::from_u64(balances[k])));
    }
    const uint64_t from = seed % n, to = (seed + 1) % n;
    const Fr amt = Fr::from_u64(amount);
    const std::pair<uint64_t, Fr> writes[2] = {{from, poseidon_hash2_host(keys[from], Fr::from_u64(balances[from]) - amt)},
                                               {to, poseidon_hash2_host(keys[to], Fr::from_u64(balances[to]) + amt)}};
    std::printf("circuit sha256 %s\n", built_circuit_digest(circuit).c_str());
    auto sign = [&](const Fr &old_root) { return jubjub_sign_host({seed + 1 + (forge ? to : from), 0, 0, 0}, jubjub_signed_transfer_message(keys[to], amt, old_root)); };
    if (sample_only) {
        FrVec tree = poseidon_merkle_host(leaves);
        const Fr old_root = tree.back();
        std::printf("signature sha256 %s\n", jubjub_signature_digest(sign(old_root)).c_str());
        for (const auto &w : writes) tree = poseidon_update_host(tree, n, {w});
        std::printf("roots %s %s\n", hex_of(old_root).c_str(), hex_of(tree.back()).c_str());
        return 0;
    }
    Ctx be(0);
    const std::shared_ptr<PoseidonParams> pp = poseidon_params(be);
    const DevPtr tree = be.poseidon_merkle(*pp, be.to_device(leaves), n);
    const Fr old_root = be.to_host(tree.fr(2 * n - 2), 1)[0];
    const JjSignature sig = sign(old_root);
    std::printf("signature sha256 %s\n", jubjub_signature_digest(sig).c_str());
    SignedTransferSide side[2];
    for (size_t k = 0; k < 2; ++k) {
        side[k].balance = Fr::from_u64(balances[writes[k].first]);
        side[k].siblings = be.to_host(be.poseidon_merkle_paths(tree, n, {writes[k].first}), depth);
        for (size_t j = 0; j < depth; ++j) side[k].bits.push_back((writes[k].first >> j) & 1);
        poseidon_update(be, *pp, tree, n, {writes[k]});
    }
    const Fr new_root = be.to_host(tree.fr(2 * n - 2), 1)[0];
    std::printf("roots %s %s\n", hex_of(old_root).c_str(), hex_of(new_root).c_str());
    return prove_and_verify(be, circuit, FrVec{old_root, new_root}, jubjub_merkle_signed_transfer_inputs(layout, v, amt, pks[from], keys[to], sig, side[0], side[1]), seed);
}

int main(int argc, char **argv) {
    long long depth = -1, seed = 7, time_k = 0, time_s = 0, update = 0, bits = 64, amount = 5;
    std::string brk;
    bool sample_only = false, transfer = false, schnorr = false, signed_transfer = false, forge = false, usage = argc < 2;
    auto number = [](const char *s, long long &out) {
        char *end = nullptr;
        out = std::strtoll(s, &end, 10);
        return *s && end && !*end && out >= 0;
    };
    for (int i = 1; i < argc && !usage; ++i) {
        const std::string k = argv[i];
        if (k == "--sample-only") sample_only = true;
        else if (k == "--transfer") transfer = true;
        else if (k == "--schnorr") schnorr = true;
        else if (k == "--signed-transfer") signed_transfer = true;
        else if (k == "--forge") forge = true;
        else if (i + 1 < argc && k == "--time-schnorr") usage = !number(argv[++i], time_s) || time_s < 1;
        else if (i + 1 < argc && k == "--bits") usage = !number(argv[++i], bits) || bits < 4 || bits > 64;
        else if (i + 1 < argc && k == "--amount") usage = !number(argv[++i], amount);
        else if (i + 1 < argc && k == "--depth") usage = !number(argv[++i], depth) || depth < 1 || depth > 40;
        else if (i + 1 < argc && k == "--seed") usage = !number(argv[++i], seed);
        else if (i + 1 < argc && k == "--time-host") usage = !number(argv[++i], time_k) || time_k < 1;
        else if (i + 1 < argc && k == "--update") usage = !number(argv[++i], update) || update < 1;
        else if (i + 1 < argc && k == "--break") brk = argv[++i], usage = brk != "bit" && brk != "sibling" && brk != "root" && brk != "leaf";
        else usage = true;
    }
    if (brk == "leaf" && update == 0) usage = true;
    if (transfer && (update > 0 || (!brk.empty() && brk != "sibling"))) usage = true;
    if ((schnorr || signed_transfer) && (transfer || update > 0 || !brk.empty() || (schnorr && signed_transfer))) usage = true;
    if (forge && !signed_transfer) usage = true;
    if (!usage && time_k > 0 && depth < 0) return time_host((size_t)time_k);
    try {
        if (!usage && time_s > 0 && depth < 0) return time_schnorr((size_t)time_s);
        if (!usage && schnorr && time_k == 0 && time_s == 0) return schnorr_check((uint64_t)seed, sample_only);
        if (!usage && signed_transfer && depth >= 1 && time_k == 0 && time_s == 0) return signed_transfer_check((size_t)depth, (uint64_t)seed, (size_t)bits, (uint64_t)amount, forge, sample_only);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "poseidon_check: %s\n", e.what());
        return 4;
    }
    if (usage || depth < 0 || time_k > 0 || time_s > 0) {
        std::fprintf(stderr, "usage: poseidon_check --depth D [--seed S] [--update COUNT | --transfer [--bits B] [--amount A]] [--break bit|sibling|root|leaf (leaf: with --update; --transfer: sibling)] "
                             "[--sample-only] | --schnorr [--seed S] [--sample-only] | --depth D --signed-transfer [--bits B] [--amount A] [--forge] [--sample-only] | --time-host K | --time-schnorr K\n");
        return 2;
    }
    try {
        if (transfer) return transfer_check((size_t)depth, (uint64_t)seed, (size_t)bits, (uint64_t)amount, brk, sample_only);
        if (update > 0) return update_check((size_t)depth, (uint64_t)seed, (size_t)update, brk, sample_only);
        const size_t n = size_t(1) << depth, index = (size_t)seed % n;
        CircuitLayout layout;
        MerkleCircuitVars v;
        const PlonkCircuit circuit = poseidon_merkle_circuit((size_t)depth, layout, v);
        const FrVec leaves = SplitMix64((uint64_t)seed).fr_vec(n);
        std::printf("circuit sha256 %s\n", built_circuit_digest(circuit).c_str());
        if (sample_only) {
            std::printf("root %s\n", hex_of(poseidon_merkle_host(leaves).back()).c_str());
            return 0;
        }
        Ctx be(0);
        const std::shared_ptr<PoseidonParams> pp = poseidon_params(be);
        const FrVec tree = be.to_host(be.poseidon_merkle(*pp, be.to_device(leaves), n), 2 * n - 1);
        const Fr root = tree.back();
        std::printf("root %s\n", hex_of(root).c_str());
        FrVec sibs;
        std::vector<uint64_t> bits;
        poseidon_merkle_path(tree, n, index, sibs, bits);
        if (brk == "bit") bits[0] ^= 1;
        if (brk == "sibling") sibs[0] += Fr::one();
        const FrVec pi{brk == "root" ? root + Fr::one() : root};
        const FrVec s = SplitMix64((uint64_t)seed + 1).fr_vec(circuit.mu + 1);
        const PolynomialCommitmentCub cub = PolynomialCommitmentCub::make(be, s);
        const std::vector<uint64_t> pg2 = powers_of_g2(be, s);
        std::vector<G2Rec> keys(pg2.size() / 24);
        std::memcpy(keys.data(), pg2.data(), 8 * pg2.size());
        std::vector<G2Rec> keys_mu{keys[0]};
        keys_mu.insert(keys_mu.end(), keys.begin() + 2, keys.end());
        std::shared_ptr<PcsVk> vk_mu1 = be.pcs_vk(nullptr, keys[0].data(), 192, keys.size()), vk_mu = be.pcs_vk(nullptr, keys_mu[0].data(), 192, keys_mu.size());
        PlonkVk vk;
        const PlonkPk pk = preprocess(be, cub.mature(), circuit, vk);
        const std::shared_ptr<WitnessPlan> plan = witness_plan(be, circuit);
        const FrVec free = poseidon_merkle_witness_inputs(layout, v, tree[index], sibs, bits);
        std::array<DevPtr, 3> w;
        try {
            w = plonk_witness(be, pk, *plan, pi, &free);
        } catch (const ZkError &e) {
            if (e.status != ZK_ERR_INVALID) throw;
            const char *msg = std::strstr(e.what(), ": ");  // past ZkError's "zkhip error -1: "
            std::printf("refused: %s\n", msg ? msg + 2 : e.what());
            return 1;
        }
        const PlonkProof proof = plonk_prove(be, cub.mature(), pk, w[0], w[1], w[2], pi, DevPtr());
        std::printf("proof sha256 %s\n", proof_digest(proof).c_str());
        const bool ok = verify_bytes(be, *vk_mu, *vk_mu1, vk, pi, proof_to_bytes(proof));
        std::printf("verdict %s\n", ok ? "accept" : "reject");
        return ok ? 0 : 1;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "poseidon_check: %s\n", e.what());
        return 4;
    }
}
