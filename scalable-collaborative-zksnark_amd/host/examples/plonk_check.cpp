// plonk_check -- one HyperPlonk proof of one circuit on the compiled host (zkhost/plonk.hpp): the test circuit of
// zkhip.plonk.sample_circuit (the same SplitMix64 streams, so the same tables for one seed), preprocessed, proved with every challenge
// drawn from the device transcript and verified by replaying the schedule on the host transcript.  One digest for one seed across the
// two hosts (zkhip.plonk.proof_digest).
//
//     bin/plonk_check --mu M [--seed S] [--gate wide] [--witness] [--lookup | --lookup-fn [--find] [--break-lookup K]] [--break-gate K | --break-wire K | --bad-input | --break K|all]
//                     [--circuit-only | --sample-only [--time-sample R]] [--bytes [--dump-proof FILE] [--torsion K]]
//                     (with --bytes: [--dump-vk FILE] [--dump-public FILE] [--vk-torsion K])
//     bin/plonk_check --g1check-time K [--reps R] | --g2check-time K [--reps R] | --vk-vectors
//     bin/plonk_check --verify-files VK PROOF PUBLIC [--host-checks]
//     bin/plonk_check --mu M [--seed S] [--gate wide] [--lookup] --verify-many K [--break-one J]
//
// --verify-many K verifies K proofs under ONE key with ONE pairing check (plonk_verify_many: zk_pcs_verify_agg).  The key, and with it the
// SRS, is the one of seed S -- the aggregate needs one set of G2 keys, and every seed has its own trapdoor -- and proof k is a proof of
// that circuit for the public inputs of seed S + k: proof 0 from the sampler's wires, the others from wires the device generates
// (plonk_witness).  With --lookup the proof of seed S is repeated K times instead (the sampler's lookup rows must hit the table; the
// aggregate does not care).  --break-one J moves a point of proof J's first opening (opening[0] = opening[last]): its field checks hold,
// its pairing does not, the aggregate rejects and the one-by-one pass names it.  Prints one digest per proof and the line
// "verify-many K=.. verdicts 1,0,.. weights sha256 .." -- the verdicts and the SHA-256 of the weights zk_pcs_agg_weights derives from the
// aggregate's input arrays (count x 2 little-endian u64; computed on the host beside the call, which derives the same bits itself), identical to the Python host's for the same arguments (tests/test_host_plonk_agg.py).  Exit 0 when every verdict is 1.
// --bytes proves, encodes the record (zkhost/proof_io.hpp: the byte format of zkhip/proof_io.py) and verifies THE BYTES with verify_bytes:
// one device call validates every G1 point (canonical encoding, on the curve, in the prime-order subgroup) before plonk_verify runs.  Prints
// the SHA-256 of the bytes -- one digest for one seed in both hosts -- and the verdict; --dump-proof FILE writes the bytes.  --torsion K adds
// a point of order 3 to point K of the encoding (K counts the G1 points in the order of the bytes) before verifying: the point stays on the
// curve and leaves G1, and the refusal names it ("refused: opening point 7 of v_batch: not in the subgroup", exit 1).
// --bytes also encodes the verifying key (zkhost/vk_io.hpp: the byte format of zkhip/vk_io.py, the raw G2 keys in it) and prints its SHA-256
// -- one digest for one seed in both hosts; --dump-vk FILE and --dump-public FILE write the key and the public inputs (l canonical 32-byte
// Fr) beside --dump-proof.  --vk-torsion K adds a point of order 13 to G2 key K of the key's encoding and reads it back: the point stays on
// the twist and leaves G2, and the refusal names it ("refused: G2 key 3: not in the subgroup", exit 1).
// --verify-files VK PROOF PUBLIC verifies from three files in a process that never preprocesses: the key's points are validated on the device
// (--host-checks: by the serial rules), the pairing keys rebuilt, then verify_bytes.  Prints the SHA-256 of each file and "verdict accepted"
// (exit 0), "verdict rejected" (1) or "verdict refused: <cause>" (2): the lines of tools/plonk_verify.py.
// --vk-vectors needs no GPU: the encoding of a synthetic key (commitments (3 + j) G1, keys (5 + 7 j) G2, mu = 4, l = 2) for both gate kinds
// with and without a lookup, read back by the serial rules, and the refusal of key 3 plus a point of order 13; one line each.
// --g2check-time K needs no GPU: g2_decompress_check_host on G2, 2 G2, .., K G2, as --g1check-time.
// --g1check-time K needs no GPU: the host rule (g1_decompress_check_host, serial big integers) on the K points G, 2G, .., KG, warm-up 3,
// the median of R (default 20) calls, one line in ms -- the compiled host's column of tools/g1check_time.py.
// --lookup proves the test circuit with lookup rows (zkhip.plonk.sample_circuit_lookup, mu >= 3) under the label + "-lookup": three opening
// proofs.  --find (with --lookup) proves without the sample's indices: the device finds them (plonk_prove(.., kFind)); the sampler only ever
// names first occurrences, so the digest is the one without --find.  --break-lookup K moves the triple of lookup row K out of the table with gate and wiring intact: the prover refuses (exit 3, the
// device's "K of N rows" message on stderr).  --break K flips one bit of part K of the honest record before it is verified; the parts, in the
// order of the digest: 0 commitments, 1 v_commitment, 2 p_rounds, 3 g_rounds, 4 g_values, 5 p_values, 6 v_values, 7 batch.rounds,
// 8 batch.opening, 9 v_batch.rounds, 10 v_batch.opening and, with --lookup, 11 lookup.commitments, 12 lookup.rounds, 13 lookup.values,
// 14 lookup.batch.rounds, 15 lookup.batch.opening.  --break all proves once and verifies one tampered copy per part: one line each, exit 1 when
// every copy is rejected and 0 when one is accepted.
//
// --lookup-fn (with --gate wide) is --lookup on the circuit of zkhip.plonk.sample_circuit_lookup_fn instead: lookup rows with the gate switched
// off against an XOR table.  With --witness the plan is built WITH the lookup (zk_witness_plan_create_lookup) and the device takes the c of
// those rows from the table (zk_plonk_witness_lookup), from the public inputs and the sampler's free values alone; --break-lookup K (a lookup
// row with a free a) moves that value out of the table: with --witness the generator refuses, without it the prover does (exit 3).
// --witness drops the sampler's a, b, c and generates them on the device (plonk_witness: zk_witness_plan_create + zk_plonk_witness) from the
// circuit, the public inputs and -- with --lookup -- the free values of the lookup rows; the digest is the one without the flag.  Not with
// --break-gate / --break-wire, which break the sampler's wires.
// --gate wide proves the test circuit of the wide gate (zkhip.plonk.sample_circuit_wide: six selectors and a fifth-power term) instead.
// --dump-srs FILE writes the parameter set of the seed's trapdoor in the byte format of zkhip/srs_io.py (zkhost/srs_io.hpp; TEST MATERIAL: the
// seed is a known trapdoor) and prints "srs_sha256 .. bytes .." -- one digest for one seed in both hosts.  --srs FILE proves on a parameter
// set LOADED from such a file instead: validated, halved and pairing-checked on the device, cut down to mu + 1 variables, the pairing keys
// made from its G2 keys; zk_srs_powers is not called.  It prints the srs_sha256 line and then what the run without the flag prints; a file
// that is refused: "verdict refused: <cause>", exit 2 (the lines of tools/plonk_srs.py --check).
// --break-gate K adds 1 to c[K]; --break-wire K (K past the input rows) changes a[K] and recomputes c[K], so that only the copy
// constraint fails; --bad-input hands the verifier a public input the prover did not use.  The verifier rejects each.  Prints the proof
// digest and accept / reject; exit 0 on accept, 1 on reject, 2 on error (arguments are checked before any device is touched).
// Without a GPU it refuses (no CPU fallback) -- but for --circuit-only (--sample-only is the same mode), which builds the test circuit, prints
// the SHA-256 of its tables (the selectors, a, b, c, the public inputs, the trapdoor, sigma and, with --lookup, qk, t0, t1, t2, idx:
// little-endian words in that order, zkhip.plonk.circuit_digest) and exits 0 without touching a device.  --time-sample R (with that mode)
// samples 3 + R more times and prints a second line, the median of the last R calls' time in the sampler's ROW LOOP alone (the loop that
// copies a, b and computes c; no draws, no sigma): the CPU baseline of tools/witness_time.py.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "zkhost/hyperplonk.hpp"
#include "zkhost/pcs_vk.hpp"
#include "zkhost/plonk.hpp"
#include "zkhost/proof_io.hpp"
#include "zkhost/sha256.hpp"
#include "zkhost/srs_io.hpp"
#include "zkhost/vk_io.hpp"
#include <chrono>

using namespace zkhost;

static bool number(const char *s, long long &out) {
    char *end = nullptr;
    out = std::strtoll(s, &end, 10);
    return *s && end && !*end && out >= 0;
}

struct Options {
    long long mu = -1, seed = 7, break_gate = -1, break_wire = -1, break_lookup = -1, break_part = -1;
    long long time_sample = 0, torsion = -1, g1check_time = 0, reps = 20, verify_many = 0, break_one = -1;
    long long vk_torsion = -1, g2check_time = 0;
    bool bytes = false, vk_vectors = false, host_checks = false;
    std::string dump_proof, dump_vk, dump_public, files[3], dump_srs, srs;
    bool bad_input = false, wide = false, lookup = false, break_all = false, find = false, witness = false, lookup_fn = false;
};

static PlonkCircuit sample(const Options &o, bool broken) {
    if (o.lookup_fn) return sample_circuit_lookup_fn((size_t)o.mu, (uint64_t)o.seed, broken ? o.break_lookup : -1);
    if (o.lookup) return sample_circuit_lookup((size_t)o.mu, (uint64_t)o.seed, o.wide, broken ? o.break_lookup : -1);
    return (o.wide ? sample_circuit_wide : sample_circuit)((size_t)o.mu, (uint64_t)o.seed, broken ? o.break_gate : -1, broken ? o.break_wire : -1, nullptr);
}

static int circuit_only(const Options &o) {
    const PlonkCircuit c = sample(o, true);
    std::printf("circuit sha256 %s\n", circuit_digest(c).c_str());
    if (o.time_sample > 0) {
        // the sampler's row loop alone (detail::sample_loop_seconds): the median of R calls after three, one process
        std::vector<double> t;
        for (long long i = 0; i < 3 + o.time_sample; ++i) {
            sample(o, true);
            if (i >= 3) t.push_back(detail::sample_loop_seconds());
        }
        std::sort(t.begin(), t.end());
        const size_t n = t.size();
        std::printf("sample row loop seconds %.6f\n", n % 2 ? t[n / 2] : 0.5 * (t[n / 2 - 1] + t[n / 2]));
    }
    return 0;
}

// the host rule on G, 2G, .., KG: median of `reps` calls after three, ms
static int g1check_time(const Options &o) {
    const size_t k = (size_t)o.g1check_time;
    const G1Affine g = g1_deserialize_compressed((const uint8_t *)"\x97\xf1\xd3\xa7\x31\x97\xd7\x94\x26\x95\x63\x8c\x4f\xa9\xac\x0f\xc3\x68\x8c\x4f\x97\x74\xb9\x05"
                                                                   "\xa1\x4e\x3a\x3f\x17\x1b\xac\x58\x6c\x55\xe8\x3f\xf9\x7a\x1a\xef\xfb\x3a\xf0\x0a\xdb\x22\xc6\xbb");
    const detail::JacQ G{g.x, g.y, Fq::one()};
    detail::JacQ acc{Fq::one(), Fq::one(), Fq::zero()};
    Bytes enc;
    for (size_t i = 0; i < k; ++i) {
        acc = detail::jq_add(acc, G);
        const Fq zi = acc.z.inverse(), zi2 = zi * zi;
        g1_serialize_compressed(G1Affine{acc.x * zi2, acc.y * zi2 * zi, false}, enc);
    }
    G1Vec pts;
    std::vector<uint8_t> st;
    std::vector<double> t;
    for (long long i = 0; i < 3 + o.reps; ++i) {
        const auto t0 = std::chrono::steady_clock::now();
        g1_decompress_check_host(enc.data(), k, pts, st);
        if (i >= 3) t.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    bool all_ok = true;
    for (uint8_t s : st) all_ok = all_ok && s == kG1Ok;
    std::sort(t.begin(), t.end());
    const size_t n = t.size();
    Sha256 h;
    h.update(pts.data(), 144 * pts.size());
    std::printf("g1check host points %zu ms %.6f all_ok %d points_sha256 %s\n", k, n % 2 ? t[n / 2] : 0.5 * (t[n / 2 - 1] + t[n / 2]), all_ok ? 1 : 0, h.hex().c_str());
    return all_ok ? 0 : 1;
}

// ---- G2 on the host for the modes below ----
static detail::Jac2 g2_generator() {
    detail::Fq2 x{detail::fq_words(kG2Gen[0]), detail::fq_words(kG2Gen[1])}, y{detail::fq_words(kG2Gen[2]), detail::fq_words(kG2Gen[3])};
    return {x, y, detail::Fq2::one()};
}
static G2Rec g2_affine_record(const detail::Jac2 &p) {
    if (p.z.is_zero()) return G2Rec{};
    const detail::Fq2 zi = detail::fq2_inverse(p.z), zi2 = zi * zi;
    return detail::g2_record(p.x * zi2, p.y * zi2 * zi);
}
static detail::Jac2 g2_times(const detail::Jac2 &g, unsigned k) {
    detail::Jac2 acc = detail::j2_inf();
    for (unsigned i = 0; i < k; ++i) acc = detail::j2_add(acc, g);
    return acc;
}
// a point of order 13 of the twist (tests/g2check_model.py, points(1)["order13"]), compressed
static const char kOrder13[] = "950a3bc83828ad1e76601cd7f02dd2b6cf3d796cb9d253fb4890132f540cd4e032b00cb52033eb04480ae31d5cb2b53409d9acc6dfec295b33b81207e234d0806642df2fc6b3dce14c0c3ecc7380a280338c1b757d0411eaec597b1f6547a4fe";
// key K of the encoding += that point
static void add_vk_torsion(Bytes &vkb, size_t K) {
    const ProofHeader h = parse_vk(vkb);
    if (K >= h.mu + 2) throw std::invalid_argument("--vk-torsion names one of the key's " + std::to_string(h.mu + 2) + " G2 keys");
    const size_t off = kProofHeaderBytes + 48 * vk_commitment_count(h.gate, h.lookup) + 96 * K;
    uint8_t t[96];
    for (int i = 0; i < 96; ++i) t[i] = (uint8_t)std::stoul(std::string(kOrder13 + 2 * i, 2), nullptr, 16);
    detail::Fq2 x, y, tx, ty;
    bool inf = false, tinf = false;
    if (detail::g2_decode(&vkb[off], x, y, inf) || detail::g2_decode(t, tx, ty, tinf)) throw std::invalid_argument("--vk-torsion: key " + std::to_string(K) + " does not decode");
    const detail::Jac2 sum = detail::j2_add(inf ? detail::j2_inf() : detail::Jac2{x, y, detail::Fq2::one()}, detail::Jac2{tx, ty, detail::Fq2::one()});
    Bytes enc;
    g2_serialize_compressed(g2_affine_record(sum), enc);
    std::memcpy(&vkb[off], enc.data(), 96);
}
static std::string sha_hex(const Bytes &b) {
    Sha256 h;
    h.update(b.data(), b.size());
    return h.hex();
}

static int g2check_time(const Options &o) {
    const size_t k = (size_t)o.g2check_time;
    const detail::Jac2 G = g2_generator();
    detail::Jac2 acc = detail::j2_inf();
    Bytes enc;
    for (size_t i = 0; i < k; ++i) {
        acc = detail::j2_add(acc, G);
        g2_serialize_compressed(g2_affine_record(acc), enc);
    }
    std::vector<G2Rec> pts;
    std::vector<uint8_t> st;
    std::vector<double> t;
    for (long long i = 0; i < 3 + o.reps; ++i) {
        const auto t0 = std::chrono::steady_clock::now();
        g2_decompress_check_host(enc.data(), k, pts, st);
        if (i >= 3) t.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    bool all_ok = true;
    for (uint8_t s : st) all_ok = all_ok && s == kG2Ok;
    std::sort(t.begin(), t.end());
    const size_t n = t.size();
    Sha256 h;
    h.update(pts.data(), 192 * pts.size());
    std::printf("g2check host points %zu ms %.6f all_ok %d points_sha256 %s\n", k, n % 2 ? t[n / 2] : 0.5 * (t[n / 2 - 1] + t[n / 2]), all_ok ? 1 : 0, h.hex().c_str());
    return all_ok ? 0 : 1;
}

static int vk_vectors() {
    const G1Affine g = g1_deserialize_compressed((const uint8_t *)"\x97\xf1\xd3\xa7\x31\x97\xd7\x94\x26\x95\x63\x8c\x4f\xa9\xac\x0f\xc3\x68\x8c\x4f\x97\x74\xb9\x05"
                                                                   "\xa1\x4e\x3a\x3f\x17\x1b\xac\x58\x6c\x55\xe8\x3f\xf9\x7a\x1a\xef\xfb\x3a\xf0\x0a\xdb\x22\xc6\xbb");
    const detail::JacQ G1g{g.x, g.y, Fq::one()};
    const detail::Jac2 G2g = g2_generator();
    const size_t mu = 4;
    bool all = true;
    for (int kind = 0; kind < 2; ++kind)
        for (int lookup = 0; lookup < 2; ++lookup) {
            PlonkVk vk;
            vk.gate = kind ? GateKind::wide : GateKind::basic, vk.lookup = lookup != 0, vk.mu = mu, vk.l = 2;
            for (size_t j = 0; j < vk_commitment_count(vk.gate, vk.lookup); ++j) {
                detail::JacQ acc{Fq::one(), Fq::one(), Fq::zero()};
                for (size_t i = 0; i < 3 + j; ++i) acc = detail::jq_add(acc, G1g);
                G1 w{};
                std::memcpy(&w[0], acc.x.v, 48), std::memcpy(&w[6], acc.y.v, 48), std::memcpy(&w[12], acc.z.v, 48);  // (any representative)
                vk.commitments.push_back(w);
            }
            for (size_t j = 0; j < mu + 2; ++j) vk.g2.push_back(g2_affine_record(g2_times(G2g, 5 + 7 * (unsigned)j)));
            Bytes data = vk_to_bytes(vk);
            const PlonkVk back = vk_from_bytes(nullptr, data, true);
            const bool same = vk_to_bytes(back) == data && back.g2 == vk.g2 && data.size() == vk_size(vk.gate, vk.lookup, mu);
            add_vk_torsion(data, 3);
            std::string why = "accepted";
            try {
                vk_from_bytes(nullptr, data, true);
            } catch (const std::invalid_argument &e) {
                why = e.what();
            }
            std::printf("vk vectors gate=%s lookup=%d bytes %zu sha256 %s round_trip %d torsion: %s\n", kind ? "wide" : "basic", lookup, data.size(),
                        sha_hex(vk_to_bytes(vk)).c_str(), same ? 1 : 0, why.c_str());
            all = all && same && why == "G2 key 3: not in the subgroup";
        }
    return all ? 0 : 1;
}

// --verify-files: no preprocess in this process
static int verify_from_files(const Options &o) {
    Bytes data[3];
    const char *names[3] = {"vk", "proof", "public"};
    for (int i = 0; i < 3; ++i) {
        data[i] = detail::read_file(o.files[i]);
        std::printf("%s_sha256 %s bytes %zu\n", names[i], sha_hex(data[i]).c_str(), data[i].size());
    }
    Ctx be(0);
    try {
        std::string why;
        const bool ok = verify_files(be, data[0], data[1], data[2], o.host_checks, &why);
        std::printf(ok ? "verdict accepted\n" : "verdict rejected\n");
        return ok ? 0 : 1;
    } catch (const std::invalid_argument &e) {
        std::printf("verdict refused: %s\n", e.what());
        return 2;
    }
}

// --bytes: encode, (--torsion K: point K += a point of order 3), verify the bytes
static bool check_bytes(Ctx &be, const Options &o, const PcsVk &vk_mu, const PcsVk &vk_mu1, const PlonkVk &vk, const FrVec &pi, const PlonkProof &proof) {
    Bytes data = proof_to_bytes(proof);
    Sha256 h;
    h.update(data.data(), data.size());
    std::printf("bytes sha256 %s (%zu bytes)\n", h.hex().c_str(), data.size());
    if (!o.dump_proof.empty()) detail::write_file(o.dump_proof, data);
    Bytes vkb = vk_to_bytes(vk);
    std::printf("vk sha256 %s (%zu bytes)\n", sha_hex(vkb).c_str(), vkb.size());
    if (!o.dump_vk.empty()) detail::write_file(o.dump_vk, vkb);
    if (!o.dump_public.empty()) detail::write_file(o.dump_public, public_to_bytes(pi));
    if (o.vk_torsion >= 0) {
        add_vk_torsion(vkb, (size_t)o.vk_torsion);
        std::printf("vk-torsion: a point of order 13 added to G2 key %lld\n", o.vk_torsion);
        try {
            vk_from_bytes(&be, vkb);
        } catch (const std::invalid_argument &e) {
            std::printf("refused: %s\n", e.what());
            return false;
        }
    }
    if (o.torsion >= 0) {
        const ParsedProof pp = parse_proof(data);
        const size_t K = (size_t)o.torsion;
        if (K >= pp.point_offsets.size()) throw std::invalid_argument("--torsion names one of the encoding's " + std::to_string(pp.point_offsets.size()) + " points");
        const size_t off = pp.point_offsets[K];
        const G1Affine p = g1_deserialize_compressed(&data[off]);
        const detail::JacQ sum = detail::jq_add(p.infinity ? detail::JacQ{Fq::one(), Fq::one(), Fq::zero()} : detail::JacQ{p.x, p.y, Fq::one()},
                                                detail::JacQ{Fq::zero(), Fq::from_u64(2), Fq::one()});  // (0, 2): 0^3 + 4 = 2^2, order 3
        const Fq zi = sum.z.inverse(), zi2 = zi * zi;
        Bytes enc;
        g1_serialize_compressed(G1Affine{sum.x * zi2, sum.y * zi2 * zi, false}, enc);
        std::memcpy(&data[off], enc.data(), 48);
        std::printf("torsion: a point of order 3 added to %s\n", (pp.point_parts[K].first + "[" + std::to_string(pp.point_parts[K].second) + "]").c_str());
    }
    std::string why;
    const bool ok = verify_bytes(be, vk_mu, vk_mu1, vk, pi, data, &why);
    if (!ok) std::printf("refused: %s\n", why.c_str());
    return ok;
}

static const char *const kParts[16] = {"commitments", "v_commitment", "p_rounds", "g_rounds", "g_values", "p_values", "v_values", "batch.rounds", "batch.opening",
                                       "v_batch.rounds", "v_batch.opening", "lookup.commitments", "lookup.rounds", "lookup.values", "lookup.batch.rounds",
                                       "lookup.batch.opening"};
// one bit of the first word of part k of the record
static void flip(PlonkProof &p, int k) {
    uint64_t *w[16] = {p.commitments[0].data(), p.v_commitment.data(), p.p_rounds[0][0].v, p.g_rounds[0][0].v, p.g_values[0].v, p.p_values[0].v, p.v_values[0].v,
                       p.batch.rounds[0][0].v, p.batch.opening[0].data(), p.v_batch.rounds[0][0].v, p.v_batch.opening[0].data()};
    if (p.lookup) {
        uint64_t *l[5] = {p.l_commitments[0].data(), p.l_rounds[0][0].v, p.l_values[0].v, p.l_batch.rounds[0][0].v, p.l_batch.opening[0].data()};
        for (int j = 0; j < 5; ++j) w[11 + j] = l[j];
    }
    w[k][0] ^= 1;
}

// --verify-many K [--break-one J]: K proofs under the key of seed S, one aggregate call
static int verify_many(Ctx &be, const Options &o, const PcsVk &vk_mu, const PcsVk &vk_mu1, const PlonkVk &vk, const PlonkPk &pk, const PowersOfG &pg,
                       const PlonkCircuit &good, const PlonkProof &first) {
    const size_t K = (size_t)o.verify_many;
    std::vector<PlonkItem> items{PlonkItem{good.public_inputs, first}};
    std::shared_ptr<WitnessPlan> plan;
    for (size_t k = 1; k < K; ++k) {
        if (o.lookup) {
            items.push_back(items[0]);
            continue;
        }
        if (!plan) plan = witness_plan(be, good, false);
        Options ok = o;
        ok.seed = o.seed + (long long)k;
        const FrVec pi = sample(ok, false).public_inputs;
        const std::array<DevPtr, 3> w = plonk_witness(be, pk, *plan, pi, nullptr);
        items.push_back(PlonkItem{pi, plonk_prove(be, pg, pk, w[0], w[1], w[2], pi)});
    }
    if (o.break_one >= 0) {
        G1Vec &op = items[(size_t)o.break_one].proof.batch.opening;
        op.front() = op.back();
    }
    for (size_t k = 0; k < K; ++k) std::printf("proof %zu sha256 %s\n", k, proof_digest(items[k].proof).c_str());
    std::vector<uint64_t> rho;
    const std::vector<bool> got = plonk_verify_many(be, vk_mu, vk_mu1, vk, items, &rho);
    Sha256 h;
    h.update(rho.data(), 8 * rho.size());
    std::string verdicts;
    bool all = true;
    for (size_t k = 0; k < K; ++k) verdicts += (k ? "," : ""), verdicts += got[k] ? "1" : "0", all = all && got[k];
    std::printf("verify-many K=%zu verdicts %s weights sha256 %s\n", K, verdicts.c_str(), h.hex().c_str());
    return all ? 0 : 1;
}

static int run(const Options &o) {
    Ctx be(0);
    const size_t mu = (size_t)o.mu, N = size_t(1) << mu;
    const uint64_t seed = (uint64_t)o.seed;
    const bool wide = o.wide, bad_input = o.bad_input;
    const PlonkCircuit good = sample(o, false), c = sample(o, true);
    PolynomialCommitmentCub cub;
    std::vector<G2Rec> keys;  // the mu + 2 raw keys [g2, s_0 g2, .., s_mu g2]
    if (!o.srs.empty()) {
        // the parameter set comes from a file (zkhost/srs_io.hpp): loaded, checked on the device, cut down to mu + 1 variables; the trapdoor
        // of the seed is not used for it
        const Bytes data = detail::read_file(o.srs);
        std::printf("srs_sha256 %s bytes %zu\n", sha_hex(data).c_str(), data.size());
        try {
            auto loaded = srs_from_bytes(be, data);
            auto cut = srs_restrict(loaded.first, loaded.second, mu + 1);
            cub.powers_of_g = cut.first, keys = cut.second;
        } catch (const std::invalid_argument &e) {
            std::printf("verdict refused: %s\n", e.what());
            return 2;
        }
    } else {
        cub = PolynomialCommitmentCub::make(be, good.s);
        const std::vector<uint64_t> pg2 = powers_of_g2(be, good.s);
        keys.resize(pg2.size() / 24);
        std::memcpy(keys.data(), pg2.data(), 8 * pg2.size());
        if (!o.dump_srs.empty()) {  // the seed's parameter set as a file: TEST MATERIAL, the seed is a known trapdoor
            const Bytes data = srs_to_bytes(be, cub.mature(), pg2);
            std::printf("srs_sha256 %s bytes %zu\n", sha_hex(data).c_str(), data.size());
            detail::write_file(o.dump_srs, data);
        }
    }
    // level mu of the parameter set uses s_1 .. s_mu: its openings verify against [g2, s_1 g2, .., s_mu g2]
    std::vector<G2Rec> keys_mu{keys[0]};
    keys_mu.insert(keys_mu.end(), keys.begin() + 2, keys.end());
    std::shared_ptr<PcsVk> vk_mu1 = be.pcs_vk(nullptr, keys[0].data(), 192, keys.size()), vk_mu = be.pcs_vk(nullptr, keys_mu[0].data(), 192, keys_mu.size());
    PlonkVk vk;
    const PlonkPk pk = preprocess(be, cub.mature(), good, vk);
    if (o.bytes) vk.g2 = keys;  // the raw keys, for the key's encoding
    DevPtr idx;
    if (o.lookup && !o.find) {
        idx = be.alloc(4 * N);
        be.upload(idx, c.idx.data(), 4 * N);
    }
    PlonkProof proof;
    try {
        std::array<DevPtr, 3> w;
        if (o.witness) {
            // the sampler's a, b, c are dropped: the device generates them from the circuit, the public inputs and -- with a lookup -- the free
            // values of the lookup rows, whose a and b slots are fixed points of sigma and hold the table's u, v
            const std::shared_ptr<WitnessPlan> plan = witness_plan(be, good, o.lookup_fn);
            FrVec free;
            if (o.lookup_fn) {
                free = c.free;
            } else if (o.lookup) {
                free.assign(3 * N, Fr::zero());
                for (size_t x = 0; x < N; ++x)
                    if (!(c.qk[x] == Fr::zero())) free[x] = c.a[x], free[N + x] = c.b[x];
            }
            w = plonk_witness(be, pk, *plan, good.public_inputs, o.lookup ? &free : nullptr);
            const std::array<size_t, 3> info = plan->info();
            std::printf("witness on the device: %zu levels, %zu rows in the largest, %zu level launches\n", info[0], info[1], info[2]);
        } else {
            w = {be.to_device(c.a), be.to_device(c.b), be.to_device(c.c)};
        }
        proof = o.find ? plonk_prove(be, cub.mature(), pk, w[0], w[1], w[2], good.public_inputs, kFind) : plonk_prove(be, cub.mature(), pk, w[0], w[1], w[2], good.public_inputs, idx);
    } catch (const ZkError &e) {
        if (o.break_lookup < 0 || e.status != ZK_ERR_INVALID) throw;
        std::fprintf(stderr, "plonk_check: the prover refused: %s\n", e.what());
        return 3;
    }
    FrVec pi = good.public_inputs;
    if (bad_input) pi[1] += Fr::one();
    if (o.verify_many > 0) {
        const int rc = verify_many(be, o, *vk_mu, *vk_mu1, vk, pk, cub.mature(), good, proof);
        std::printf("plonk_check mu=%zu N=%zu l=%zu seed=%llu%s%s: %s\n", mu, N, good.l, (unsigned long long)seed, wide ? " gate=wide" : "", o.lookup ? " lookup" : "",
                    rc ? "reject" : "accept");
        return rc;
    }
    std::printf("proof sha256 %s\n", proof_digest(proof).c_str());
    bool ok = true;
    if (o.break_all) {
        const int parts = o.lookup ? 16 : 11;
        bool any = false;
        for (int k = 0; k < parts; ++k) {
            PlonkProof t = proof;
            flip(t, k);
            const bool acc = plonk_verify(be, *vk_mu, *vk_mu1, vk, pi, t);
            std::printf("break %d %s: %s\n", k, kParts[k], acc ? "accept" : "reject");
            any = any || acc;
        }
        ok = any;
    } else if (o.bytes) {
        ok = check_bytes(be, o, *vk_mu, *vk_mu1, vk, pi, proof);
    } else {
        if (o.break_part >= 0) flip(proof, (int)o.break_part);
        ok = plonk_verify(be, *vk_mu, *vk_mu1, vk, pi, proof);
    }
    std::printf("plonk_check mu=%zu N=%zu l=%zu seed=%llu%s%s: %s\n", mu, N, good.l, (unsigned long long)seed, wide ? " gate=wide" : "", o.lookup ? " lookup" : "",
                ok ? "accept" : "reject");
    return ok ? 0 : 1;
}

int main(int argc, char **argv) {
    Options o;
    long long &mu = o.mu, &seed = o.seed, &break_gate = o.break_gate, &break_wire = o.break_wire;
    bool &bad_input = o.bad_input, &wide = o.wide, only_circuit = false, usage = argc < 2;
    for (int i = 1; i < argc && !usage; ++i) {
        const std::string k = argv[i];
        if (k == "--bad-input") bad_input = true;
        else if (k == "--circuit-only" || k == "--sample-only") only_circuit = true;
        else if (k == "--lookup") o.lookup = true;
        else if (k == "--lookup-fn") o.lookup = o.lookup_fn = true;
        else if (k == "--find") o.find = true;
        else if (k == "--witness") o.witness = true;
        else if (k == "--bytes") o.bytes = true;
        else if (k == "--vk-vectors") o.vk_vectors = true;
        else if (k == "--host-checks") o.host_checks = true;
        else if (i + 1 < argc && k == "--dump-proof") o.dump_proof = argv[++i];
        else if (i + 1 < argc && k == "--dump-vk") o.dump_vk = argv[++i];
        else if (i + 1 < argc && k == "--dump-public") o.dump_public = argv[++i];
        else if (i + 1 < argc && k == "--dump-srs") o.dump_srs = argv[++i];
        else if (i + 1 < argc && k == "--srs") o.srs = argv[++i];
        else if (i + 3 < argc && k == "--verify-files") o.files[0] = argv[i + 1], o.files[1] = argv[i + 2], o.files[2] = argv[i + 3], i += 3;
        else if (i + 1 < argc && k == "--vk-torsion") usage = !number(argv[++i], o.vk_torsion);
        else if (i + 1 < argc && k == "--g2check-time") usage = !number(argv[++i], o.g2check_time) || o.g2check_time < 1;
        else if (i + 1 < argc && k == "--torsion") usage = !number(argv[++i], o.torsion);
        else if (i + 1 < argc && k == "--g1check-time") usage = !number(argv[++i], o.g1check_time) || o.g1check_time < 1;
        else if (i + 1 < argc && k == "--verify-many") usage = !number(argv[++i], o.verify_many) || o.verify_many < 1 || o.verify_many > 256;
        else if (i + 1 < argc && k == "--break-one") usage = !number(argv[++i], o.break_one);
        else if (i + 1 < argc && k == "--reps") usage = !number(argv[++i], o.reps) || o.reps < 1;
        else if (i + 1 < argc && k == "--time-sample") usage = !number(argv[++i], o.time_sample) || o.time_sample < 1;
        else if (i + 1 < argc && k == "--break-lookup") usage = !number(argv[++i], o.break_lookup);
        else if (i + 1 < argc && k == "--break" && !std::strcmp(argv[i + 1], "all")) o.break_all = true, ++i;
        else if (i + 1 < argc && k == "--break") usage = !number(argv[++i], o.break_part);
        else if (i + 1 < argc && k == "--gate") usage = std::strcmp(argv[++i], "wide") != 0, wide = true;
        else if (i + 1 < argc && k == "--mu") usage = !number(argv[++i], mu);
        else if (i + 1 < argc && k == "--seed") usage = !number(argv[++i], seed);
        else if (i + 1 < argc && k == "--break-gate") usage = !number(argv[++i], break_gate);
        else if (i + 1 < argc && k == "--break-wire") usage = !number(argv[++i], break_wire);
        else usage = true;
    }
    const bool tamper = o.break_all || o.break_part >= 0;
    if (o.g1check_time > 0 && !usage && mu < 0 && argc <= 5) {
        try {
            return g1check_time(o);
        } catch (const std::exception &e) {
            std::fprintf(stderr, "plonk_check: %s\n", e.what());
            return 2;
        }
    }
    if ((o.g2check_time > 0 || o.vk_vectors) && !usage && mu < 0 && argc <= 5 && !(o.g2check_time > 0 && o.vk_vectors)) {
        try {
            return o.vk_vectors ? (argc == 2 ? vk_vectors() : 2) : g2check_time(o);
        } catch (const std::exception &e) {
            std::fprintf(stderr, "plonk_check: %s\n", e.what());
            return 2;
        }
    }
    if (!o.files[0].empty() && !usage && mu < 0 && argc == 5 + (o.host_checks ? 1 : 0)) {
        if (zk_device_count() <= 0) {
            std::fprintf(stderr, "plonk_check: no GPU visible -- this host has no CPU fallback\n");
            return 2;
        }
        try {
            return verify_from_files(o);
        } catch (const std::exception &e) {
            std::fprintf(stderr, "plonk_check: %s\n", e.what());
            return 2;
        }
    }
    usage = usage || o.g2check_time > 0 || o.vk_vectors || !o.files[0].empty() || o.host_checks || ((o.vk_torsion >= 0 || !o.dump_vk.empty() || !o.dump_public.empty()) && !o.bytes);
    usage = usage || (o.break_one >= 0 && o.break_one >= o.verify_many) ||
            (o.verify_many > 0 && (o.bytes || tamper || bad_input || o.witness || o.find || o.lookup_fn || break_gate >= 0 || break_wire >= 0 || o.break_lookup >= 0 || only_circuit));
    usage = usage || (!o.dump_srs.empty() && !o.srs.empty()) || ((!o.dump_srs.empty() || !o.srs.empty()) && (only_circuit || o.verify_many > 0));
    usage = usage || o.g1check_time > 0 || ((o.torsion >= 0 || !o.dump_proof.empty()) && !o.bytes) || (o.bytes && tamper);
    if (usage || mu < 0 || (break_gate >= 0) + (break_wire >= 0) + (bad_input ? 1 : 0) + (o.break_lookup >= 0) + (tamper ? 1 : 0) > 1 ||
        (o.break_all && o.break_part >= 0) || (o.break_lookup >= 0 && !o.lookup) || (o.find && !o.lookup) || (o.lookup && (break_gate >= 0 || break_wire >= 0)) ||
        (o.witness && (break_gate >= 0 || break_wire >= 0)) || (o.time_sample > 0 && !only_circuit) || (o.lookup_fn && (!wide || o.time_sample > 0))) {
        std::fprintf(stderr, "usage: plonk_check --mu M [--seed S] [--gate wide] [--witness] [--lookup | --gate wide --lookup-fn [--find] [--break-lookup K]] [--break-gate K | --break-wire K | --bad-input | --break K|all] [--circuit-only | --sample-only [--time-sample R]] [--bytes [--dump-proof FILE] [--torsion K] [--dump-vk FILE] [--dump-public FILE] [--vk-torsion K]] [--dump-srs FILE | --srs FILE] | --verify-many K [--break-one J] | --g1check-time K [--reps R] | --g2check-time K [--reps R] | --vk-vectors | --verify-files VK PROOF PUBLIC [--host-checks]\n");
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
    if (o.lookup && mu < 3) {
        std::fprintf(stderr, "plonk_check: --lookup needs --mu >= 3\n");
        return 2;
    }
    if (o.break_part >= (o.lookup ? 16 : 11) || o.break_lookup >= N) {
        std::fprintf(stderr, "plonk_check: --break names one of the record's %d parts, --break-lookup a row below 2^mu\n", o.lookup ? 16 : 11);
        return 2;
    }
    try {
        if (only_circuit) return circuit_only(o);
    } catch (const std::exception &e) {  // --break-lookup on a row that is no lookup row
        std::fprintf(stderr, "plonk_check: %s\n", e.what());
        return 2;
    }
    int ngpu = zk_device_count();
    if (ngpu <= 0) {
        std::fprintf(stderr, "plonk_check: no GPU visible -- this host has no CPU fallback (zk_device_count = %d)\n", ngpu);
        return 2;
    }
    try {
        return run(o);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "plonk_check: %s\n", e.what());
        return 2;
    }
}
