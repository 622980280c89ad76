// Parameter-set bytes for plonk (the mirror of zkhip/srs_io.py: one layout, one set of refusals, one digest of the bytes for one seed): a
// structured SRS read from a file and checked on the device, so that a prover never holds the trapdoor.
//
//   header, 26 bytes:  magic "ZKPLSRS" + version byte (1) | two zero bytes | n u64 LE | eight zero bytes
//   body: the 2^n points of the TOP level L_n as 48-byte compressed G1, then the n + 1 keys [g2, s_0 g2, .., s_{n-1} g2] as 96-byte
//         compressed G2.   bytes = 26 + 48 2^n + 96 (n + 1).
//
// The lower levels are derived, L_k[j] = L_{k+1}[j] + L_{k+1}[j + 2^k] (zk_srs_halve), and e(L_{k+1}[j + 2^k], g2) = e(L_k[j], s_{n-k-1} g2)
// is checked per level under 128-bit weights hashed from the SHA-256 of the file (zk_srs_check; include/zkhip.h has the argument).
// parse_srs refuses a wrong magic or version, non-zero padding, n outside 1 .. 30 and any other length; srs_from_bytes refuses the
// points by the rules of zk_g1_decompress_check_device (infinity refused) and zk_g2_decompress_check, a key at infinity, a sum at
// infinity and a level that does not match its key.  std::invalid_argument names the cause with the words of the Python host:
// "G1 point 12345: not in the subgroup", "G2 key 3: ...", "level 7 does not match G2 key 14".
// The check proves that the G1 points are consistent with the G2 keys.  It does NOT prove that nobody knows s.
// (srs_check_host, the verdict without a device, exists in the Python host only: it needs a pairing on the host, which zkhost has not.)
#pragma once
#include <stdexcept>
#include <string>
#include <utility>

#include "dist_primitive.hpp"
#include "sha256.hpp"
#include "vk_io.hpp"

namespace zkhost {

constexpr size_t kSrsMaxN = 30;
inline size_t srs_size(size_t n) { return kProofHeaderBytes + (size_t(48) << n) + 96 * (n + 1); }

struct ParsedSrs {
    size_t n = 0;
    const uint8_t *points = nullptr;  // 2^n x 48 bytes inside the caller's buffer
    const uint8_t *keys = nullptr;    // (n + 1) x 96 bytes
};

inline std::array<uint8_t, 32> srs_file_seed(const Bytes &data) {
    std::array<uint8_t, 32> d;
    Sha256 h;
    h.update(data.data(), data.size());
    h.digest(d.data());
    return d;
}

// pg: the levels 0 .. n; pg2: the n + 1 keys as 24 Montgomery words each (pcs_vk.hpp powers_of_g2).  Only the top level and the keys are written
inline Bytes srs_to_bytes(Ctx &be, const PowersOfG &pg, const std::vector<uint64_t> &pg2) {
    const size_t n = pg.empty() ? 0 : pg.size() - 1;
    if (n < 1 || n > kSrsMaxN || pg2.size() != 24 * (n + 1) || pg[n]->len() != size_t(1) << n) throw std::invalid_argument("srs_to_bytes: not an SRS of 1 .. 30 variables with its n + 1 keys");
    Bytes out = {'Z', 'K', 'P', 'L', 'S', 'R', 'S', 1, 0, 0};
    for (int i = 0; i < 8; ++i) out.push_back((uint8_t)((uint64_t)n >> (8 * i)));
    out.insert(out.end(), 8, 0);
    const std::vector<uint8_t> recs = be.srs_download(*pg[n]);
    out.reserve(srs_size(n));
    for (size_t i = 0; i < recs.size() / 96; ++i) {
        G1Affine p;
        std::memcpy(p.x.v, &recs[96 * i], 48), std::memcpy(p.y.v, &recs[96 * i + 48], 48);
        p.infinity = p.x.is_zero() && p.y.is_zero();
        g1_serialize_compressed(p, out);
    }
    for (size_t i = 0; i <= n; ++i) {
        G2Rec w;
        std::memcpy(w.data(), &pg2[24 * i], 192);
        g2_serialize_compressed(w, out);
    }
    return out;
}

inline ParsedSrs parse_srs(const Bytes &data) {
    if (data.size() < kProofHeaderBytes) throw std::invalid_argument(std::to_string(data.size()) + " bytes: shorter than the header");
    if (std::memcmp(data.data(), "ZKPLSRS", 7)) throw std::invalid_argument("wrong magic");
    if (data[7] != 1) throw std::invalid_argument("version " + std::to_string(data[7]) + ", this reader knows 1");
    bool pad = data[8] || data[9];
    for (int i = 18; i < 26; ++i) pad = pad || data[i];
    if (pad) throw std::invalid_argument("non-zero padding in the header");
    uint64_t n = 0;
    for (int i = 0; i < 8; ++i) n |= (uint64_t)data[10 + i] << (8 * i);
    if (n < 1 || n > kSrsMaxN) throw std::invalid_argument("n = " + std::to_string(n) + ": not in 1 .. 30");
    if (data.size() != srs_size(n)) throw std::invalid_argument(std::to_string(data.size()) + " bytes, the header's parameter set has " + std::to_string(srs_size(n)));
    return {(size_t)n, data.data() + kProofHeaderBytes, data.data() + kProofHeaderBytes + (size_t(48) << n)};
}

inline std::string srs_level_message(size_t k, size_t n) { return "level " + std::to_string(k + 1) + " does not match G2 key " + std::to_string(n - k); }

// the pairing step on a loaded set: ONE zk_srs_check call -> the messages of the levels that fail, lowest first
inline std::vector<std::string> check_srs(Ctx &be, const PowersOfG &pg, const std::vector<G2Rec> &keys, const uint8_t seed[32]) {
    const size_t n = pg.size() - 1;
    if (keys.size() != n + 1) throw std::invalid_argument("check_srs: n + 1 keys for n + 1 levels");
    const std::vector<uint8_t> ok = be.srs_check(pg, keys[0].data(), 192, seed);
    std::vector<std::string> out;
    for (size_t k = 0; k < n; ++k)
        if (!ok[k]) out.push_back(srs_level_message(k, n));
    return out;
}

inline const char *srs_g1_status_text(uint8_t s) { return s == ZK_G1_INFINITY_REFUSED ? "the point at infinity" : g1_status_text(s); }

// (levels 0 .. n, the n + 1 keys): one copy of the G1 block, ONE zk_g1_decompress_check_device call, ONE zk_g2_decompress_check, zk_srs_wrap_device, n
// zk_srs_halve calls, then check_srs seeded with the SHA-256 of the file; check = false skips only that pairing step
inline std::pair<PowersOfG, std::vector<G2Rec>> srs_from_bytes(Ctx &be, const Bytes &data, bool check = true) {
    const ParsedSrs p = parse_srs(data);
    const size_t n = p.n, N = size_t(1) << n;
    DevPtr d_in = be.alloc(48 * N), d_rec = be.alloc(96 * N);
    be.upload(d_in, p.points, 48 * N);
    const std::array<uint64_t, 3> res = be.g1_decompress_check_device(d_in, N, d_rec, true);
    if (res[0]) throw std::invalid_argument("G1 point " + std::to_string(res[1]) + ": " + srs_g1_status_text((uint8_t)res[2]));
    std::vector<G2Rec> keys;
    std::vector<uint8_t> kst;
    be.g2_decompress_check(p.keys, n + 1, keys, kst);
    for (size_t i = 0; i <= n; ++i) {
        if (kst[i]) throw std::invalid_argument("G2 key " + std::to_string(i) + ": " + g1_status_text(kst[i]));
        if (detail::g2_record_is_zero(keys[i])) throw std::invalid_argument("G2 key " + std::to_string(i) + ": the point at infinity");
    }
    PowersOfG pg(n + 1);
    pg[n] = be.srs_wrap_device(d_rec, N);
    for (size_t k = n; k-- > 0;) {
        try {
            pg[k] = be.srs_halve(*pg[k + 1]);
        } catch (const ZkError &e) {
            if (e.status != ZK_ERR_INVALID) throw;
            const std::string w = e.what(), tag = "zk_srs_halve: ";
            const size_t at = w.find(tag);
            throw std::invalid_argument("level " + std::to_string(k) + ": " + (at == std::string::npos ? w : w.substr(at + tag.size())));
        }
    }
    if (check) {
        const std::vector<std::string> failed = check_srs(be, pg, keys, srs_file_seed(data).data());
        if (!failed.empty()) throw std::invalid_argument(failed[0]);
    }
    return {pg, keys};
}

// the parameter set of the LAST nvars trapdoor coordinates: levels 0 .. nvars and the keys [g2, s_{n-nvars}, .., s_{n-1}]
inline std::pair<PowersOfG, std::vector<G2Rec>> srs_restrict(const PowersOfG &pg, const std::vector<G2Rec> &keys, size_t nvars) {
    const size_t n = pg.size() - 1;
    if (nvars > n || keys.size() != n + 1) throw std::invalid_argument("srs_restrict: more variables than the parameter set has");
    std::vector<G2Rec> sub{keys[0]};
    sub.insert(sub.end(), keys.begin() + 1 + (n - nvars), keys.end());
    return {PowersOfG(pg.begin(), pg.begin() + nvars + 1), sub};
}

}  // namespace zkhost
