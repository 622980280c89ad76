// Verifying-key bytes for plonk (the mirror of zkhip/vk_io.py: one layout, one set of refusals, one digest of the bytes for one seed) and
// a verifier that starts from three byte strings (vk, proof, public inputs) without a preprocess.
//
//   header, 26 bytes:  magic "ZKPLNVK" + version byte (1) | gate kind u8 (0 basic, 1 wide) | lookup u8 (0, 1) | mu u64 LE | l u64 LE
//   body: the vk's commitments in their order as 48-byte compressed G1 (5 basic, 9 wide, + 4 with a lookup), then the mu + 2 keys
//         [g2, s_0 g2, .., s_mu g2] (PlonkVk::g2) as 96-byte compressed G2.   bytes = 26 + 48 k + 96 (mu + 2).
//   A compressed G2 point (zcash / arkworks): big-endian, x.c1 in bytes 0..47, x.c0 in bytes 48..95, the top three bits of byte 0 =
//   (compressed, infinity, y is the larger of (y, -y): y.c1 decides, y.c0 when y.c1 = 0).
//
// parse_vk refuses a wrong magic or version, an unknown gate kind or lookup flag and any other length.  vk_from_bytes refuses the points
// by the rules of zk_g1_decompress_check and zk_g2_decompress_check (include/zkhip.h) -- ONE device call each, or with host = true by
// g1_decompress_check_host (proof_io.hpp) and g2_decompress_check_host below, the same rules in serial big-integer arithmetic -- and a G2
// key at infinity.  std::invalid_argument names the first bad point: "G2 key 3: not in the subgroup", "commitment 2: bad encoding".
// NOT checked: that the keys are powers of one trapdoor and belong to the prover's SRS.
#pragma once
#include <stdexcept>
#include <string>

#include "proof_io.hpp"

namespace zkhost {

enum : uint8_t { kG2Ok = 0, kG2BadEncoding = 1, kG2NotOnCurve = 2, kG2NotInSubgroup = 3 };

// ---- Fq2 = Fq[u] / (u^2 + 1) and the twist y^2 = x^3 + 4 (1 + u) in serial big integers ----
namespace detail {
struct Fq2 {
    Fq c0, c1;
    bool is_zero() const { return c0.is_zero() && c1.is_zero(); }
    bool operator==(const Fq2 &o) const { return c0 == o.c0 && c1 == o.c1; }
    friend Fq2 operator+(const Fq2 &a, const Fq2 &b) { return {a.c0 + b.c0, a.c1 + b.c1}; }
    friend Fq2 operator-(const Fq2 &a, const Fq2 &b) { return {a.c0 - b.c0, a.c1 - b.c1}; }
    friend Fq2 operator*(const Fq2 &a, const Fq2 &b) { return {a.c0 * b.c0 - a.c1 * b.c1, a.c0 * b.c1 + a.c1 * b.c0}; }
    Fq2 operator-() const { return {-c0, -c1}; }
    Fq2 conj() const { return {c0, -c1}; }
    static Fq2 one() { return {Fq::one(), Fq::zero()}; }
    static Fq2 zero() { return {Fq::zero(), Fq::zero()}; }
    Fq2 pow(const uint64_t *e) const {  // e: 6 limbs
        Fq2 r = one();
        for (int i = 383; i >= 0; --i) {
            r = r * r;
            if ((e[i / 64] >> (i % 64)) & 1) r = r * *this;
        }
        return r;
    }
};
inline Fq fq_words(const uint64_t (&w)[6]) {  // canonical little-endian limbs -> Montgomery
    Fq c;
    std::memcpy(c.v, w, 48);
    return Fq::from_canonical(c);
}
inline void q_minus(uint64_t k, int shift, uint64_t (&e)[6]) {  // (q - k) >> shift
    unsigned __int128 b = 0;
    for (int i = 0; i < 6; ++i) {
        const unsigned __int128 d = (unsigned __int128)FqParams::MOD[i] - (i ? 0 : k) - (uint64_t)b;
        e[i] = (uint64_t)d;
        b = (d >> 64) ? 1 : 0;
    }
    for (int i = 0; i < 6; ++i) e[i] = (e[i] >> shift) | (i < 5 ? e[i + 1] << (64 - shift) : 0);
}
// a root of a, or false: the two-exponentiation method of csrc/zk_g2check.hip (q = 3 mod 4), the candidate checked by squaring
inline bool fq2_sqrt(const Fq2 &a, Fq2 &y) {
    uint64_t e1[6], e2[6];
    q_minus(3, 2, e1), q_minus(1, 1, e2);
    const Fq2 a1 = a.pow(e1), x0 = a1 * a, alpha = a1 * x0;
    if (alpha == -Fq2::one()) y = Fq2{-x0.c1, x0.c0};
    else y = (alpha + Fq2::one()).pow(e2) * x0;
    return y * y == a;
}
inline Fq2 twist_rhs(const Fq2 &x) { return x * x * x + Fq2{Fq::from_u64(4), Fq::from_u64(4)}; }
inline bool fq2_larger(const Fq2 &y) { return y.c1.is_zero() ? lexicographically_largest(y.c0) : lexicographically_largest(y.c1); }

struct Jac2 {
    Fq2 x, y, z;  // z = 0: infinity
};
inline Jac2 j2_inf() { return {Fq2::one(), Fq2::one(), Fq2::zero()}; }
inline Jac2 j2_dbl(const Jac2 &p) {  // dbl-2009-l, a = 0
    if (p.z.is_zero()) return p;
    const Fq2 A = p.x * p.x, B = p.y * p.y, C = B * B, t = p.x + B;
    Fq2 D = t * t - A - C;
    D = D + D;
    const Fq2 E = A + A + A, X3 = E * E - (D + D);
    Fq2 C8 = C + C;
    C8 = C8 + C8, C8 = C8 + C8;
    const Fq2 yz = p.y * p.z;
    return {X3, E * (D - X3) - C8, yz + yz};
}
inline Jac2 j2_add(const Jac2 &p, const Jac2 &q) {  // complete: equal operands, opposite operands, infinity on either side
    if (p.z.is_zero()) return q;
    if (q.z.is_zero()) return p;
    const Fq2 Z1Z1 = p.z * p.z, Z2Z2 = q.z * q.z, U1 = p.x * Z2Z2, U2 = q.x * Z1Z1, S1 = p.y * q.z * Z2Z2, S2 = q.y * p.z * Z1Z1;
    if (U1 == U2) return S1 == S2 ? j2_dbl(p) : j2_inf();
    const Fq2 H = U2 - U1, r = S2 - S1, HH = H * H, HHH = H * HH, V = U1 * HH, X3 = r * r - HHH - (V + V);
    return {X3, r * (V - X3) - S1 * HHH, p.z * q.z * H};
}
inline Fq2 fq2_inverse(const Fq2 &a) {
    const Fq n = (a.c0 * a.c0 + a.c1 * a.c1).inverse();
    return {a.c0 * n, -(a.c1 * n)};
}
// psi(x, y) = (c_x conj(x), c_y conj(y)), c_x = (1 + u)^(-(q-1)/3), c_y = (1 + u)^(-(q-1)/2) (derived in tests/g2check_model.py)
inline const Fq2 &psi_cx() {
    static const Fq2 c = {Fq::zero(), fq_words({0x8bfd00000000aaadull, 0x409427eb4f49fffdull, 0x897d29650fb85f9bull, 0xaa0d857d89759ad4ull, 0xec02408663d4de85ull, 0x1a0111ea397fe699ull})};
    return c;
}
inline const Fq2 &psi_cy() {
    static const Fq2 c = {fq_words({0xf1ee7b04121bdea2ull, 0x304466cf3e67fa0aull, 0xef396489f61eb45eull, 0x1c3dedd930b1cf60ull, 0xe2e9c448d77a2cd9ull, 0x135203e60180a68eull}),
                          fq_words({0xc81084fbede3cc09ull, 0xee67992f72ec05f4ull, 0x77f76e17009241c5ull, 0x48395dabc2d3435eull, 0x6831e36d6bd17ffeull, 0x06af0e0437ff400bull})};
    return c;
}
// psi(P) == [x]P = -[|x|]P (Scott's test) for an affine point of the twist
inline bool g2_in_subgroup(const Fq2 &x, const Fq2 &y) {
    const uint64_t xabs = 0xd201000000010000ull;
    const Jac2 P{x, y, Fq2::one()};
    Jac2 a = P;
    for (int b = 62; b >= 0; --b) {
        a = j2_dbl(a);
        if ((xabs >> b) & 1) a = j2_add(a, P);
    }
    if (a.z.is_zero()) return false;
    const Fq2 zz = a.z * a.z;
    return psi_cx() * x.conj() * zz == a.x && (psi_cy() * y.conj() * zz * a.z + a.y).is_zero();
}
inline G2Rec g2_record(const Fq2 &x, const Fq2 &y) {
    G2Rec w{};
    std::memcpy(&w[0], x.c0.v, 48), std::memcpy(&w[6], x.c1.v, 48), std::memcpy(&w[12], y.c0.v, 48), std::memcpy(&w[18], y.c1.v, 48);
    return w;
}
inline bool g2_record_is_zero(const G2Rec &w) {
    uint64_t o = 0;
    for (uint64_t v : w) o |= v;
    return o == 0;
}
inline void g2_record_point(const G2Rec &w, Fq2 &x, Fq2 &y) {
    std::memcpy(x.c0.v, &w[0], 48), std::memcpy(x.c1.v, &w[6], 48), std::memcpy(y.c0.v, &w[12], 48), std::memcpy(y.c1.v, &w[18], 48);
}
// (status 0 / 1 / 2, the point): the rule without membership
inline uint8_t g2_decode(const uint8_t *b, Fq2 &x, Fq2 &y, bool &infinity) {
    infinity = false;
    if (!(b[0] & 0x80)) return kG2BadEncoding;
    if (b[0] & 0x40) {
        bool rest = (b[0] & 0x3F) != 0;
        for (int j = 1; j < 96; ++j) rest = rest || b[j];
        infinity = !rest;
        return rest ? kG2BadEncoding : kG2Ok;
    }
    try {
        x = Fq2{fq_from_be(b + 48, b[48]), fq_from_be(b, b[0] & 0x1F)};
    } catch (const std::invalid_argument &) {  // a coordinate >= q
        return kG2BadEncoding;
    }
    if (!fq2_sqrt(twist_rhs(x), y)) return kG2NotOnCurve;
    if (fq2_larger(y) != bool(b[0] & 0x20)) y = -y;
    return kG2Ok;
}
}  // namespace detail

inline void g2_serialize_compressed(const G2Rec &w, Bytes &out) {
    uint8_t b[96] = {0};
    if (detail::g2_record_is_zero(w)) {
        b[0] = 0xC0;
    } else {
        detail::Fq2 x, y;
        detail::g2_record_point(w, x, y);
        detail::fq_be(x.c1, b), detail::fq_be(x.c0, b + 48);
        b[0] |= 0x80;
        if (detail::fq2_larger(y)) b[0] |= 0x20;
    }
    out.insert(out.end(), b, b + 96);
}
// k compressed points -> the records and statuses of zk_g2_decompress_check, bit for bit (status 1, 2 and infinity: zero records)
inline void g2_decompress_check_host(const uint8_t *in96, size_t k, std::vector<G2Rec> &points, std::vector<uint8_t> &status) {
    points.assign(k, G2Rec{});
    status.assign(k, kG2Ok);
    for (size_t i = 0; i < k; ++i) {
        detail::Fq2 x, y;
        bool inf = false;
        status[i] = detail::g2_decode(in96 + 96 * i, x, y, inf);
        if (status[i] || inf) continue;
        points[i] = detail::g2_record(x, y);
        if (!detail::g2_in_subgroup(x, y)) status[i] = kG2NotInSubgroup;
    }
}

// ---- the layout ----
inline size_t vk_commitment_count(GateKind g, bool lookup) { return gate_desc(g).selectors + 3 + (lookup ? 4 : 0); }
inline size_t vk_size(GateKind g, bool lookup, size_t mu) { return kProofHeaderBytes + 48 * vk_commitment_count(g, lookup) + 96 * (mu + 2); }

inline Bytes vk_to_bytes(const PlonkVk &vk) {
    if (vk.g2.empty()) throw std::invalid_argument("the verifying key holds no G2 keys");
    if (vk.commitments.size() != vk_commitment_count(vk.gate, vk.lookup) || vk.g2.size() != vk.mu + 2)
        throw std::invalid_argument(std::to_string(vk.commitments.size()) + " commitments and " + std::to_string(vk.g2.size()) + " G2 keys: not a vk of this kind with mu = " + std::to_string(vk.mu));
    Bytes out;
    const char magic[8] = {'Z', 'K', 'P', 'L', 'N', 'V', 'K', (char)kProofVersion};
    out.insert(out.end(), magic, magic + 8);
    out.push_back(vk.gate == GateKind::wide ? 1 : 0);
    out.push_back(vk.lookup ? 1 : 0);
    const uint64_t ml[2] = {vk.mu, vk.l};
    out.insert(out.end(), (const uint8_t *)ml, (const uint8_t *)ml + 16);
    for (const G1 &c : vk.commitments) g1_serialize_compressed(detail::g1_affine_any(c), out);
    for (const G2Rec &k : vk.g2) g2_serialize_compressed(k, out);
    return out;
}
// the header and the length it implies; the points stay compressed at data[26 ..]
inline ProofHeader parse_vk(const Bytes &data) {
    if (data.size() < kProofHeaderBytes) throw std::invalid_argument(std::to_string(data.size()) + " bytes: shorter than the header");
    if (std::memcmp(data.data(), "ZKPLNVK", 7)) throw std::invalid_argument("wrong magic");
    if (data[7] != kProofVersion) throw std::invalid_argument("version " + std::to_string(data[7]) + ", this reader knows " + std::to_string(kProofVersion));
    if (data[8] > 1) throw std::invalid_argument("unknown gate kind " + std::to_string(data[8]));
    if (data[9] > 1) throw std::invalid_argument("lookup flag " + std::to_string(data[9]));
    uint64_t ml[2];
    std::memcpy(ml, &data[10], 16);
    if (ml[0] > 64) throw std::invalid_argument("mu = " + std::to_string(ml[0]));
    ProofHeader h{data[8] ? GateKind::wide : GateKind::basic, data[9] != 0, (size_t)ml[0], (size_t)ml[1]};
    const size_t want = vk_size(h.gate, h.lookup, h.mu);
    if (data.size() != want) throw std::invalid_argument(std::to_string(data.size()) + " bytes, the header's key has " + std::to_string(want));
    return h;
}
namespace detail {
inline std::string vk_first_bad(const std::vector<uint8_t> &cst, const std::vector<uint8_t> &kst, const std::vector<G2Rec> &keys, bool all, std::vector<std::string> *list) {
    std::string first;
    auto note = [&](const std::string &m) {
        if (first.empty()) first = m;
        if (list) list->push_back(m);
    };
    for (size_t i = 0; i < cst.size() && (all || first.empty()); ++i)
        if (cst[i]) note("commitment " + std::to_string(i) + ": " + g1_status_text(cst[i]));
    for (size_t i = 0; i < kst.size() && (all || first.empty()); ++i) {
        if (kst[i]) note("G2 key " + std::to_string(i) + ": " + g1_status_text(kst[i]));
        else if (g2_record_is_zero(keys[i])) note("G2 key " + std::to_string(i) + ": the point at infinity");
    }
    return first;
}
}  // namespace detail
// the vk of the bytes: parse_vk, ONE g1_decompress_check over the commitments, ONE g2_decompress_check over the keys (host: the serial
// rules, be unused); std::invalid_argument names the first bad point; a key at infinity is refused
inline PlonkVk vk_from_bytes(Ctx *be, const Bytes &data, bool host = false) {
    if (!be && !host) throw std::invalid_argument("vk_from_bytes needs a device context, or host = true");
    const ProofHeader h = parse_vk(data);
    const size_t k = vk_commitment_count(h.gate, h.lookup);
    const uint8_t *c48 = data.data() + kProofHeaderBytes, *k96 = c48 + 48 * k;
    PlonkVk vk;
    vk.gate = h.gate, vk.lookup = h.lookup, vk.mu = h.mu, vk.l = h.l;
    std::vector<uint8_t> cst, kst;
    if (host) g1_decompress_check_host(c48, k, vk.commitments, cst), g2_decompress_check_host(k96, h.mu + 2, vk.g2, kst);
    else be->g1_decompress_check(c48, k, vk.commitments, cst), be->g2_decompress_check(k96, h.mu + 2, vk.g2, kst);
    const std::string bad = detail::vk_first_bad(cst, kst, vk.g2, false, nullptr);
    if (!bad.empty()) throw std::invalid_argument(bad);
    return vk;
}
// the same validation for a struct: ONE g1_check and ONE g2_check call -> the messages of every bad point
inline std::vector<std::string> check_vk(Ctx &be, const PlonkVk &vk) {
    if (vk.g2.empty()) throw std::invalid_argument("the verifying key holds no G2 keys");
    std::vector<std::string> out;
    detail::vk_first_bad(be.g1_check(vk.commitments), be.g2_check(vk.g2), vk.g2, true, &out);
    return out;
}
// (vk_mu, vk_mu1) of the keys [g2, s_0 g2, .., s_mu g2]: the mu-variate tables use the last mu variables
inline std::pair<std::shared_ptr<PcsVk>, std::shared_ptr<PcsVk>> vk_pairing_keys(Ctx &be, const PlonkVk &vk) {
    std::vector<G2Rec> tail{vk.g2[0]};
    tail.insert(tail.end(), vk.g2.begin() + 2, vk.g2.end());
    return {be.pcs_vk(nullptr, tail[0].data(), 192, tail.size()), be.pcs_vk(nullptr, vk.g2[0].data(), 192, vk.g2.size())};
}

inline Bytes public_to_bytes(const FrVec &pi) {
    Bytes out;
    for (const Fr &x : pi) fr_serialize(x, out);
    return out;
}
inline FrVec public_from_bytes(const Bytes &data, size_t l) {
    if (data.size() != 32 * l) throw std::invalid_argument(std::to_string(data.size()) + " bytes of public inputs, the key has l = " + std::to_string(l) + ": " + std::to_string(32 * l));
    FrVec out(l);
    for (size_t i = 0; i < l; ++i) {
        std::memcpy(out[i].v, &data[32 * i], 32);
        if (Fr::geq_mod(out[i].v)) throw std::invalid_argument("public input " + std::to_string(i) + ": not a canonical Fr");
        out[i] = Fr::from_canonical(out[i]);
    }
    return out;
}
// the verdict on three byte strings; std::invalid_argument for a key or inputs that are refused, false for a proof that is refused or
// does not verify (*why says which)
inline bool verify_files(Ctx &be, const Bytes &vk_bytes, const Bytes &proof_bytes, const Bytes &public_bytes, bool host = false, std::string *why = nullptr) {
    const PlonkVk vk = vk_from_bytes(&be, vk_bytes, host);
    const FrVec pi = public_from_bytes(public_bytes, vk.l);
    const auto keys = vk_pairing_keys(be, vk);
    return verify_bytes(be, *keys.first, *keys.second, vk, pi, proof_bytes, why);
}

}  // namespace zkhost
