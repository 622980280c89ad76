// Proof bytes for plonk (the mirror of zkhip/proof_io.py: one layout, one set of refusals, one digest of the bytes for one seed):
// a PlonkProof as ONE byte string and back, with every G1 point validated on the way in.
//
//   header, 26 bytes:  magic "ZKPLONK" + version byte (1) | gate kind u8 (0 basic, 1 wide) | lookup u8 (0, 1) | mu u64 LE | l u64 LE
//   body: the record's parts in the order proof_digest walks them -- commitments (3 G1), v_commitment (1 G1), p_rounds (6 mu Fr),
//     g_rounds (E mu Fr), g_values (S + 3 Fr), p_values (6 Fr), v_values (5 Fr), batch.rounds (3 mu Fr), batch.opening (mu G1),
//     v_batch.rounds (3 (mu + 1) Fr), v_batch.opening (mu + 1 G1) and with a lookup: lookup.commitments (3 G1), lookup.rounds (4 mu Fr),
//     lookup.values (10 Fr), lookup.batch.rounds (3 mu Fr), lookup.batch.opening (mu G1).   E, S = 5, 2 (basic), 8, 6 (wide).
//   Every G1 point is the 48-byte compressed encoding of serialize.hpp, every Fr the canonical little-endian 32 bytes.
//   points k = 2 mu + 5 (+ mu + 3 with a lookup),  scalars f = (12 + E) mu + S + 17 (+ 7 mu + 10),  bytes = 26 + 48 k + 32 f.
//
// parse_proof refuses a wrong magic or version, an unknown gate kind or lookup flag, any length but the header's (trailing bytes
// included) and any Fr >= r.  The points are refused by the rule of zk_g1_decompress_check (include/zkhip.h): on the device in ONE call
// (Ctx::g1_decompress_check), or with host = true by g1_decompress_check_host below, the same rule in serial big-integer arithmetic.
// NOT checked here: the verifying key.  One that comes from outside is read and validated by vk_io.hpp.
#pragma once
#include <stdexcept>
#include <string>

#include "plonk.hpp"
#include "serialize.hpp"

namespace zkhost {

constexpr size_t kProofHeaderBytes = 26;
constexpr uint8_t kProofVersion = 1;
enum : uint8_t { kG1Ok = 0, kG1BadEncoding = 1, kG1NotOnCurve = 2, kG1NotInSubgroup = 3 };

inline size_t proof_size(GateKind g, bool lookup, size_t mu) {
    const GateDesc &d = gate_desc(g);
    const size_t k = 2 * mu + 5 + (lookup ? mu + 3 : 0), f = (12 + d.evals) * mu + d.selectors + 17 + (lookup ? 7 * mu + 10 : 0);
    return kProofHeaderBytes + 48 * k + 32 * f;
}
inline const char *g1_status_text(uint8_t s) {
    static const char *const t[4] = {"ok", "bad encoding", "x is not on the curve", "not in the subgroup"};
    return t[s & 3];
}
// e.g. "opening point 7 of v_batch: not in the subgroup"
inline std::string describe_point(const std::string &part, size_t index, uint8_t status) {
    const std::string tail = ".opening";
    const bool opening = part.size() > tail.size() && part.compare(part.size() - tail.size(), tail.size(), tail) == 0;
    return (opening ? "opening point " + std::to_string(index) + " of " + part.substr(0, part.size() - tail.size())
                    : "point " + std::to_string(index) + " of " + part) + ": " + g1_status_text(status);
}
struct BadPoint {
    std::string part;
    size_t index;
    uint8_t status;
};

// ---- the host rule: Fq big integers, one point after the other ----
namespace detail {
struct JacQ {
    Fq x, y, z;  // z = 0: infinity
};
inline JacQ jq_dbl(const JacQ &p) {  // dbl-2009-l, a = 0
    if (p.z.is_zero()) return p;
    const Fq A = p.x * p.x, B = p.y * p.y, C = B * B, t = p.x + B;
    Fq D = t * t - A - C;
    D = D + D;
    const Fq E = A + A + A, X3 = E * E - (D + D);
    Fq C8 = C + C;
    C8 = C8 + C8, C8 = C8 + C8;
    const Fq yz = p.y * p.z;
    return {X3, E * (D - X3) - C8, yz + yz};
}
inline JacQ jq_add(const JacQ &p, const JacQ &q) {  // complete: equal operands, opposite operands, infinity on either side
    if (p.z.is_zero()) return q;
    if (q.z.is_zero()) return p;
    const Fq Z1Z1 = p.z * p.z, Z2Z2 = q.z * q.z, U1 = p.x * Z2Z2, U2 = q.x * Z1Z1, S1 = p.y * q.z * Z2Z2, S2 = q.y * p.z * Z1Z1;
    if (U1 == U2) return S1 == S2 ? jq_dbl(p) : JacQ{Fq::one(), Fq::one(), Fq::zero()};
    const Fq H = U2 - U1, r = S2 - S1, HH = H * H, HHH = H * HH, V = U1 * HH, X3 = r * r - HHH - (V + V);
    return {X3, r * (V - X3) - S1 * HHH, p.z * q.z * H};
}
inline JacQ jq_mul_x(const JacQ &p) {  // [|x|]P, |x| = 0xd201000000010000
    const uint64_t x = 0xd201000000010000ull;
    JacQ acc = p;
    for (int b = 62; b >= 0; --b) {
        acc = jq_dbl(acc);
        if ((x >> b) & 1) acc = jq_add(acc, p);
    }
    return acc;
}
inline const Fq &fq_beta() {  // the cube root of unity whose endomorphism is -x^2 on G1 (csrc/zk_g1check.hip)
    static const Fq b = [] {
        Fq c;
        const uint64_t w[6] = {0x2e01fffffffefffeull, 0xde17d813620a0002ull, 0xddb3a93be6f89688ull, 0xba69c6076a0f77eaull, 0x5f19672fdf76ce51ull, 0};
        std::memcpy(c.v, w, 48);
        return Fq::from_canonical(c);
    }();
    return b;
}
// phi(P) == -[x^2]P (Scott's test) for an affine point of the curve
inline bool g1_in_subgroup(const Fq &x, const Fq &y) {
    const JacQ a = jq_mul_x(jq_mul_x(JacQ{x, y, Fq::one()}));
    if (a.z.is_zero()) return false;
    const Fq zz = a.z * a.z;
    return fq_beta() * x * zz == a.x && (y * zz * a.z + a.y).is_zero();
}
inline G1 g1_words(const Fq &x, const Fq &y, bool infinity) {  // the library's normalised Jacobian record
    G1 w{};
    const Fq one = Fq::one();
    std::memcpy(&w[0], infinity ? one.v : x.v, 48), std::memcpy(&w[6], infinity ? one.v : y.v, 48);
    if (!infinity) std::memcpy(&w[12], one.v, 48);
    return w;
}
// the affine point of an 18-word Jacobian record in any representative
inline G1Affine g1_affine_any(const G1 &p) {
    G1Affine a = g1_affine(p);
    Fq z;
    std::memcpy(z.v, &p[12], 48);
    if (a.infinity || z == Fq::one()) return a;
    const Fq zi = z.inverse(), zi2 = zi * zi;
    a.x = a.x * zi2, a.y = a.y * zi2 * zi;
    return a;
}
}  // namespace detail

// k compressed points -> the points and statuses of zk_g1_decompress_check, bit for bit (the points of status 1 and 2 are zero)
inline void g1_decompress_check_host(const uint8_t *in48, size_t k, G1Vec &points, std::vector<uint8_t> &status) {
    points.assign(k, G1{});
    status.assign(k, kG1Ok);
    for (size_t i = 0; i < k; ++i) {
        const uint8_t *b = in48 + 48 * i;
        bool rest = (b[0] & 0x1F) != 0;
        for (int j = 1; j < 48; ++j) rest = rest || b[j];
        if (!(b[0] & 0x80)) {
            status[i] = kG1BadEncoding;
        } else if (b[0] & 0x40) {
            if ((b[0] & 0x20) || rest) status[i] = kG1BadEncoding;
            else points[i] = detail::g1_words(Fq::zero(), Fq::zero(), true);
        } else {
            try {
                const G1Affine p = g1_deserialize_compressed(b);
                points[i] = detail::g1_words(p.x, p.y, false);
                if (!detail::g1_in_subgroup(p.x, p.y)) status[i] = kG1NotInSubgroup;
            } catch (const std::invalid_argument &e) {  // x >= q, or no root
                status[i] = std::string(e.what()) == "x is not on the curve" ? kG1NotOnCurve : kG1BadEncoding;
            }
        }
    }
}

// ---- the layout ----
namespace detail {
inline void proof_shape(PlonkProof &p) {  // sizes every part from gate, lookup, mu
    const GateDesc &d = gate_desc(p.gate);
    const size_t mu = p.mu;
    p.commitments.assign(3, G1{});
    p.p_rounds.assign(mu, {});
    p.g_rounds.assign(mu, FrVec(d.evals));
    p.g_values.assign(d.selectors + 3, Fr::zero()), p.p_values.assign(6, Fr::zero()), p.v_values.assign(5, Fr::zero());
    p.batch.rounds.assign(mu, {}), p.batch.opening.assign(mu, G1{});
    p.v_batch.rounds.assign(mu + 1, {}), p.v_batch.opening.assign(mu + 1, G1{});
    if (p.lookup) {
        p.l_commitments.assign(3, G1{}), p.l_rounds.assign(mu, {}), p.l_values.assign(10, Fr::zero());
        p.l_batch.rounds.assign(mu, {}), p.l_batch.opening.assign(mu, G1{});
    }
}
inline bool proof_shaped(const PlonkProof &p) {
    const GateDesc &d = gate_desc(p.gate);
    const size_t mu = p.mu;
    bool ok = p.commitments.size() == 3 && p.p_rounds.size() == mu && p.g_rounds.size() == mu && p.g_values.size() == d.selectors + 3 && p.p_values.size() == 6 &&
              p.v_values.size() == 5 && p.batch.rounds.size() == mu && p.batch.opening.size() == mu && p.v_batch.rounds.size() == mu + 1 && p.v_batch.opening.size() == mu + 1;
    for (const FrVec &r : p.g_rounds) ok = ok && r.size() == d.evals;
    if (p.lookup) ok = ok && p.l_commitments.size() == 3 && p.l_rounds.size() == mu && p.l_values.size() == 10 && p.l_batch.rounds.size() == mu && p.l_batch.opening.size() == mu;
    return ok;
}
// the parts of a shaped record in the order of the body: v.points(name, G1 *, n) / v.scalars(name, Fr *, n), one call per contiguous run
template <class P, class V>
inline void proof_walk(P &p, V &v) {
    v.points("commitments", p.commitments.data(), p.commitments.size());
    v.points("v_commitment", &p.v_commitment, 1);
    for (auto &r : p.p_rounds) v.scalars("p_rounds", r.data(), r.size());
    for (auto &r : p.g_rounds) v.scalars("g_rounds", r.data(), r.size());
    v.scalars("g_values", p.g_values.data(), p.g_values.size());
    v.scalars("p_values", p.p_values.data(), p.p_values.size());
    v.scalars("v_values", p.v_values.data(), p.v_values.size());
    for (auto &r : p.batch.rounds) v.scalars("batch.rounds", r.data(), r.size());
    v.points("batch.opening", p.batch.opening.data(), p.batch.opening.size());
    for (auto &r : p.v_batch.rounds) v.scalars("v_batch.rounds", r.data(), r.size());
    v.points("v_batch.opening", p.v_batch.opening.data(), p.v_batch.opening.size());
    if (!p.lookup) return;
    v.points("lookup.commitments", p.l_commitments.data(), p.l_commitments.size());
    for (auto &r : p.l_rounds) v.scalars("lookup.rounds", r.data(), r.size());
    v.scalars("lookup.values", p.l_values.data(), p.l_values.size());
    for (auto &r : p.l_batch.rounds) v.scalars("lookup.batch.rounds", r.data(), r.size());
    v.points("lookup.batch.opening", p.l_batch.opening.data(), p.l_batch.opening.size());
}
struct ProofWriter {
    Bytes out;
    void points(const char *, const G1 *p, size_t n) {
        for (size_t i = 0; i < n; ++i) g1_serialize_compressed(g1_affine_any(p[i]), out);
    }
    void scalars(const char *, const Fr *x, size_t n) {
        for (size_t i = 0; i < n; ++i) fr_serialize(x[i], out);
    }
};
struct PointRef {
    std::string part;
    size_t index;
    G1 *slot;
    size_t offset = 0;  // of the point's 48 bytes in the encoding (ProofReader)
};
struct ProofReader {
    const uint8_t *data = nullptr;
    size_t pos = kProofHeaderBytes;
    Bytes compressed;
    std::vector<PointRef> refs;
    std::string last;
    size_t seen = 0;
    void points(const char *name, G1 *p, size_t n) {
        for (size_t i = 0; i < n; ++i) refs.push_back({name, i, p + i, pos + 48 * i});
        compressed.insert(compressed.end(), data + pos, data + pos + 48 * n);
        pos += 48 * n;
    }
    void scalars(const char *name, Fr *x, size_t n) {
        if (last != name) last = name, seen = 0;
        for (size_t i = 0; i < n; ++i, ++seen, pos += 32) {
            std::memcpy(x[i].v, data + pos, 32);
            if (Fr::geq_mod(x[i].v)) throw std::invalid_argument("element " + std::to_string(seen) + " of " + name + ": not a canonical Fr");
            x[i] = Fr::from_canonical(x[i]);
        }
    }
};
struct PointLister {
    std::vector<PointRef> refs;
    void points(const char *name, const G1 *p, size_t n) {
        for (size_t i = 0; i < n; ++i) refs.push_back({name, i, const_cast<G1 *>(p + i), 0});
    }
    void scalars(const char *, const Fr *, size_t) {}
};
}  // namespace detail

inline Bytes proof_to_bytes(const PlonkProof &p) {
    if (!detail::proof_shaped(p)) throw std::invalid_argument("proof_to_bytes: a part of the record has the wrong length");
    detail::ProofWriter w;
    const char magic[8] = {'Z', 'K', 'P', 'L', 'O', 'N', 'K', (char)kProofVersion};
    w.out.insert(w.out.end(), magic, magic + 8);
    w.out.push_back(p.gate == GateKind::wide ? 1 : 0);
    w.out.push_back(p.lookup ? 1 : 0);
    const uint64_t ml[2] = {p.mu, p.l};
    w.out.insert(w.out.end(), (const uint8_t *)ml, (const uint8_t *)ml + 16);
    detail::proof_walk(p, w);
    return w.out;
}

struct ProofHeader {
    GateKind gate = GateKind::basic;
    bool lookup = false;
    size_t mu = 0, l = 0;
};
// the 26 bytes and the length they imply: std::invalid_argument for a wrong magic, version, gate kind, lookup flag or length
inline ProofHeader parse_proof_header(const Bytes &data) {
    if (data.size() < kProofHeaderBytes) throw std::invalid_argument(std::to_string(data.size()) + " bytes: shorter than the header");
    if (std::memcmp(data.data(), "ZKPLONK", 7)) throw std::invalid_argument("wrong magic");
    if (data[7] != kProofVersion) throw std::invalid_argument("version " + std::to_string(data[7]) + ", this reader knows " + std::to_string(kProofVersion));
    if (data[8] > 1) throw std::invalid_argument("unknown gate kind " + std::to_string(data[8]));
    if (data[9] > 1) throw std::invalid_argument("lookup flag " + std::to_string(data[9]));
    uint64_t ml[2];
    std::memcpy(ml, &data[10], 16);
    if (ml[0] > 64) throw std::invalid_argument("mu = " + std::to_string(ml[0]));
    ProofHeader h{data[8] ? GateKind::wide : GateKind::basic, data[9] != 0, (size_t)ml[0], (size_t)ml[1]};
    const size_t want = proof_size(h.gate, h.lookup, h.mu);
    if (data.size() != want) throw std::invalid_argument(std::to_string(data.size()) + " bytes, the header's record has " + std::to_string(want));
    return h;
}
// bytes -> the record with its scalars filled and its points still compressed (k x 48 bytes, in the order of the encoding); host only
struct ParsedProof {
    ProofHeader header;
    PlonkProof proof;
    Bytes compressed;
    std::vector<std::pair<std::string, size_t>> point_parts;  // (part, index) of the k points
    std::vector<size_t> point_offsets;                        // where each one's 48 bytes lie in the encoding
};
namespace detail {
inline std::vector<PointRef> parse_into(const Bytes &data, ParsedProof &out) {
    out.header = parse_proof_header(data);
    out.proof.gate = out.header.gate, out.proof.lookup = out.header.lookup, out.proof.mu = out.header.mu, out.proof.l = out.header.l;
    proof_shape(out.proof);
    ProofReader r;
    r.data = data.data();
    proof_walk(out.proof, r);
    out.compressed = std::move(r.compressed);
    for (const PointRef &p : r.refs) out.point_parts.push_back({p.part, p.index}), out.point_offsets.push_back(p.offset);
    return r.refs;
}
}  // namespace detail
inline ParsedProof parse_proof(const Bytes &data) {
    ParsedProof out;
    detail::parse_into(data, out);
    return out;
}
// the record of the bytes: parse_proof, then ONE g1_decompress_check over all k points (host: the rule above, be unused);
// std::invalid_argument names the first bad point by part, index and status
inline PlonkProof proof_from_bytes(Ctx &be, const Bytes &data, bool host = false) {
    ParsedProof pp;
    const std::vector<detail::PointRef> refs = detail::parse_into(data, pp);
    G1Vec points;
    std::vector<uint8_t> status;
    if (host) g1_decompress_check_host(pp.compressed.data(), refs.size(), points, status);
    else be.g1_decompress_check(pp.compressed.data(), refs.size(), points, status);
    for (size_t i = 0; i < refs.size(); ++i)
        if (status[i]) throw std::invalid_argument(describe_point(refs[i].part, refs[i].index, status[i]));
    for (size_t i = 0; i < refs.size(); ++i) *refs[i].slot = points[i];
    return pp.proof;
}
// the same validation for a record that is already a struct: ONE g1_check call -> every bad point
inline std::vector<BadPoint> check_points(Ctx &be, const PlonkProof &p) {
    detail::PointLister l;
    detail::proof_walk(p, l);
    G1Vec pts;
    for (const detail::PointRef &r : l.refs) pts.push_back(*r.slot);
    const std::vector<uint8_t> st = be.g1_check(pts);
    std::vector<BadPoint> bad;
    for (size_t i = 0; i < st.size(); ++i)
        if (st[i]) bad.push_back({l.refs[i].part, l.refs[i].index, st[i]});
    return bad;
}
// proof_from_bytes, the header against the vk (gate kind, lookup, mu, l) before anything else is converted, then plonk_verify; any refusal is
// false, and *why (optional) says what was refused
inline bool verify_bytes(Ctx &be, const PcsVk &vk_mu, const PcsVk &vk_mu1, const PlonkVk &vk, const FrVec &pi, const Bytes &data, std::string *why = nullptr) {
    try {
        const ProofHeader h = parse_proof_header(data);
        if (h.gate != vk.gate || h.lookup != vk.lookup || h.mu != vk.mu || h.l != vk.l) throw std::invalid_argument("the header disagrees with the verifying key");
        const PlonkProof p = proof_from_bytes(be, data);
        const bool ok = plonk_verify(be, vk_mu, vk_mu1, vk, pi, p);
        if (!ok && why) *why = "the proof does not verify";
        return ok;
    } catch (const std::invalid_argument &e) {
        if (why) *why = e.what();
        return false;
    }
}

}  // namespace zkhost
