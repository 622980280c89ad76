// RAII wrappers over the C ABI of libzkhip.so (include/zkhip.h): the compute backend of the C++ host mirror.
// Nothing here computes: every method is one C-ABI call, and a failed call throws ZkError carrying the library's status
// and message (the reference's call sites `.unwrap()` their Results; an exception is the C++ form of that panic).
#pragma once
#include <array>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "fr.hpp"
#include "zkhip.h"

namespace zkhost {

using G1 = std::array<uint64_t, 18>;  // normalised Jacobian, as ark-ec Projective (include/zkhip.h)
using G1Vec = std::vector<G1>;

struct ZkError : std::runtime_error {
    int status;
    ZkError(int status_, const std::string &what) : std::runtime_error("zkhip error " + std::to_string(status_) + ": " + what), status(status_) {}
};
// `G::msm` -> Err(min_len) (dmsm.rs:23)
struct MsmLengthError : ZkError {
    using ZkError::ZkError;
    size_t min_len = 0;
};

class Ctx;

// in the place of a prover's row-to-table indices: the device finds the first occurrence of every value itself (zkhip.lookup.FIND;
// zk_lookup_find / zk_lookup3_find).  lookup_prove(.., kFind), plonk_prove(.., kFind)
struct FindIndices {};
static const FindIndices kFind{};

// the zk_ctx itself: shared by the Ctx object and by every buffer / SRS level / job created from it, so that the library
// context is destroyed only after the last of them (a buffer that outlives its `Ctx` variable stays valid and is freed properly)
struct CtxHandle {
    zk_ctx *h = nullptr;
    explicit CtxHandle(zk_ctx *h_) : h(h_) {}
    CtxHandle(const CtxHandle &) = delete;
    ~CtxHandle() {
        if (h) zk_ctx_destroy(h);
    }
};
using CtxRef = std::shared_ptr<CtxHandle>;
using G2 = std::array<uint64_t, 36>;  // normalised G2 projective (3 x Fq2), as zk_msm_g2 returns it
using G2Rec = std::array<uint64_t, 24>;  // affine G2 x.c0 | x.c1 | y.c0 | y.c1, Montgomery form; all zero: infinity (what zk_pcs_vk_create takes)

// the verifying key of PolynomialCommitment held by the library (zk_pcs_vk: g1 and powers_of_g2)
struct PcsVk {
    CtxRef ctx;
    zk_pcs_vk *h = nullptr;
    size_t n_g2 = 0;
    PcsVk(CtxRef c, zk_pcs_vk *h_, size_t n) : ctx(std::move(c)), h(h_), n_g2(n) {}
    PcsVk(const PcsVk &) = delete;
    ~PcsVk() {
        if (h) zk_pcs_vk_free(ctx->h, h);
    }
};

// the flat arrays of zk_pcs_verify_agg / zk_pcs_agg_weights (zkhip.dist_primitive.agg_arrays): opening k has nvars[k] variables, its
// proof point i pairs with powers_g2[1 + skip[k] + i] of the FULL key, its commitment is sum_j e_j C_j over the terms cstart[k] ..
// cstart[k+1] of cpoints / cscalars (Montgomery); proofs / points hold the openings' rows one after another
struct AggArrays {
    std::vector<size_t> nvars, skip, cstart{0};
    G1Vec cpoints, proofs;
    FrVec cscalars, values, points;
    size_t count() const { return nvars.size(); }
    // one opening: (C [J], e [J], value, proofs [n], point [n], skip)
    void add(const G1Vec &c, const FrVec &e, const Fr &value, const G1Vec &pf, const FrVec &pt, size_t skip_) {
        if (c.size() != e.size() || pf.size() != pt.size()) throw ZkError(ZK_ERR_INVALID, "AggArrays::add: list lengths differ");
        nvars.push_back(pf.size()), skip.push_back(skip_), cstart.push_back(cstart.back() + c.size());
        cpoints.insert(cpoints.end(), c.begin(), c.end()), cscalars.insert(cscalars.end(), e.begin(), e.end());
        values.push_back(value), proofs.insert(proofs.end(), pf.begin(), pf.end()), points.insert(points.end(), pt.begin(), pt.end());
    }
    // the openings of `o` after mine
    void append(const AggArrays &o) {
        nvars.insert(nvars.end(), o.nvars.begin(), o.nvars.end()), skip.insert(skip.end(), o.skip.begin(), o.skip.end());
        const size_t base = cstart.back();
        for (size_t k = 1; k < o.cstart.size(); ++k) cstart.push_back(base + o.cstart[k]);
        cpoints.insert(cpoints.end(), o.cpoints.begin(), o.cpoints.end()), cscalars.insert(cscalars.end(), o.cscalars.begin(), o.cscalars.end());
        values.insert(values.end(), o.values.begin(), o.values.end());
        proofs.insert(proofs.end(), o.proofs.begin(), o.proofs.end()), points.insert(points.end(), o.points.begin(), o.points.end());
    }
};
// zk_pcs_agg_weights (host only, no ctx, no GPU): the derived 128-bit weights of pcs_verify_agg -> count x 2 u64
inline std::vector<uint64_t> pcs_agg_weights(const AggArrays &a) {
    std::vector<uint64_t> rho(2 * a.count());
    const int rc = zk_pcs_agg_weights(a.count(), a.nvars.data(), a.skip.data(), a.cstart.data(), a.cpoints.empty() ? nullptr : a.cpoints[0].data(),
                                      a.cscalars.empty() ? nullptr : a.cscalars[0].v, a.values.empty() ? nullptr : a.values[0].v,
                                      a.proofs.empty() ? nullptr : a.proofs[0].data(), a.points.empty() ? nullptr : a.points[0].v, rho.data());
    if (rc) throw ZkError(rc, "zk_pcs_agg_weights: the commitment offsets must start at 0 and not decrease");
    return rho;
}

// the witness plan of one Plonk circuit held by the library (zk_witness_plan: sources, levels, launch schedule and, built with a lookup,
// the key table of (t0, t1)); it holds its ctx
struct WitnessPlan {
    CtxRef ctx;
    zk_witness_plan *h = nullptr;
    size_t N = 0;
    bool wide = false;    // built with the wide gate's output selector
    bool lookup = false;  // built by zk_witness_plan_create_lookup: the _lookup calls serve it, the plain ones refuse it
    WitnessPlan(CtxRef c, zk_witness_plan *h_, size_t n, bool w, bool lk = false) : ctx(std::move(c)), h(h_), N(n), wide(w), lookup(lk) {}
    WitnessPlan(const WitnessPlan &) = delete;
    ~WitnessPlan() { zk_witness_plan_free(h); }
    // levels, rows of the largest level, level launches of one zk_plonk_witness
    std::array<size_t, 3> info() const {
        std::array<size_t, 3> v{};
        zk_witness_plan_info(h, &v[0], &v[1], &v[2]);
        return v;
    }
};
// the constants of one Poseidon instance on the device (zk_poseidon_params); it holds its ctx
struct PoseidonParams {
    CtxRef ctx;
    zk_poseidon_params *h = nullptr;
    PoseidonParams(CtxRef c, zk_poseidon_params *h_) : ctx(std::move(c)), h(h_) {}
    PoseidonParams(const PoseidonParams &) = delete;
    ~PoseidonParams() { zk_poseidon_params_free(h); }
};
struct WitnessReport {  // zk_plonk_witness_check(_lookup): the counts and the smallest row / slot (~0: none); the lookups on a lookup plan only
    uint64_t bad_rows = 0, first_bad_row = ~0ull, bad_copies = 0, first_bad_copy = ~0ull, bad_lookups = 0, first_bad_lookup = ~0ull;
    bool ok() const { return !bad_rows && !bad_copies && !bad_lookups; }
};

// a Fiat-Shamir transcript whose state lives on the device (zk_transcript); freed before its ctx because it holds the ctx
struct DeviceTranscript {
    CtxRef ctx;
    zk_transcript *h = nullptr;
    DeviceTranscript(CtxRef c, zk_transcript *h_) : ctx(std::move(c)), h(h_) {}
    DeviceTranscript(const DeviceTranscript &) = delete;
    ~DeviceTranscript() {
        if (h) zk_transcript_free(h);
    }
};

// a device allocation (zk_malloc / zk_free); DevPtr below shares it
struct DevAlloc {
    CtxRef ctx;
    void *ptr;
    size_t bytes;
    DevAlloc(CtxRef c, void *p, size_t b) : ctx(std::move(c)), ptr(p), bytes(b) {}
    DevAlloc(const DevAlloc &) = delete;
    ~DevAlloc() {
        if (ptr) zk_free(ctx->h, ptr);
    }
};

// a device address that keeps its allocation alive (a `Vec<Fr>` in HBM, or a slice of one)
struct DevPtr {
    std::shared_ptr<DevAlloc> owner;
    char *p = nullptr;
    DevPtr() {}
    DevPtr(std::shared_ptr<DevAlloc> o, char *p_) : owner(std::move(o)), p(p_) {}
    DevPtr at(size_t byte_off) const { return DevPtr(owner, p + byte_off); }
    DevPtr fr(size_t index) const { return at(32 * index); }
    void *get() const { return p; }
    explicit operator bool() const { return p != nullptr; }
};

// one SRS level resident in HBM (zk_srs)
class Srs {
  public:
    Srs(CtxRef c, zk_srs *h) : ctx_(std::move(c)), h_(h) {}
    Srs(const Srs &) = delete;
    ~Srs() {
        if (h_) zk_srs_free(ctx_->h, h_);
    }
    zk_srs *handle() const { return h_; }
    size_t len() const { return zk_srs_len(h_); }

  private:
    CtxRef ctx_;
    zk_srs *h_;
};
using SrsPtr = std::shared_ptr<Srs>;

// one item of zk_sumcheck_batch and what it returned
struct ScRequest {
    enum Kind { Plain = 0, Product = 1, Fold = 2, Open = 3 } kind;
    DevPtr f, g;
    size_t len;
    FrVec chal;  // the rounds' challenges (Plain / Product / Open: log2 len of them; Fold: any number)
    DevPtr out;  // optional: the output buffer of a Fold / Open request (allocated by the batch when empty)
};
struct ScResult {
    FrVec sums;       // Plain: 2 log2(len); Product: 3 log2(len)
    Fr last_f, last_g;  // Plain: last element; Product: both; Open: last_f = the value
    DevPtr out;       // Fold: folded table; Open: the len - 1 quotient elements
};

// test / self-check hook: the operands of one product sumcheck (zkhost/verify.hpp anchors every transcript of a run on them)
struct ScTrace {
    char kind;  // 'p' sumcheck_product, 'c' c_sumcheck_product, 'd' d_sumcheck_product
    DevPtr f, g;
    size_t len;
    FrVec challenge;
};

class Ctx {
  public:
    // when set, dist_primitive.hpp / pipeline.hpp append the operands of every product sumcheck they run (the DevPtrs keep the
    // tables alive); never read by the compute path
    std::vector<ScTrace> *sc_trace = nullptr;

    explicit Ctx(int device = 0) {
        int rc = zk_ctx_create(device, &h_);
        if (rc) throw ZkError(rc, "zk_ctx_create failed (no gfx950 device / library without device code?)");
        ref_ = std::make_shared<CtxHandle>(h_);
    }
    Ctx(const Ctx &) = delete;
    zk_ctx *handle() const { return h_; }
    void check(int rc) const {
        if (rc == ZK_ERR_LENGTH) throw MsmLengthError(rc, zk_last_error(h_));
        if (rc) throw ZkError(rc, zk_last_error(h_));
    }
    void sync() { check(zk_ctx_sync(h_)); }

    // ---- memory ----
    DevPtr alloc(size_t bytes) {
        void *p = nullptr;
        check(zk_malloc(h_, bytes ? bytes : 1, &p));
        return DevPtr(std::make_shared<DevAlloc>(ref_, p, bytes), (char *)p);
    }
    DevPtr alloc_fr(size_t n) { return alloc(32 * n); }
    void upload(const DevPtr &dst, const void *src, size_t bytes) {
        if (bytes) check(zk_memcpy_h2d(h_, dst.get(), src, bytes));
    }
    void download(void *dst, const DevPtr &src, size_t bytes) {
        if (bytes) check(zk_memcpy_d2h(h_, dst, src.get(), bytes));
    }
    void copy_d2d(const DevPtr &dst, const DevPtr &src, size_t bytes) {
        if (bytes) check(zk_memcpy_d2d(h_, dst.get(), src.get(), bytes));
    }
    DevPtr to_device(const FrVec &v) {
        DevPtr d = alloc_fr(v.size());
        upload(d, v.data(), 32 * v.size());
        return d;
    }
    FrVec to_host(const DevPtr &d, size_t n) {
        FrVec v(n);
        download(v.data(), d, 32 * n);
        return v;
    }

    // ---- element-wise Fr (dhyperplonk.rs:233-238,251-256,326-339) ----
    DevPtr fr_add(const DevPtr &a, const DevPtr &b, size_t n) { return binary(zk_fr_add, a, b, n); }
    DevPtr fr_sub(const DevPtr &a, const DevPtr &b, size_t n) { return binary(zk_fr_sub, a, b, n); }
    DevPtr fr_mul(const DevPtr &a, const DevPtr &b, size_t n) { return binary(zk_fr_mul, a, b, n); }
    DevPtr fr_batch_div(const DevPtr &a, const DevPtr &b, size_t n) { return binary(zk_fr_batch_div, a, b, n); }
    // out = a + alpha b + beta (a may be null: alpha b + beta)
    DevPtr fr_axpb(const DevPtr &a, const DevPtr &b, const Fr &alpha, const Fr &beta, size_t n) {
        DevPtr out = alloc_fr(n);
        check(zk_fr_axpb(h_, a.get(), b.get(), alpha.v, beta.v, out.get(), n));
        return out;
    }
    DevPtr fr_scale(const DevPtr &b, const Fr &alpha, size_t n) { return fr_axpb(DevPtr(), b, alpha, Fr::zero(), n); }
    // out[j osv + r osr] = sum_c M[r][c] in[j isv + c isc]   (zk_fr_apply_matrix)
    DevPtr fr_apply_matrix(const std::vector<FrVec> &m, const DevPtr &in, size_t isv, size_t isc, size_t k, size_t osv, size_t osr) {
        size_t rows = m.size(), cols = rows ? m[0].size() : 0;
        FrVec flat;
        for (auto &r : m) flat.insert(flat.end(), r.begin(), r.end());
        size_t span = (k && rows) ? (k - 1) * osv + (rows - 1) * osr + 1 : 1;
        DevPtr out = alloc_fr(span);
        check(zk_fr_apply_matrix(h_, flat.empty() ? nullptr : flat[0].v, rows, cols, in.get(), isv, isc, out.get(), osv, osr, k));
        return out;
    }
    template <class Tables>
    DevPtr fr_ntt_map(const Tables &t, const DevPtr &in, size_t isv, size_t isc, size_t k, size_t osv, size_t osr) {
        size_t span = k ? (k - 1) * osv + (t.take - 1) * osr + 1 : 1;
        DevPtr out = alloc_fr(span);
        check(zk_fr_ntt_map(h_, t.A, t.winv[0].v, t.B, t.w[0].v, t.scale[0].v, t.n_in, t.take, t.step, in.get(), isv, isc, out.get(), osv, osr, k));
        return out;
    }
    std::pair<DevPtr, DevPtr> fr_deinterleave(const DevPtr &t, size_t n) {
        DevPtr even = alloc_fr(n), odd = alloc_fr(n);
        check(zk_fr_deinterleave(h_, t.get(), even.get(), odd.get(), n));
        return {even, odd};
    }

    // ---- sumcheck family: the Phase-1 loops (dsumcheck.rs:10-21,37-85; mle.rs:88-105; dpoly_comm.rs:309-323; dacc_product.rs:31-38) ----
    ScResult sumcheck(const DevPtr &tab, size_t len, const FrVec &chal) {
        size_t n = log2_exact(len);
        need(chal.size() >= n, "sumcheck: fewer challenges than rounds");
        ScResult r;
        r.sums.resize(2 * n);
        check(zk_sumcheck(h_, tab.get(), len, n ? chal[0].v : nullptr, n ? r.sums[0].v : nullptr, r.last_f.v));
        return r;
    }
    ScResult sumcheck_product(const DevPtr &f, const DevPtr &g, size_t len, const FrVec &chal) {
        size_t n = log2_exact(len);
        need(chal.size() >= n, "sumcheck_product: fewer challenges than rounds");
        ScResult r;
        r.sums.resize(3 * n);
        check(zk_sumcheck_product(h_, f.get(), g.get(), len, n ? chal[0].v : nullptr, n ? r.sums[0].v : nullptr, r.last_f.v, r.last_g.v));
        return r;
    }
    DevPtr fold(const DevPtr &tab, size_t len, const FrVec &points) {
        size_t rounds = std::min(log2_exact(len), points.size());
        DevPtr out = alloc_fr(len >> rounds);
        check(zk_fold(h_, tab.get(), len, points.empty() ? nullptr : points[0].v, points.size(), out.get()));
        return out;
    }
    // zk_eq_table: eq(point, x) over the cube, x_0 the top index bit
    DevPtr eq_table(const FrVec &point) {
        DevPtr out = alloc_fr(size_t(1) << point.size());
        check(zk_eq_table(h_, point.empty() ? nullptr : point[0].v, point.size(), out.get()));
        return out;
    }
    // zk_sumcheck_gate: tabs = eq, q1, q2, a, b, c, in -> r.sums = 5 Fr per round (t = 0 .. 4), `last` = the seven remaining elements
    ScResult sumcheck_gate(const std::array<DevPtr, 7> &tabs, size_t len, const FrVec &chal, FrVec &last) {
        return fused(kFusedGate, false, len, chal, last, [&](uint64_t *sums, uint64_t *lst) {
            return zk_sumcheck_gate(h_, tabs[0].get(), tabs[1].get(), tabs[2].get(), tabs[3].get(), tabs[4].get(), tabs[5].get(), tabs[6].get(), len, chal[0].v, sums, lst);
        });
    }
    // zk_sumcheck_wiring: tree = the 2N Fr of product_tree -> r.sums = 4 Fr per round (t = 0 .. 3), `last` = eq, v1x, vx0, vx1, h, num, den
    ScResult sumcheck_wiring(const DevPtr &eq, const DevPtr &tree, const DevPtr &num, const DevPtr &den, size_t N, const Fr &gamma, const FrVec &chal,
                             FrVec &last) {
        return fused(kFusedWiring, false, N, chal, last, [&](uint64_t *sums, uint64_t *lst) {
            return zk_sumcheck_wiring(h_, eq.get(), tree.get(), num.get(), den.get(), N, gamma.v, chal[0].v, sums, lst);
        });
    }
    // zk_perm3_terms: the derived tables of the three-column wiring identity in one pass (asynchronous)
    struct Perm3Terms {
        std::array<DevPtr, 3> num, den;
        DevPtr P, Q;
    };
    Perm3Terms perm3_terms(const std::array<DevPtr, 3> &w, const std::array<DevPtr, 3> &ssigma, size_t N, const Fr &alpha, const Fr &beta) {
        Perm3Terms t;
        const void *pw[3], *ps[3];
        void *pn[3], *pd[3];
        for (int j = 0; j < 3; j++) {
            t.num[j] = alloc_fr(N), t.den[j] = alloc_fr(N);
            pw[j] = w[j].get(), ps[j] = ssigma[j].get(), pn[j] = t.num[j].get(), pd[j] = t.den[j].get();
        }
        t.P = alloc_fr(N), t.Q = alloc_fr(N);
        check(zk_perm3_terms(h_, pw, ps, N, alpha.v, beta.v, pn, pd, t.P.get(), t.Q.get()));
        return t;
    }
    // zk_sumcheck_perm3: tree = the 2N Fr of product_tree -> r.sums = 6 Fr per round (t = 0 .. 5), `last` = eq, v1x, vx0, vx1, h, n_0..2, d_0..2
    ScResult sumcheck_perm3(const DevPtr &eq, const DevPtr &tree, const std::array<DevPtr, 3> &num, const std::array<DevPtr, 3> &den, size_t N, const Fr &gamma,
                            const FrVec &chal, FrVec &last) {
        const auto pn = ptrs(num), pd = ptrs(den);
        return fused(kFusedPerm3, false, N, chal, last, [&](uint64_t *sums, uint64_t *lst) {
            return zk_sumcheck_perm3(h_, eq.get(), tree.get(), pn.data(), pd.data(), N, gamma.v, chal[0].v, sums, lst);
        });
    }
    // zk_sumcheck_gate_wide: tabs = eq, qL, qR, qM, qO, qC, qH, a, b, c, in -> r.sums = 8 Fr per round (t = 0 .. 7), `last` = the eleven remaining elements
    ScResult sumcheck_gate_wide(const std::array<DevPtr, 11> &tabs, size_t len, const FrVec &chal, FrVec &last) {
        const auto p = ptrs(tabs);
        return fused(kFusedGateWide, false, len, chal, last, [&](uint64_t *sums, uint64_t *lst) { return zk_sumcheck_gate_wide(h_, p.data(), len, chal[0].v, sums, lst); });
    }
    // zk_lookup_multiplicities: m[y] = #{x : idx[x] = y} as N Fr; idx = N u32 on the device.  A row that is not in the table: ZkError(ZK_ERR_INVALID)
    DevPtr lookup_multiplicities(const DevPtr &f, const DevPtr &t, const DevPtr &idx, size_t N) {
        DevPtr m = alloc_fr(N);
        check(zk_lookup_multiplicities(h_, f.get(), t.get(), (const uint32_t *)idx.get(), N, m.get()));
        return m;
    }
    // zk_sumcheck_lookup: tabs = E, df, dt, m, hf, ht -> r.sums = 4 Fr per round (t = 0 .. 3), `last` = the six remaining elements
    ScResult sumcheck_lookup(const std::array<DevPtr, 6> &tabs, size_t len, const Fr &gamma, const FrVec &chal, FrVec &last) {
        const auto p = ptrs(tabs);
        return fused(kFusedLookup, false, len, chal, last, [&](uint64_t *sums, uint64_t *lst) { return zk_sumcheck_lookup(h_, p.data(), len, gamma.v, chal[0].v, sums, lst); });
    }
    // zk_lookup3_multiplicities: m[y] = #{x : qk(x) = 1, idx[x] = y} as N Fr; w = a, b, c; t = t0, t1, t2; idx = N u32 on the device.  A selected
    // row whose triple is not the table entry it names, or a qk that is neither 0 nor 1: ZkError(ZK_ERR_INVALID)
    DevPtr lookup3_multiplicities(const std::array<DevPtr, 3> &w, const std::array<DevPtr, 3> &t, const DevPtr &qk, const DevPtr &idx, size_t N) {
        DevPtr m = alloc_fr(N);
        const void *pw[3] = {w[0].get(), w[1].get(), w[2].get()}, *pt[3] = {t[0].get(), t[1].get(), t[2].get()};
        check(zk_lookup3_multiplicities(h_, pw, pt, qk.get(), (const uint32_t *)idx.get(), N, m.get()));
        return m;
    }
    // zk_lookup_find: idx[x] = the smallest y with t[y] = f[x] (N u32) and the multiplicities of that idx (N Fr), found on the device.  A row
    // whose value is no entry of the table: ZkError(ZK_ERR_INVALID)
    std::pair<DevPtr, DevPtr> lookup_find(const DevPtr &f, const DevPtr &t, size_t N) {
        DevPtr idx = alloc(4 * N), m = alloc_fr(N);
        check(zk_lookup_find(h_, f.get(), t.get(), N, (uint32_t *)idx.get(), m.get()));
        return {idx, m};
    }
    // zk_lookup3_find: the same for the rows with qk(x) = 1 of a Plonk circuit (idx = 0 where qk = 0); w = a, b, c; t = t0, t1, t2.  A selected
    // row whose triple is no entry of the table, or a qk that is neither 0 nor 1: ZkError(ZK_ERR_INVALID)
    std::pair<DevPtr, DevPtr> lookup3_find(const std::array<DevPtr, 3> &w, const std::array<DevPtr, 3> &t, const DevPtr &qk, size_t N) {
        DevPtr idx = alloc(4 * N), m = alloc_fr(N);
        const void *pw[3] = {w[0].get(), w[1].get(), w[2].get()}, *pt[3] = {t[0].get(), t[1].get(), t[2].get()};
        check(zk_lookup3_find(h_, pw, pt, qk.get(), N, (uint32_t *)idx.get(), m.get()));
        return {idx, m};
    }
    // zk_lookup3_terms: df = beta + a + zeta b + zeta^2 c, dt = beta + t0 + zeta t1 + zeta^2 t2 in one pass (asynchronous)
    std::pair<DevPtr, DevPtr> lookup3_terms(const std::array<DevPtr, 3> &w, const std::array<DevPtr, 3> &t, size_t N, const Fr &zeta, const Fr &beta) {
        DevPtr df = alloc_fr(N), dt = alloc_fr(N);
        const void *pw[3] = {w[0].get(), w[1].get(), w[2].get()}, *pt[3] = {t[0].get(), t[1].get(), t[2].get()};
        check(zk_lookup3_terms(h_, pw, pt, N, zeta.v, beta.v, df.get(), dt.get()));
        return {df, dt};
    }
    // zk_sumcheck_lookup_sel: tabs = E, df, dt, m, hf, ht, qk -> r.sums = 4 Fr per round (t = 0 .. 3), `last` = the seven remaining elements
    ScResult sumcheck_lookup_sel(const std::array<DevPtr, 7> &tabs, size_t len, const Fr &gamma, const FrVec &chal, FrVec &last) {
        const auto p = ptrs(tabs);
        return fused(kFusedLookupSel, false, len, chal, last, [&](uint64_t *sums, uint64_t *lst) { return zk_sumcheck_lookup_sel(h_, p.data(), len, gamma.v, chal[0].v, sums, lst); });
    }
    // zk_eq_table_acc: acc[x] += weight * eq(point, x), acc = 2^n Fr (asynchronous)
    void eq_table_acc(const FrVec &point, const Fr &weight, const DevPtr &acc) {
        check(zk_eq_table_acc(h_, point.empty() ? nullptr : point[0].v, point.size(), weight.v, acc.get()));
    }
    // zk_fr_lincomb: out[x] = sum_j coeffs[j] tabs[j][x], 1 .. 16 tables of len Fr (asynchronous)
    DevPtr fr_lincomb(const std::vector<DevPtr> &tabs, const FrVec &coeffs, size_t len) {
        need(!tabs.empty() && tabs.size() == coeffs.size(), "fr_lincomb: one coefficient per table");
        std::vector<const void *> p;
        for (const DevPtr &t : tabs) p.push_back(t.get());
        DevPtr out = alloc_fr(len);
        check(zk_fr_lincomb(h_, p.size(), p.data(), coeffs[0].v, len, out.get()));
        return out;
    }
    // zk_sumcheck_multi: the rounds of sum_j es[j] fs[j] -> r.sums = 3 Fr per round (t0, t1, t2); last_e / last_f = the folded-out values
    ScResult sumcheck_multi(const std::vector<DevPtr> &es, const std::vector<DevPtr> &fs, size_t len, const FrVec &chal, FrVec &last_e,
                            FrVec &last_f) {
        size_t n = log2_exact(len);
        need(!es.empty() && es.size() == fs.size(), "sumcheck_multi: one eq table per table");
        need(n >= 1 && chal.size() >= n, "sumcheck_multi: fewer challenges than rounds");
        std::vector<const void *> pe, pf;
        for (const DevPtr &t : es) pe.push_back(t.get());
        for (const DevPtr &t : fs) pf.push_back(t.get());
        ScResult r;
        r.sums.resize(3 * n);
        last_e.assign(es.size(), Fr::zero());
        last_f.assign(es.size(), Fr::zero());
        check(zk_sumcheck_multi(h_, pe.size(), pe.data(), pf.data(), len, chal[0].v, r.sums[0].v, last_e[0].v, last_f[0].v));
        return r;
    }
    // ---- Fiat-Shamir: the transcript on the device and the three sumchecks driven by it (`chal` receives the derived challenges) ----
    std::shared_ptr<DeviceTranscript> transcript(const std::string &label) {
        zk_transcript *t = nullptr;
        check(zk_transcript_create(h_, label.data(), label.size(), &t));
        return std::make_shared<DeviceTranscript>(ref_, t);
    }
    void absorb(DeviceTranscript &t, const void *bytes, size_t n) { check(zk_transcript_absorb(h_, t.h, bytes, n)); }
    FrVec challenges(DeviceTranscript &t, size_t count) {
        FrVec out(count);
        if (count) check(zk_transcript_challenges(h_, t.h, count, out[0].v));
        return out;
    }
    ScResult sumcheck_gate_fs(const std::array<DevPtr, 7> &tabs, size_t len, DeviceTranscript &t, FrVec &last, FrVec &chal) {
        chal.assign(log2_exact(len), Fr::zero());
        return fused(kFusedGate, true, len, chal, last, [&](uint64_t *sums, uint64_t *lst) {
            return zk_sumcheck_gate_fs(h_, tabs[0].get(), tabs[1].get(), tabs[2].get(), tabs[3].get(), tabs[4].get(), tabs[5].get(), tabs[6].get(), len, t.h, sums, lst, chal[0].v);
        });
    }
    ScResult sumcheck_wiring_fs(const DevPtr &eq, const DevPtr &tree, const DevPtr &num, const DevPtr &den, size_t N, const Fr &gamma, DeviceTranscript &t, FrVec &last,
                                FrVec &chal) {
        chal.assign(log2_exact(N), Fr::zero());
        return fused(kFusedWiring, true, N, chal, last, [&](uint64_t *sums, uint64_t *lst) {
            return zk_sumcheck_wiring_fs(h_, eq.get(), tree.get(), num.get(), den.get(), N, gamma.v, t.h, sums, lst, chal[0].v);
        });
    }
    ScResult sumcheck_perm3_fs(const DevPtr &eq, const DevPtr &tree, const std::array<DevPtr, 3> &num, const std::array<DevPtr, 3> &den, size_t N, const Fr &gamma,
                               DeviceTranscript &t, FrVec &last, FrVec &chal) {
        const auto pn = ptrs(num), pd = ptrs(den);
        chal.assign(log2_exact(N), Fr::zero());
        return fused(kFusedPerm3, true, N, chal, last, [&](uint64_t *sums, uint64_t *lst) {
            return zk_sumcheck_perm3_fs(h_, eq.get(), tree.get(), pn.data(), pd.data(), N, gamma.v, t.h, sums, lst, chal[0].v);
        });
    }
    ScResult sumcheck_gate_wide_fs(const std::array<DevPtr, 11> &tabs, size_t len, DeviceTranscript &t, FrVec &last, FrVec &chal) {
        const auto p = ptrs(tabs);
        chal.assign(log2_exact(len), Fr::zero());
        return fused(kFusedGateWide, true, len, chal, last, [&](uint64_t *sums, uint64_t *lst) { return zk_sumcheck_gate_wide_fs(h_, p.data(), len, t.h, sums, lst, chal[0].v); });
    }
    ScResult sumcheck_lookup_fs(const std::array<DevPtr, 6> &tabs, size_t len, const Fr &gamma, DeviceTranscript &t, FrVec &last, FrVec &chal) {
        const auto p = ptrs(tabs);
        chal.assign(log2_exact(len), Fr::zero());
        return fused(kFusedLookup, true, len, chal, last, [&](uint64_t *sums, uint64_t *lst) { return zk_sumcheck_lookup_fs(h_, p.data(), len, gamma.v, t.h, sums, lst, chal[0].v); });
    }
    ScResult sumcheck_lookup_sel_fs(const std::array<DevPtr, 7> &tabs, size_t len, const Fr &gamma, DeviceTranscript &t, FrVec &last, FrVec &chal) {
        const auto p = ptrs(tabs);
        chal.assign(log2_exact(len), Fr::zero());
        return fused(kFusedLookupSel, true, len, chal, last, [&](uint64_t *sums, uint64_t *lst) { return zk_sumcheck_lookup_sel_fs(h_, p.data(), len, gamma.v, t.h, sums, lst, chal[0].v); });
    }
    ScResult sumcheck_multi_fs(const std::vector<DevPtr> &es, const std::vector<DevPtr> &fs, size_t len, DeviceTranscript &t, FrVec &last_e, FrVec &last_f,
                               FrVec &chal) {
        size_t n = log2_exact(len);
        need(!es.empty() && es.size() == fs.size(), "sumcheck_multi_fs: one eq table per table");
        need(n >= 1, "sumcheck_multi_fs: at least one round");
        std::vector<const void *> pe, pf;
        for (const DevPtr &x : es) pe.push_back(x.get());
        for (const DevPtr &x : fs) pf.push_back(x.get());
        ScResult r;
        r.sums.resize(3 * n);
        last_e.assign(es.size(), Fr::zero());
        last_f.assign(es.size(), Fr::zero());
        chal.assign(n, Fr::zero());
        check(zk_sumcheck_multi_fs(h_, pe.size(), pe.data(), pf.data(), len, t.h, r.sums[0].v, last_e[0].v, last_f[0].v, chal[0].v));
        return r;
    }
    ScResult open_rounds(const DevPtr &tab, size_t len, const FrVec &point) {
        need(point.size() >= log2_exact(len), "open: fewer point coordinates than rounds");
        ScResult r;
        r.out = alloc_fr(len - 1);
        check(zk_open_rounds(h_, tab.get(), len, point.empty() ? nullptr : point[0].v, r.out.get(), r.last_f.v));
        return r;
    }
    DevPtr product_tree(const DevPtr &x, size_t N) {
        DevPtr out = alloc_fr(2 * N);
        check(zk_product_tree(h_, x.get(), N, out.get()));
        return out;
    }
    // several independent calls in one go (zk_sumcheck_batch); every output equals the single call's
    std::vector<ScResult> sumcheck_batch(const std::vector<ScRequest> &reqs) {
        std::vector<ScResult> res(reqs.size());
        std::vector<zk_sc_item> items(reqs.size());
        for (size_t i = 0; i < reqs.size(); ++i) {
            const ScRequest &q = reqs[i];
            size_t n = log2_exact(q.len);
            zk_sc_item &it = items[i];
            it = zk_sc_item{};
            it.mode = (int)q.kind, it.d_f = q.f.get(), it.d_g = q.g.get(), it.len = q.len;
            it.h_chal = q.chal.empty() ? nullptr : q.chal[0].v;
            it.n_points = q.chal.size();
            if (q.kind != ScRequest::Fold) need(q.chal.size() >= n, "sumcheck_batch: fewer challenges than rounds");
            if (q.kind == ScRequest::Plain || q.kind == ScRequest::Product) {
                res[i].sums.resize((q.kind == ScRequest::Plain ? 2 : 3) * n);
                it.h_sums = n ? res[i].sums[0].v : nullptr;
            } else if (q.kind == ScRequest::Fold) {
                res[i].out = q.out ? q.out : alloc_fr(q.len >> std::min(n, q.chal.size()));
            } else {
                res[i].out = q.out ? q.out : alloc_fr(q.len - 1);
            }
            it.h_last_f = res[i].last_f.v, it.h_last_g = res[i].last_g.v, it.d_out = res[i].out.get();
        }
        if (!reqs.empty()) check(zk_sumcheck_batch(h_, items.size(), items.data()));
        return res;
    }

    // ---- SRS ----
    SrsPtr srs_register(const void *bases, size_t stride, size_t n) {
        zk_srs *s = nullptr;
        check(zk_srs_register(h_, bases, stride, n, &s));
        return std::make_shared<Srs>(ref_, s);
    }
    // P_i = (k0 + i k1) G (canonical scalars)
    SrsPtr srs_generate(uint64_t k0, uint64_t k1, size_t n) {
        uint64_t a[4] = {k0, 0, 0, 0}, b[4] = {k1, 0, 0, 0};
        zk_srs *s = nullptr;
        check(zk_srs_generate(h_, a, b, n, &s));
        return std::make_shared<Srs>(ref_, s);
    }
    // PolynomialCommitmentCub::new (dpoly_comm.rs:37-67): levels 0 .. nvars
    std::vector<SrsPtr> srs_powers(const FrVec &s, const void *g96 = nullptr) {
        std::vector<zk_srs *> lv(s.size() + 1, nullptr);
        check(zk_srs_powers(h_, g96, s.empty() ? nullptr : s[0].v, s.size(), lv.data()));
        std::vector<SrsPtr> out;
        for (zk_srs *x : lv) out.push_back(std::make_shared<Srs>(ref_, x));
        return out;
    }
    // to_packed for ONE party (dpoly_comm.rs:164-194): row = l canonical pack coefficients
    SrsPtr srs_to_packed(const Srs &level, const FrVec &row_canonical, size_t l) {
        zk_srs *s = nullptr;
        check(zk_srs_to_packed(h_, level.handle(), row_canonical[0].v, l, &s));
        return std::make_shared<Srs>(ref_, s);
    }
    void srs_precompute(Srs &s, int window_bits = 0, int record_bytes = 0) {  // record_bytes: 0 / 96 packed (default), 128 = one G1 record per cache line
        check(record_bytes ? zk_srs_precompute_layout(h_, s.handle(), window_bits, record_bytes) : zk_srs_precompute(h_, s.handle(), window_bits));
    }

    // ---- MSM ----
    G1 msm_g1(const Srs &srs, const DevPtr &scalars, size_t n, size_t offset = 0) {
        G1 out;
        check(zk_msm_g1(h_, srs.handle(), offset, scalars.get(), n, out.data()));
        return out;
    }
    // drop-in for `G::msm(&[Affine], &[Fr]) -> Result<G, usize>` on host slices (dmsm.rs:23): bases at `stride` bytes (96, or 104 =
    // the Rust struct); a length mismatch throws MsmLengthError whose min_len is the reference's Err(min_len)
    G1 msm_g1_host(const void *bases, size_t stride, size_t n_bases, const FrVec &scalars) {
        G1 out;
        size_t min_len = 0;
        int rc = zk_msm_g1_host(h_, bases, stride, n_bases, scalars.empty() ? nullptr : scalars[0].v, scalars.size(), out.data(), &min_len);
        if (rc == ZK_ERR_LENGTH) {
            MsmLengthError e(rc, zk_last_error(h_));
            e.min_len = min_len;
            throw e;
        }
        check(rc);
        return out;
    }
    G1Vec msm_g1_batch(const std::vector<const Srs *> &srs, const std::vector<DevPtr> &scalars, const std::vector<size_t> &lens) {
        size_t count = lens.size();
        need(srs.size() == count && scalars.size() == count, "msm batch: list lengths differ");
        G1Vec out(count);
        if (!count) return out;
        std::vector<const zk_srs *> h(count);
        std::vector<const void *> sp(count);
        for (size_t i = 0; i < count; ++i) h[i] = srs[i]->handle(), sp[i] = scalars[i].get();
        check(zk_msm_g1_batch(h_, count, h.data(), nullptr, sp.data(), lens.data(), out[0].data()));
        return out;
    }
    // asynchronous form: the pass runs on the ctx's job lanes while the caller enqueues other work; wait() collects the points.
    // The scalar buffers must stay alive and unmodified until then (MsmJob holds them).
    struct MsmJob {
        CtxRef ctx;
        zk_msm_job *job = nullptr;
        size_t count = 0;
        std::vector<DevPtr> keep;
        MsmJob() {}
        MsmJob(const MsmJob &) = delete;
        MsmJob(MsmJob &&o) noexcept { *this = std::move(o); }
        MsmJob &operator=(MsmJob &&o) noexcept {
            drain();
            ctx = std::move(o.ctx), job = o.job, count = o.count, keep = std::move(o.keep);
            o.job = nullptr;
            return *this;
        }
        ~MsmJob() { drain(); }
        bool pending() const { return job != nullptr; }
        void drain() {  // never waited for: let it finish and release it
            if (job) {
                G1Vec tmp(count);
                zk_msm_wait(ctx->h, job, tmp[0].data());
                job = nullptr;
            }
        }
    };
    MsmJob msm_g1_batch_async(const std::vector<const Srs *> &srs, const std::vector<DevPtr> &scalars, const std::vector<size_t> &lens) {
        size_t count = lens.size();
        need(srs.size() == count && scalars.size() == count && count > 0, "msm batch: list lengths differ / empty");
        std::vector<const zk_srs *> h(count);
        std::vector<const void *> sp(count);
        for (size_t i = 0; i < count; ++i) h[i] = srs[i]->handle(), sp[i] = scalars[i].get();
        MsmJob j;
        j.ctx = ref_, j.count = count, j.keep = scalars;
        check(zk_msm_g1_batch_async(h_, count, h.data(), nullptr, sp.data(), lens.data(), &j.job));
        return j;
    }
    G1Vec msm_wait(MsmJob &j) {
        G1Vec out(j.count);
        zk_msm_job *job = j.job;
        j.job = nullptr;  // (zk_msm_wait releases the job also on error)
        int rc = job ? zk_msm_wait(h_, job, out[0].data()) : 0;
        j.keep.clear();  // only now: the pass read the scalar buffers until the wait returned
        check(rc);
        return out;
    }
    // the whole of d_msm in one call over the ctx's communicator (zk_d_msm)
    G1Vec d_msm(const std::vector<const Srs *> &srs, const std::vector<DevPtr> &scalars, const std::vector<size_t> &lens, const Fr *lambda_mont,
                const FrVec &coeffs_canonical) {
        size_t count = lens.size();
        G1Vec out(count);
        if (!count) return out;
        std::vector<const zk_srs *> h(count);
        std::vector<const void *> sp(count);
        for (size_t i = 0; i < count; ++i) h[i] = srs[i]->handle(), sp[i] = scalars[i].get();
        check(zk_d_msm(h_, count, h.data(), nullptr, sp.data(), lens.data(), lambda_mont ? lambda_mont->v : nullptr, coeffs_canonical[0].v, out[0].data()));
        return out;
    }
    // the level's points in the reference layout (96 B each: x || y Montgomery limbs, zeros = infinity), on the host
    std::vector<uint8_t> srs_download(const Srs &s) {
        std::vector<uint8_t> out(96 * s.len());
        if (!out.empty()) check(zk_srs_download(h_, s.handle(), out.data()));
        return out;
    }
    // zk_fr_apply_matrix on affine G1 points in HBM (96-B records): the PSS maps are generic over DomainCoeff (pss.rs:93-171).
    // m: CANONICAL scalars; out[j osv + r osr] = sum_c m[r][c] in[j isv + c isc]
    DevPtr g1_apply_matrix(const std::vector<FrVec> &m_canonical, const DevPtr &in96, size_t isv, size_t isc, size_t k, size_t osv, size_t osr) {
        size_t rows = m_canonical.size(), cols = rows ? m_canonical[0].size() : 0;
        FrVec flat;
        for (auto &r : m_canonical) flat.insert(flat.end(), r.begin(), r.end());
        size_t span = (k && rows) ? (k - 1) * osv + (rows - 1) * osr + 1 : 1;
        DevPtr out = alloc(96 * span);
        check(zk_g1_apply_matrix(h_, flat.empty() ? nullptr : flat[0].v, rows, cols, in96.get(), isv, isc, out.get(), osv, osr, k));
        return out;
    }
    // out[r] = sum_i k_i P[r n + i]; k canonical (zk_g1_lincomb_batch: the leader's public maps on points)
    // ---- G2 and the pairing ----
    SrsPtr srs_register_g2(const void *bases, size_t stride, size_t n) {
        zk_srs *s = nullptr;
        check(zk_srs_register_g2(h_, bases, stride, n, &s));
        return std::make_shared<Srs>(ref_, s);
    }
    G2 msm_g2(const Srs &srs, const DevPtr &scalars, size_t n, size_t offset = 0) {
        G2 out;
        check(zk_msm_g2(h_, srs.handle(), offset, scalars.get(), n, out.data()));
        return out;
    }
    // ---- Poseidon at t = 3 (zk_poseidon_*; the rule and the instance: include/zkhip.h, zkhost/poseidon.hpp) ----
    // rc: 3 (rf + rp) round constants, mds: 9 matrix entries row-major.  An odd rf, rf = 0 or rf + rp > 256: ZkError(ZK_ERR_INVALID)
    std::shared_ptr<PoseidonParams> poseidon_params(int rf, int rp, const FrVec &rc, const FrVec &mds) {
        need(rf + rp >= 0 && rc.size() == 3 * size_t(rf + rp) && mds.size() == 9, "poseidon_params: 3 (rf + rp) round constants and 9 matrix entries are needed");
        zk_poseidon_params *p = nullptr;
        check(zk_poseidon_params_create(h_, rf, rp, rc.empty() ? mds[0].v : rc[0].v, mds[0].v, &p));
        return std::make_shared<PoseidonParams>(ref_, p);
    }
    // n states of three Fr; out may be the input itself (default: a new buffer).  Asynchronous
    DevPtr poseidon_permute(const PoseidonParams &pp, const DevPtr &in, size_t n, const DevPtr *out = nullptr) {
        DevPtr o = out ? *out : alloc_fr(3 * n);
        check(zk_poseidon_permute(h_, pp.h, in.get(), o.get(), n));
        return o;
    }
    DevPtr poseidon_hash2(const PoseidonParams &pp, const DevPtr &left, const DevPtr &right, size_t n, const DevPtr *out = nullptr) {
        DevPtr o = out ? *out : alloc_fr(n);
        check(zk_poseidon_hash2(h_, pp.h, left.get(), right.get(), o.get(), n));
        return o;
    }
    // the tree of n = 2^k leaves: 2n - 1 Fr, the root last.  Asynchronous
    DevPtr poseidon_merkle(const PoseidonParams &pp, const DevPtr &leaves, size_t n) {
        DevPtr o = alloc_fr(n ? 2 * n - 1 : 1);
        check(zk_poseidon_merkle(h_, pp.h, leaves.get(), n, o.get()));
        return o;
    }
    // the tree kept on the device.  Indices are host integers, validated by the library (ZkError(ZK_ERR_INVALID) with its message).  Asynchronous
    // [count][d] siblings of the leaves `index` (any order, repeats allowed), path k contiguous from the leaf level up
    DevPtr poseidon_merkle_paths(const DevPtr &tree, size_t n, const std::vector<uint64_t> &index) {
        size_t d = 0;
        while ((size_t(1) << d) < n) ++d;
        DevPtr o = alloc_fr(index.size() * d);
        check(zk_poseidon_merkle_paths(h_, tree.get(), n, index.data(), index.size(), o.get()));
        return o;
    }
    // the root each leaf reaches through its `depth` siblings with the bits of its index
    DevPtr poseidon_merkle_roots(const PoseidonParams &pp, const DevPtr &leaves, const std::vector<uint64_t> &index, const DevPtr &siblings, size_t depth) {
        DevPtr o = alloc_fr(index.size());
        check(zk_poseidon_merkle_roots(h_, pp.h, leaves.get(), index.data(), siblings.get(), depth, index.size(), o.get()));
        return o;
    }
    // tree[index[k]] = values[k] in place, then the nodes above the written leaves; index strictly ascending (zkhost::poseidon_update sorts)
    void poseidon_merkle_update(const PoseidonParams &pp, const DevPtr &tree, size_t n, const std::vector<uint64_t> &index, const DevPtr &values) {
        check(zk_poseidon_merkle_update(h_, pp.h, tree.get(), n, index.data(), values.get(), index.size()));
    }
    // ---- Jubjub and Schnorr verification (zk_jubjub_*, zk_schnorr_verify; the rule: include/zkhip.h, zkhost/jubjub.hpp) ----
    // out[i] = [scalars[i]] points[i]: points n x 2 Fr (a null DevPtr: the fixed base G), scalars n x 4 uint64_t plain integers.  An off-curve
    // point: ZkError(ZK_ERR_INVALID) with the library's "K of N points are not on the curve; the first is I", nothing written
    DevPtr jubjub_mul(const DevPtr &points, const DevPtr &scalars, size_t n) {
        DevPtr o = alloc_fr(n ? 2 * n : 1);
        check(zk_jubjub_mul(h_, points.get(), scalars.get(), o.get(), n));
        return o;
    }
    // one status per point: 0 in the prime-order subgroup, 2 not on the curve, 3 on the curve but outside the subgroup.  Blocking
    std::vector<uint32_t> jubjub_check(const DevPtr &points, size_t n) {
        std::vector<uint32_t> status(n, 0);
        DevPtr st = alloc(n ? 4 * n : 4);
        check(zk_jubjub_check(h_, points.get(), static_cast<uint32_t *>(st.get()), n));
        download(status.data(), st, 4 * n);
        return status;
    }
    // one status per signature (0 valid, 1 s >= l, 2 off the curve, 3 PK outside the subgroup or the identity, 4 the equation): pk n x 2 Fr,
    // msg n Fr, sig n x 3 words (R.x, R.y Montgomery; s a plain integer).  Blocking
    std::vector<uint32_t> schnorr_verify(const PoseidonParams &pp, const DevPtr &pk, const DevPtr &msg, const DevPtr &sig, size_t n) {
        std::vector<uint32_t> status(n, 0);
        DevPtr st = alloc(n ? 4 * n : 4);
        check(zk_schnorr_verify(h_, pp.h, pk.get(), msg.get(), sig.get(), static_cast<uint32_t *>(st.get()), n));
        download(status.data(), st, 4 * n);
        return status;
    }
    // ---- Plonk witness (zk_witness_plan_create, zk_plonk_witness, zk_plonk_witness_check) ----
    // sigma: 3N slot numbers; out_sel: the wide gate's qO on the device (null: every row computes).  Rows that depend on their own output or a
    // sigma that is not a permutation: ZkError(ZK_ERR_INVALID)
    std::shared_ptr<WitnessPlan> witness_plan(const std::vector<uint64_t> &sigma, size_t N, const DevPtr *out_sel = nullptr) {
        need(sigma.size() == 3 * N, "witness_plan: sigma must hold 3N slot numbers");
        zk_witness_plan *p = nullptr;
        check(zk_witness_plan_create(h_, sigma.data(), out_sel ? out_sel->get() : nullptr, N, &p));
        return std::make_shared<WitnessPlan>(ref_, p, N, out_sel != nullptr);
    }
    // a, b, c generated on the device; free: 3N Fr or null (zeros).  A bad gate row or copy: ZkError(ZK_ERR_INVALID) with the library's message
    std::array<DevPtr, 3> plonk_witness(const WitnessPlan &plan, const std::vector<DevPtr> &sel, const FrVec &public_inputs, const DevPtr *free = nullptr) {
        std::array<DevPtr, 3> w = {alloc_fr(plan.N), alloc_fr(plan.N), alloc_fr(plan.N)};
        std::vector<const void *> ps;
        for (const DevPtr &d : sel) ps.push_back(d.get());
        check(zk_plonk_witness(h_, plan.h, sel.size() == 6 ? 1 : 0, ps.data(), public_inputs.empty() ? nullptr : public_inputs[0].v, public_inputs.size(),
                               free ? free->get() : nullptr, w[0].get(), w[1].get(), w[2].get()));
        return w;
    }
    WitnessReport plonk_witness_check(const WitnessPlan &plan, const std::vector<DevPtr> &sel, const FrVec &public_inputs, const DevPtr &a, const DevPtr &b, const DevPtr &c) {
        std::vector<const void *> ps;
        for (const DevPtr &d : sel) ps.push_back(d.get());
        uint64_t bad[4];
        check(zk_plonk_witness_check(h_, plan.h, sel.size() == 6 ? 1 : 0, ps.data(), public_inputs.empty() ? nullptr : public_inputs[0].v, public_inputs.size(), a.get(),
                                     b.get(), c.get(), bad));
        WitnessReport r;
        r.bad_rows = bad[0], r.first_bad_row = bad[1], r.bad_copies = bad[2], r.first_bad_copy = bad[3];
        return r;
    }
    // ---- the same with the circuit's lookup (zk_witness_plan_create_lookup, zk_plonk_witness_lookup, zk_plonk_witness_check_lookup) ----
    // qk, table = t0, t1, t2: N Fr each on the device.  Beyond witness_plan's refusals: a qk entry that is neither 0 nor 1, a table that is no
    // function of (t0, t1): ZkError(ZK_ERR_INVALID) with the library's message.  The two calls take the qk and the table the plan was built from
    std::shared_ptr<WitnessPlan> witness_plan_lookup(const std::vector<uint64_t> &sigma, size_t N, const DevPtr *out_sel, const DevPtr &qk, const std::array<DevPtr, 3> &table) {
        need(sigma.size() == 3 * N, "witness_plan_lookup: sigma must hold 3N slot numbers");
        const void *t[3] = {table[0].get(), table[1].get(), table[2].get()};
        zk_witness_plan *p = nullptr;
        check(zk_witness_plan_create_lookup(h_, sigma.data(), out_sel ? out_sel->get() : nullptr, qk.get(), t, N, &p));
        return std::make_shared<WitnessPlan>(ref_, p, N, out_sel != nullptr, true);
    }
    std::array<DevPtr, 3> plonk_witness_lookup(const WitnessPlan &plan, const std::vector<DevPtr> &sel, const DevPtr &qk, const std::array<DevPtr, 3> &table,
                                               const FrVec &public_inputs, const DevPtr *free = nullptr) {
        std::array<DevPtr, 3> w = {alloc_fr(plan.N), alloc_fr(plan.N), alloc_fr(plan.N)};
        std::vector<const void *> ps;
        for (const DevPtr &d : sel) ps.push_back(d.get());
        const void *t[3] = {table[0].get(), table[1].get(), table[2].get()};
        check(zk_plonk_witness_lookup(h_, plan.h, sel.size() == 6 ? 1 : 0, ps.data(), qk.get(), t, public_inputs.empty() ? nullptr : public_inputs[0].v, public_inputs.size(),
                                      free ? free->get() : nullptr, w[0].get(), w[1].get(), w[2].get()));
        return w;
    }
    WitnessReport plonk_witness_check_lookup(const WitnessPlan &plan, const std::vector<DevPtr> &sel, const DevPtr &qk, const std::array<DevPtr, 3> &table,
                                             const FrVec &public_inputs, const DevPtr &a, const DevPtr &b, const DevPtr &c) {
        std::vector<const void *> ps;
        for (const DevPtr &d : sel) ps.push_back(d.get());
        const void *t[3] = {table[0].get(), table[1].get(), table[2].get()};
        uint64_t bad[6];
        check(zk_plonk_witness_check_lookup(h_, plan.h, sel.size() == 6 ? 1 : 0, ps.data(), qk.get(), t, public_inputs.empty() ? nullptr : public_inputs[0].v,
                                            public_inputs.size(), a.get(), b.get(), c.get(), bad));
        WitnessReport r;
        r.bad_rows = bad[0], r.first_bad_row = bad[1], r.bad_copies = bad[2], r.first_bad_copy = bad[3], r.bad_lookups = bad[4], r.first_bad_lookup = bad[5];
        return r;
    }
    // ---- a plan with the circuit's advice codes (zk_witness_plan_create_advice): N u32 (0: none, ZK_ADV_INV0, ZK_ADV_BITS(shift, width)); qk and
    // table as witness_plan_lookup takes them, or both null.  Beyond the refusals of those two: unknown codes, advice rows that also compute by
    // the gate or the table.  plonk_witness / plonk_witness_lookup and the checks take the plan as they take the others
    std::shared_ptr<WitnessPlan> witness_plan_advice(const std::vector<uint64_t> &sigma, size_t N, const DevPtr *out_sel, const std::vector<uint32_t> &advice,
                                                     const DevPtr *qk = nullptr, const std::array<DevPtr, 3> *table = nullptr) {
        need(sigma.size() == 3 * N && advice.size() == N, "witness_plan_advice: sigma must hold 3N slot numbers and advice N codes");
        need((qk != nullptr) == (table != nullptr), "witness_plan_advice: a lookup needs qk and the table");
        const void *t[3] = {nullptr, nullptr, nullptr};
        for (size_t j = 0; table && j < 3; ++j) t[j] = (*table)[j].get();
        zk_witness_plan *p = nullptr;
        check(zk_witness_plan_create_advice(h_, sigma.data(), out_sel ? out_sel->get() : nullptr, qk ? qk->get() : nullptr, table ? t : nullptr, advice.data(), N, &p));
        return std::make_shared<WitnessPlan>(ref_, p, N, out_sel != nullptr, qk != nullptr);
    }
    // g1_96: powers_of_g[0][0] as a 96-byte affine record (nullptr: the generator); powers_g2: n_g2 affine records at `stride`
    std::shared_ptr<PcsVk> pcs_vk(const void *g1_96, const void *powers_g2, size_t stride, size_t n_g2) {
        zk_pcs_vk *vk = nullptr;
        check(zk_pcs_vk_create(h_, g1_96, powers_g2, stride, n_g2, &vk));
        return std::make_shared<PcsVk>(ref_, vk, n_g2);
    }
    // count openings of nvars-variate polynomials: proofs count x nvars, points count x nvars -> one verdict per opening
    std::vector<bool> pcs_verify_batch(const PcsVk &vk, size_t nvars, const G1Vec &commitments, const FrVec &values, const G1Vec &proofs,
                                       const FrVec &points) {
        size_t count = commitments.size();
        need(values.size() == count && proofs.size() == count * nvars && points.size() == count * nvars, "pcs_verify_batch: list lengths differ");
        std::vector<uint8_t> ok(count ? count : 1, 0);
        if (count)
            check(zk_pcs_verify_batch(h_, vk.h, nvars, count, commitments[0].data(), values[0].v, nvars ? proofs[0].data() : nullptr,
                                      nvars ? points[0].v : nullptr, ok.data()));
        return std::vector<bool>(ok.begin(), ok.begin() + count);
    }

    // out[s] = sum_{starts[s] <= t < starts[s+1]} k_t P_t on the device (zk_g1_lincomb_seg): starts = segments + 1 offsets from 0, points
    // Jacobian in any representative, scalars CANONICAL -> one normalised point per segment.  A term that is not canonical or not on the
    // curve: ZkError(ZK_ERR_INVALID) naming the smallest such term
    G1Vec g1_lincomb_seg(const std::vector<size_t> &starts, const G1Vec &points, const FrVec &scalars_canonical) {
        const size_t segments = starts.empty() ? 0 : starts.size() - 1;
        need(!segments || (points.size() >= starts.back() && scalars_canonical.size() >= starts.back()), "g1_lincomb_seg: fewer terms than the last offset");
        G1Vec out(segments);
        if (segments)
            check(zk_g1_lincomb_seg(h_, segments, starts.data(), points.empty() ? nullptr : points[0].data(),
                                    scalars_canonical.empty() ? nullptr : scalars_canonical[0].v, out[0].data()));
        return out;
    }
    // every opening of `a` in ONE pairing check (zk_pcs_verify_agg); rho: count x 2 u64 explicit weights (tests), nullptr: derived
    bool pcs_verify_agg(const PcsVk &vk, const AggArrays &a, const uint64_t *rho = nullptr) {
        const size_t count = a.count();
        size_t rows = 0;
        for (size_t n : a.nvars) rows += n;
        need(a.skip.size() == count && a.cstart.size() == count + 1 && a.values.size() == count && a.proofs.size() == rows && a.points.size() == rows &&
                 a.cpoints.size() == a.cscalars.size() && a.cpoints.size() >= a.cstart.back(),
             "pcs_verify_agg: the arrays disagree on the number of openings, terms or rows");
        uint8_t ok = 0;
        check(zk_pcs_verify_agg(h_, vk.h, count, a.nvars.data(), a.skip.data(), a.cstart.data(), a.cpoints.empty() ? nullptr : a.cpoints[0].data(),
                                a.cscalars.empty() ? nullptr : a.cscalars[0].v, a.values.empty() ? nullptr : a.values[0].v,
                                a.proofs.empty() ? nullptr : a.proofs[0].data(), a.points.empty() ? nullptr : a.points[0].v, rho, &ok));
        return ok != 0;
    }

    // zk_g1_decompress_check: k x 48 bytes of compressed G1 -> the normalised points and one status per point (0 ok, 1 bad encoding,
    // 2 x not on the curve, 3 not in G1); a bad point is a status, not an error.  The check zk_pcs_verify_batch leaves to its caller
    void g1_decompress_check(const uint8_t *in48, size_t k, G1Vec &points, std::vector<uint8_t> &status) {
        points.assign(k, G1{});
        status.assign(k, 0);
        if (k) check(zk_g1_decompress_check(h_, k, in48, points[0].data(), status.data()));
    }
    // ---- a parameter set from a file (csrc/zk_srsio.hip; zkhost/srs_io.hpp is the caller) ----
    // zk_g1_decompress_check on device memory: count compressed points at in48 -> 96-byte affine records at out96 (as srs_wrap_device takes
    // them); -> { points whose status is not 0, the smallest such index, its status (4: infinity, refused with refuse_infinity) }
    std::array<uint64_t, 3> g1_decompress_check_device(const DevPtr &in48, size_t count, const DevPtr &out96, bool refuse_infinity = false) {
        std::array<uint64_t, 3> res{};
        check(zk_g1_decompress_check_device(h_, count, in48.get(), out96.get(), refuse_infinity ? 1u : 0u, res.data()));
        return res;
    }
    SrsPtr srs_wrap_device(const DevPtr &bases96, size_t n) {
        zk_srs *s = nullptr;
        check(zk_srs_wrap_device(h_, bases96.get(), n, &s));
        return std::make_shared<Srs>(ref_, s);
    }
    // out[j] = level[j] + level[j + m]; ZkError(ZK_ERR_INVALID) when a sum is the point at infinity
    SrsPtr srs_halve(const Srs &level) {
        zk_srs *s = nullptr;
        check(zk_srs_halve(h_, level.handle(), &s));
        return std::make_shared<Srs>(ref_, s);
    }
    // out[j] = the low 128 bits of SHA-256(seed || u32le(domain) || u64le(j)), Montgomery Fr
    DevPtr fr_hash_expand(const uint8_t seed32[32], uint32_t domain, size_t n) {
        DevPtr out = alloc_fr(n);
        check(zk_fr_hash_expand(h_, seed32, domain, n, out.get()));
        return out;
    }
    // relation (B) per level: levels 0 .. n, the n + 1 keys at g2_stride bytes -> ok[k], k < n
    std::vector<uint8_t> srs_check(const std::vector<SrsPtr> &levels, const void *powers_g2, size_t g2_stride, const uint8_t seed32[32]) {
        const size_t n = levels.size() - 1;
        std::vector<const zk_srs *> h(levels.size());
        for (size_t k = 0; k < levels.size(); ++k) h[k] = levels[k]->handle();
        std::vector<uint8_t> ok(n ? n : 1, 0);
        check(zk_srs_check(h_, h.data(), n, powers_g2, g2_stride, seed32, ok.data()));
        ok.resize(n);
        return ok;
    }
    // zk_g1_check: Jacobian points in any representative -> one status per point
    std::vector<uint8_t> g1_check(const G1Vec &points) {
        std::vector<uint8_t> status(points.size(), 0);
        if (!points.empty()) check(zk_g1_check(h_, points.size(), points[0].data(), status.data()));
        return status;
    }
    // zk_g2_decompress_check: k x 96 bytes of compressed G2 -> the affine records and one status per point (0 ok, 1 bad encoding,
    // 2 x not on the twist, 3 not in G2); the check zk_pairing and zk_pcs_vk_create leave to their caller
    void g2_decompress_check(const uint8_t *in96, size_t k, std::vector<G2Rec> &points, std::vector<uint8_t> &status) {
        points.assign(k, G2Rec{});
        status.assign(k, 0);
        if (k) check(zk_g2_decompress_check(h_, k, in96, points[0].data(), status.data()));
    }
    // zk_g2_check: affine records -> one status per point
    std::vector<uint8_t> g2_check(const std::vector<G2Rec> &points) {
        std::vector<uint8_t> status(points.size(), 0);
        if (!points.empty()) check(zk_g2_check(h_, points.size(), points[0].data(), 192, status.data()));
        return status;
    }

    G1Vec g1_lincomb_batch(const G1Vec &points, const FrVec &scalars_canonical, size_t count) {
        size_t n = scalars_canonical.size();
        need(points.size() == n * count, "g1_lincomb_batch: points != count x scalars");
        G1Vec out(count);
        if (count) check(zk_g1_lincomb_batch(h_, points[0].data(), scalars_canonical[0].v, n, count, out[0].data()));
        return out;
    }

    static size_t log2_exact(size_t len) {
        if (!len || (len & (len - 1))) throw ZkError(ZK_ERR_INVALID, "length is not a power of two");
        size_t n = 0;
        while ((size_t(1) << n) < len) ++n;
        return n;
    }

  private:
    static void need(bool ok, const char *what) {
        if (!ok) throw ZkError(ZK_ERR_INVALID, what);
    }
    // The six fused identities (each in a preset-challenge and a transcript-driven form): the name of the preset member, the elements
    // folded out into `last`, the evaluations per round.
    struct Fused {
        const char *name;
        size_t tabs, evals;
    };
    static constexpr Fused kFusedGate{"sumcheck_gate", 7, 5}, kFusedWiring{"sumcheck_wiring", 7, 4}, kFusedPerm3{"sumcheck_perm3", 11, 6},
        kFusedGateWide{"sumcheck_gate_wide", 11, 8}, kFusedLookup{"sumcheck_lookup", 6, 4}, kFusedLookupSel{"sumcheck_lookup_sel", 7, 4};
    // What their twelve members share: the round count checked -- and, for the preset form, the challenge count -- r.sums and `last` sized,
    // then call(sums, last), which lays out the identity's pointers for its C call.  fs: the transcript-driven form, whose member has
    // sized its own `chal` to receive the challenges.
    template <class Call>
    ScResult fused(const Fused &id, bool fs, size_t len, const FrVec &chal, FrVec &last, Call call) {
        const size_t n = log2_exact(len);
        if (n < 1 || (!fs && chal.size() < n)) throw ZkError(ZK_ERR_INVALID, std::string(id.name) + (fs ? "_fs: at least one round" : ": fewer challenges than rounds"));
        ScResult r;
        r.sums.resize(id.evals * n);
        last.assign(id.tabs, Fr::zero());
        check(call(r.sums[0].v, last[0].v));
        return r;
    }
    template <size_t N>
    static std::array<const void *, N> ptrs(const std::array<DevPtr, N> &t) {
        std::array<const void *, N> p;
        for (size_t k = 0; k < N; ++k) p[k] = t[k].get();
        return p;
    }
    template <class F>
    DevPtr binary(F fn, const DevPtr &a, const DevPtr &b, size_t n) {
        DevPtr out = alloc_fr(n);
        check(fn(h_, a.get(), b.get(), out.get(), n));
        return out;
    }
    zk_ctx *h_ = nullptr;
    CtxRef ref_;
};

}  // namespace zkhost
