// zk_pairing.hip -- the BLS12-381 pairing on the device: e(P, Q) values, grouped product checks and the batched verifier of
// PolynomialCommitment (dist-primitive/src/dpoly_comm.rs:466-484).
//
// Layout: one lane per (P, Q) pair, three kernels.
//   k_pairing_miller   f_{|x|,Q}(P): optimal ate over |x| = 0xd201000000010000, Q in homogeneous projective coordinates on the
//                      M-twist, line functions after Costello-Lange-Naehrig / Aranha et al. 2010 (derived in the comments below),
//                      each line multiplied into f as a sparse Fq12.  63 doublings + 5 additions, a fixed trip count: nothing
//                      branches on the data, and degenerate inputs (infinity, off-subgroup points) only produce a wrong value.
//   k_pairing_group    product of the Miller values of each group (one lane per group).
//   k_pairing_final    final exponentiation: easy part (q^6 - 1)(q^2 + 1), hard part the x-chain of Hayashida-Hayasaka-Teruya
//                      (eprint 2020/875) on Granger-Scott cyclotomic squarings; writes the value (ark layout) or a verdict.
// The result is zkhip.pairing.pairing(Q, P) ** ZK_PAIRING_EXP_MULTIPLE (= 3, pairing_consts.cuh): the Miller loop is the
// unconjugated f_{|x|,Q} of zkhip/pairing.py and the HHT chain raises to 3 (q^4 - q^2 + 1) / r.  Lines differ from the affine
// ones of zkhip/pairing.py by factors in Fq4 (Fq2 denominators, the w^3 of the untwisting), which the final exponentiation kills.
//
// The verifier (pcs_verify_batch): by bilinearity  e(C - v g1, g2) = prod_i e(pi_i, s_i g2 - u_i g2)  holds exactly when
//     e(A, g2) * prod_i e(-pi_i, s_i g2) = 1,   A = C - v g1 + sum_i u_i pi_i,
// so every pair uses one of the FIXED points of powers_of_g2; A is one G1 linear combination of nvars + 2 terms per opening
// (host, threads over openings), the nvars + 1 Miller loops and the final exponentiation run here.
#include "fq12.cuh"
#include "host_curve.hpp"
#include "host_fr.hpp"
#include "host_sha256.hpp"
#include "zk_ctx.hpp"

#include <algorithm>
#include <cstring>
#include <thread>
#include <vector>

namespace zk {

static constexpr int kPairBlk = 64;  // one wave per workgroup: the Miller / final-exponentiation lanes are register-bound

// ---- Miller loop -------------------------------------------------------------------------------------------------------------------
// The line through T (tangent) or through T and Q on the twist E': y^2 = x^3 + b', untwisted by (x, y) -> (x / w^2, y / w^3) and
// evaluated at P = (xp, yp), times w^3 (in Fq4: killed by the final exponentiation): with slope lambda on E',
//     w^3 l(P) = (y_T - lambda x_T) + lambda xp w^2 - yp w^3,   w^2 = v, w^3 = v w  ->  slots c0.c0, c0.c1, c1.c1 (f12_mul_by_014).
struct MillerT {
    Fq2x X, Y, Z;
};
struct Line {
    Fq2x c0, c1, c4;
};
// Doubling (T = (X : Y : Z), x_T = X / Z):  lambda = 3 X^2 / (2 Y Z); scaled by 2 Y Z and with X^3 = Y^2 Z - b' Z^3:
//     line = (3 b' Z^2 - Y^2) + 3 X^2 xp v - 2 Y Z yp v w
//     2T   = (2 XY (Y^2 - 9 b' Z^2),  (Y^2 + 9 b' Z^2)^2 - 108 b'^2 Z^4,  8 Y^3 Z)      (4 x arkworks' halved form; projective)
__device__ __noinline__ void miller_dbl(MillerT& T, Line& l, Fq30 xp, Fq30 yp) {
    const Fq2x a = f2_mulr(T.X, T.Y);
    const Fq2x b = f2_sqrr(T.Y);
    const Fq2x c = f2_sqrr(T.Z);
    const Fq2x e = f2_mulr(f2_c(pc::B3_C0, pc::B3_C1), c);  // 3 b' Z^2
    const Fq2x f = f2_addr(f2_dblr(e), e);                  // 9 b' Z^2
    const Fq2x g = f2_addr(b, f);
    const Fq2x h = f2_sub_pair(f2_sqrr(f2_add(T.Y, T.Z)), b, c);  // 2 Y Z
    const Fq2x j = f2_sqrr(T.X);
    const Fq2x e2 = f2_sqrr(e);
    const Fq2x e2x3 = f2_addr(f2_dblr(e2), e2);
    l.c0 = f2_subr(e, b);
    l.c1 = f2_mul_fq(f2_add(f2_add(j, j), j), xp);  // 3 X^2 < 6q
    l.c4 = f2_mul_fq(f2_negr(h), yp);
    T.X = f2_mulr(f2_add(a, a), f2_subr(b, f));
    T.Y = f2_subr(f2_sqrr(g), f2_dblr(f2_dblr(e2x3)));  // g^2 - 12 e^2
    T.Z = f2_dblr(f2_dblr(f2_mulr(b, h)));
}
// Addition of the affine Q = (qx, qy):  theta = Y - qy Z, lambda = X - qx Z (slope theta / lambda); scaled by -lambda:
//     line = (theta qx - lambda qy) - theta xp v + lambda yp v w
__device__ __noinline__ void miller_add(MillerT& T, Line& l, Fq2x qx, Fq2x qy, Fq30 xp, Fq30 yp) {
    const Fq2x theta = f2_subr(T.Y, f2_mulr(qy, T.Z));
    const Fq2x lam = f2_subr(T.X, f2_mulr(qx, T.Z));
    const Fq2x c = f2_sqrr(theta);
    const Fq2x d = f2_sqrr(lam);
    const Fq2x e = f2_mulr(lam, d);
    const Fq2x f = f2_mulr(T.Z, c);
    const Fq2x g = f2_mulr(T.X, d);
    const Fq2x h = f2_r8(f2_sub4(f2_add(e, f), f2_add(g, g)));  // e + f - 2g: < 8q
    l.c0 = f2_r4(f2_add(f2_mulr(theta, qx), f2_negr(f2_mulr(lam, qy))));
    l.c1 = f2_mul_fq(f2_negr(theta), xp);
    l.c4 = f2_mul_fq(lam, yp);
    T.X = f2_mulr(lam, h);
    T.Y = f2_subr(f2_mulr(theta, f2_subr(g, h)), f2_mulr(e, T.Y));
    T.Z = f2_mulr(T.Z, e);
}
__device__ Fq12x miller_loop(const Fq2x& qx, const Fq2x& qy, const Fq30& xp, const Fq30& yp) {
    MillerT T{qx, qy, f2_one()};
    Line l;
    Fq12x f = f12_one();
    for (int i = ZK_PAIRING_ATE_BITS - 2; i >= 0; i--) {
        f = f12_sqr(f);
        miller_dbl(T, l, xp, yp);
        f = f12_mul_by_014(f, l.c0, l.c1, l.c4);
        if ((ZK_PAIRING_ATE_X >> i) & 1) {  // (the bits of the constant: uniform across lanes)
            miller_add(T, l, qx, qy, xp, yp);
            f = f12_mul_by_014(f, l.c0, l.c1, l.c4);
        }
    }
    return f;
}

// ---- final exponentiation ----------------------------------------------------------------------------------------------------------
// f^x for f in the cyclotomic subgroup, x < 0: f^|x| by cyclotomic squarings, then the conjugate (the inverse there)
__device__ __noinline__ Fq12x f12_exp_by_x(Fq12x f) {
    Fq12x r = f;
    for (int i = ZK_PAIRING_ATE_BITS - 2; i >= 0; i--) {
        r = f12_cyc_sqr(r);
        if ((ZK_PAIRING_ATE_X >> i) & 1) r = f12_mul(r, f);
    }
    return f12_conj(r);
}
// f^(3 (q^12 - 1) / r); 0 -> 0
__device__ Fq12x final_exp(const Fq12x& f) {
    Fq12x r = f12_mul(f12_conj(f), f12_inv(f));  // f^(q^6 - 1)
    r = f12_mul(f12_frob<2>(r), r);               // ^(q^2 + 1): now in the cyclotomic subgroup
    // hard part, 3 (q^4 - q^2 + 1) / r = (x - 1)^2 (x + q)(x^2 + q^2 - 1) + 3
    Fq12x y0 = f12_conj(f12_cyc_sqr(r));
    Fq12x y5 = f12_exp_by_x(r);
    Fq12x y1 = f12_cyc_sqr(y5);
    Fq12x y3 = f12_mul(y0, y5);
    y0 = f12_exp_by_x(y3);
    const Fq12x y2 = f12_exp_by_x(y0);
    Fq12x y4 = f12_mul(f12_exp_by_x(y2), y1);
    y1 = f12_mul(f12_mul(f12_exp_by_x(y4), f12_conj(y3)), r);
    y0 = f12_frob<3>(f12_mul(y0, r));
    y4 = f12_frob<1>(f12_mul(y4, f12_conj(r)));
    y5 = f12_frob<2>(f12_mul(y5, y2));
    return f12_mul(f12_mul(f12_mul(y5, y0), y4), y1);
}

// ---- kernels -----------------------------------------------------------------------------------------------------------------------
// g1: n x 96-byte affine records, g2: n x 192-byte affine records (reference Montgomery form, x = y = 0: infinity; both checked on
// their curves by the host).  out: n Fq12 in the internal form (576 bytes each).  A pair with a point at infinity gives 1.
__global__ void __launch_bounds__(kPairBlk) k_pairing_miller(size_t n, const void* __restrict__ g1, const void* __restrict__ g2,
                                                             void* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * kPairBlk + threadIdx.x;
    if (i >= n) return;
    const Fq30 px = f30_load(g1, i * 96), py = f30_load(g1, i * 96 + 48);
    const Aff2 q = aff2_load(g2, i);
    const bool inf = (f30_all_zero(px) && f30_all_zero(py)) || aff2_is_inf(q);
    const Fq2x qx{f30_from_ref(q.x.c0), f30_from_ref(q.x.c1)}, qy{f30_from_ref(q.y.c0), f30_from_ref(q.y.c1)};
    const Fq12x f = miller_loop(qx, qy, f30_from_ref(px), f30_from_ref(py));
    f12_store(out, i, inf ? f12_one() : f);
}
// out[g] = prod_{start[g] <= k < start[g+1]} in[k]  (start checked by the host: non-decreasing, start[groups] <= the values in `in`)
__global__ void __launch_bounds__(kPairBlk) k_pairing_group(size_t groups, const size_t* __restrict__ start, const void* __restrict__ in,
                                                            void* __restrict__ out) {
    const size_t g = (size_t)blockIdx.x * kPairBlk + threadIdx.x;
    if (g >= groups) return;
    Fq12x f = f12_one();
    for (size_t k = start[g]; k < start[g + 1]; k++) f = f12_mul(f, f12_load(in, k));
    f12_store(out, g, f);
}
// mode 0: out = n x 72 u64, the value in ark's layout (Montgomery radix 2^384, canonical);  mode 1: out = n bytes, value == 1
__global__ void __launch_bounds__(kPairBlk) k_pairing_final(size_t n, const void* __restrict__ in, int mode, void* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * kPairBlk + threadIdx.x;
    if (i >= n) return;
    Fq12x r = final_exp(f12_load(in, i));
    if (mode == 0) {
#pragma unroll
        for (int k = 0; k < 12; k++) f30_store(out, i * 576 + 48 * k, f30_to_ref(f12_at(r, k)));
        return;
    }
    u32 diff = 0;
#pragma unroll
    for (int k = 0; k < 12; k++) {
        const Fq30 c = f30_canon8(f12_at(r, k));
#pragma unroll
        for (int m = 0; m < 13; m++) diff |= c.l[m] ^ (k == 0 ? Q30::ONE(m) : 0u);
    }
    reinterpret_cast<unsigned char*>(out)[i] = diff == 0 ? 1 : 0;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
namespace H = zkhost;
static inline size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

// Miller loops of `count` pairs (packed g1 96 B / g2 192 B host records) -> either `count` values (groups == 0; h_out 72 u64 each) or
// the verdicts of `groups` products (h_start: groups + 1 offsets; h_out: groups bytes).  One synchronisation of the ctx stream.
int pairing_run(zk_ctx* ctx, size_t count, const void* h_g1, const void* h_g2, size_t groups, const size_t* h_start, void* h_out) {
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n_out = groups ? groups : count;
    const size_t o_g1 = 0, o_g2 = o_g1 + up256(count * 96), o_f = o_g2 + up256(count * 192), o_st = o_f + up256(count * 576),
                 o_gp = o_st + up256((groups + 1) * sizeof(size_t)), o_out = o_gp + up256(groups * 576), total = o_out + up256(n_out * 576);
    char* d = static_cast<char*>(scratch(ctx, 11, total));
    if (!d) return ZK_ERR_OOM;
    if (count) {
        ZK_HIP(ctx, hipMemcpyAsync(d + o_g1, h_g1, count * 96, hipMemcpyHostToDevice, ctx->stream));
        ZK_HIP(ctx, hipMemcpyAsync(d + o_g2, h_g2, count * 192, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(k_pairing_miller, dim3((unsigned)((count + kPairBlk - 1) / kPairBlk)), dim3(kPairBlk), 0, ctx->stream, count,
                           (const void*)(d + o_g1), (const void*)(d + o_g2), (void*)(d + o_f));
        ZK_HIP(ctx, hipGetLastError());
    }
    const void* fin = d + o_f;
    if (groups) {
        ZK_HIP(ctx, hipMemcpyAsync(d + o_st, h_start, (groups + 1) * sizeof(size_t), hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(k_pairing_group, dim3((unsigned)((groups + kPairBlk - 1) / kPairBlk)), dim3(kPairBlk), 0, ctx->stream, groups,
                           (const size_t*)(d + o_st), (const void*)(d + o_f), (void*)(d + o_gp));
        ZK_HIP(ctx, hipGetLastError());
        fin = d + o_gp;
    }
    hipLaunchKernelGGL(k_pairing_final, dim3((unsigned)((n_out + kPairBlk - 1) / kPairBlk)), dim3(kPairBlk), 0, ctx->stream, n_out, fin,
                       groups ? 1 : 0, (void*)(d + o_out));
    ZK_HIP(ctx, hipGetLastError());
    ZK_HIP(ctx, hipMemcpyAsync(h_out, d + o_out, groups ? groups : count * 576, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ZK_OK;
}

// ---- input checks (host, reference Montgomery form) ----
static const H::Fq& fq_b1() {  // 4 (G1: y^2 = x^3 + 4)
    static const H::Fq b = H::to_mont(H::Fq{4, 0, 0, 0, 0, 0});
    return b;
}
static bool fq_canon(const H::Fq& a) { return !H::geq(a, H::Q); }
// 96-byte record: canonical coordinates on y^2 = x^3 + 4, or x = y = 0
static bool g1_ok(const uint64_t* w) {
    H::Fq x, y;
    H::get_fe(x, w);
    H::get_fe(y, w + 6);
    if (!fq_canon(x) || !fq_canon(y)) return false;
    if (H::is_zero(x) && H::is_zero(y)) return true;
    return H::sqr(y) == H::add(H::mul(H::sqr(x), x), fq_b1());
}
// 192-byte record: on y^2 = x^3 + 4 (1 + u), or all zero
static bool g2_ok(const uint64_t* w) {
    H::Fq2 x, y;
    H::get_fe(x, w);
    H::get_fe(y, w + 12);
    if (!fq_canon(x.c0) || !fq_canon(x.c1) || !fq_canon(y.c0) || !fq_canon(y.c1)) return false;
    if (H::is_zero(x) && H::is_zero(y)) return true;
    const H::Fq2 b2{fq_b1(), fq_b1()};
    return H::sqr(y) == H::add(H::mul(H::sqr(x), x), b2);
}
// G2 records at a caller's stride (192, or the Rust struct's with its flag byte: the flag marks infinity) -> packed 192-byte records
static int pack_g2(zk_ctx* ctx, const void* h_g2, size_t stride, size_t n, std::vector<uint64_t>& out) {
    if (stride < 192) return fail(ctx, ZK_ERR_INVALID, "G2 stride %zu < 192", stride);
    out.assign(n * 24, 0);
    const unsigned char* p = static_cast<const unsigned char*>(h_g2);
    for (size_t i = 0; i < n; i++) {
        const unsigned char* r = p + i * stride;
        if (!(stride > 192 && r[192])) std::memcpy(&out[24 * i], r, 192);
        if (!g2_ok(&out[24 * i])) return fail(ctx, ZK_ERR_INVALID, "G2 point %zu is not on the curve", i);
    }
    return ZK_OK;
}
static int check_g1(zk_ctx* ctx, const void* h_g1, size_t n) {
    const uint64_t* w = static_cast<const uint64_t*>(h_g1);
    for (size_t i = 0; i < n; i++)
        if (!g1_ok(w + 12 * i)) return fail(ctx, ZK_ERR_INVALID, "G1 point %zu is not on the curve", i);
    return ZK_OK;
}

int pairing_values(zk_ctx* ctx, size_t count, const void* h_g1, const void* h_g2, size_t g2_stride, uint64_t* h_out) {
    std::vector<uint64_t> g2;
    int rc = pack_g2(ctx, h_g2, g2_stride, count, g2);
    if (rc) return rc;
    if ((rc = check_g1(ctx, h_g1, count))) return rc;
    if (count == 0) return ZK_OK;
    return pairing_run(ctx, count, h_g1, g2.data(), 0, nullptr, h_out);
}
int pairing_product_check(zk_ctx* ctx, size_t groups, const size_t* h_start, const void* h_g1, const void* h_g2, size_t g2_stride,
                          uint8_t* h_ok) {
    if (groups == 0) return ZK_OK;
    if (h_start[0] != 0) return fail(ctx, ZK_ERR_INVALID, "group offsets must start at 0");
    for (size_t g = 0; g < groups; g++)
        if (h_start[g + 1] < h_start[g]) return fail(ctx, ZK_ERR_INVALID, "group offsets decrease at %zu", g);
    const size_t count = h_start[groups];
    if (count && (!h_g1 || !h_g2)) return fail(ctx, ZK_ERR_INVALID, "null argument");
    std::vector<uint64_t> g2;
    int rc = pack_g2(ctx, h_g2, g2_stride, count, g2);
    if (rc) return rc;
    if ((rc = check_g1(ctx, h_g1, count))) return rc;
    return pairing_run(ctx, count, h_g1, g2.data(), groups, h_start, h_ok);
}

}  // namespace zk

// ---- the verifying key of PolynomialCommitment ----
struct zk_pcs_vk {
    zkhost::Aff g1;                   // powers_of_g[0][0]
    std::vector<uint64_t> g2;         // powers_of_g2, packed 192-byte records
    size_t n_g2 = 0;
};

namespace zk {

int pcs_vk_create(zk_ctx* ctx, const void* h_g1_96, const void* h_powers_g2, size_t g2_stride, size_t n_g2, zk_pcs_vk** out) {
    if (n_g2 < 1) return fail(ctx, ZK_ERR_INVALID, "powers_of_g2 is empty");
    zk_pcs_vk* vk = new zk_pcs_vk();
    int rc = pack_g2(ctx, h_powers_g2, g2_stride, n_g2, vk->g2);
    if (!rc && h_g1_96) rc = check_g1(ctx, h_g1_96, 1);
    if (rc) {
        delete vk;
        return rc;
    }
    if (h_g1_96) {
        H::get_fe(vk->g1.x, static_cast<const uint64_t*>(h_g1_96));
        H::get_fe(vk->g1.y, static_cast<const uint64_t*>(h_g1_96) + 6);
    } else {
        vk->g1 = H::Aff{H::to_mont(H::GX_CANON), H::to_mont(H::GY_CANON)};
    }
    vk->n_g2 = n_g2;
    *out = vk;
    return ZK_OK;
}
void pcs_vk_free(zk_pcs_vk* vk) { delete vk; }

// Fr Montgomery (radix 2^256) -> canonical
static void fr_from_mont(const uint64_t* a, uint64_t* out) {
    static const uint64_t R[4] = {0xffffffff00000001ULL, 0x53bda402fffe5bfeULL, 0x3339d80809a1d805ULL, 0x73eda753299d7d48ULL};
    static const uint64_t RINV = 0xfffffffeffffffffULL;  // -r^-1 mod 2^64
    uint64_t t[5] = {a[0], a[1], a[2], a[3], 0};
    for (int i = 0; i < 4; i++) {  // t = (t + m r) / 2^64, four times
        const uint64_t m = t[0] * RINV;
        H::u128 c = (H::u128)m * R[0] + t[0];
        c >>= 64;
        for (int k = 1; k < 4; k++) {
            c += (H::u128)m * R[k] + t[k];
            t[k - 1] = (uint64_t)c;
            c >>= 64;
        }
        c += t[4];
        t[3] = (uint64_t)c;
        t[4] = (uint64_t)(c >> 64);
    }
    bool ge = t[4] != 0;
    if (!ge) {
        ge = true;
        for (int k = 3; k >= 0; k--) {
            if (t[k] != R[k]) {
                ge = t[k] > R[k];
                break;
            }
        }
    }
    if (ge) {
        uint64_t bw = 0;
        for (int k = 0; k < 4; k++) {
            H::u128 d = (H::u128)t[k] - R[k] - bw;
            t[k] = (uint64_t)d;
            bw = (uint64_t)(d >> 64) & 1;
        }
    }
    std::memcpy(out, t, 32);
}
static void fr_neg_canon(const uint64_t* a, uint64_t* out) {  // r - a (0 -> 0)
    static const uint64_t R[4] = {0xffffffff00000001ULL, 0x53bda402fffe5bfeULL, 0x3339d80809a1d805ULL, 0x73eda753299d7d48ULL};
    if (!(a[0] | a[1] | a[2] | a[3])) {
        std::memset(out, 0, 32);
        return;
    }
    uint64_t bw = 0;
    for (int k = 0; k < 4; k++) {
        H::u128 d = (H::u128)R[k] - a[k] - bw;
        out[k] = (uint64_t)d;
        bw = (uint64_t)(d >> 64) & 1;
    }
}
// Jacobian (18 u64, any representative) -> affine; false if not on the curve / not canonical
static bool jac_in(const uint64_t* w, H::Aff& a) {
    H::Jac j;
    H::get_fe(j.x, w);
    H::get_fe(j.y, w + 6);
    H::get_fe(j.z, w + 12);
    if (!fq_canon(j.x) || !fq_canon(j.y) || !fq_canon(j.z)) return false;
    // the library's results are normalised (z = 1 or 0): no inversion for them
    a = (j.z == H::ONE) ? H::Aff{j.x, j.y} : H::jac_to_aff(j);
    uint64_t rec[12];
    H::put_fe(a.x, rec);
    H::put_fe(a.y, rec + 6);
    return g1_ok(rec);
}

int pcs_verify_batch(zk_ctx* ctx, const zk_pcs_vk* vk, size_t nvars, size_t count, const uint64_t* h_comm, const uint64_t* h_values,
                     const uint64_t* h_proofs, const uint64_t* h_points, uint8_t* h_ok) {
    if (nvars + 1 > vk->n_g2) return fail(ctx, ZK_ERR_INVALID, "nvars + 1 = %zu > %zu powers of g2", nvars + 1, vk->n_g2);
    if (count == 0) return ZK_OK;
    const size_t per = nvars + 1;  // pairs per opening
    // the affine inputs, checked before anything runs
    std::vector<H::Aff> C(count), pi(count * nvars);
    for (size_t k = 0; k < count; k++) {
        if (!jac_in(h_comm + 18 * k, C[k])) return fail(ctx, ZK_ERR_INVALID, "commitment %zu is not on the curve", k);
        for (size_t i = 0; i < nvars; i++)
            if (!jac_in(h_proofs + 18 * (k * nvars + i), pi[k * nvars + i]))
                return fail(ctx, ZK_ERR_INVALID, "proof point %zu of opening %zu is not on the curve", i, k);
    }
    // A_k = C_k + (r - v_k) g1 + sum_i u_ki pi_ki: one joint double-and-add per opening, threads over openings
    std::vector<H::Jac> A(count);
    auto work = [&](size_t k0, size_t k1) {
        std::vector<H::Aff> pts(nvars + 2);
        std::vector<uint64_t> ks(4 * (nvars + 2));
        for (size_t k = k0; k < k1; k++) {
            pts[0] = vk->g1;
            uint64_t v[4];
            fr_from_mont(h_values + 4 * k, v);
            fr_neg_canon(v, &ks[0]);
            for (size_t i = 0; i < nvars; i++) {
                pts[1 + i] = pi[k * nvars + i];
                fr_from_mont(h_points + 4 * (k * nvars + i), &ks[4 * (1 + i)]);
            }
            H::Jac acc = H::jac_inf();
            for (int b = 255; b >= 0; b--) {
                acc = H::jac_dbl(acc);
                for (size_t i = 0; i <= nvars; i++)
                    if ((ks[4 * i + b / 64] >> (b % 64)) & 1) acc = H::jac_add_mixed(acc, pts[i]);
            }
            A[k] = H::jac_add_mixed(acc, C[k]);
        }
    };
    const size_t nth = std::min<size_t>({count, (size_t)std::max(1u, std::thread::hardware_concurrency()), (size_t)16});
    if (nth <= 1) {
        work(0, count);
    } else {
        std::vector<std::thread> th;
        for (size_t t = 0; t < nth; t++) th.emplace_back(work, count * t / nth, count * (t + 1) / nth);
        for (auto& x : th) x.join();
    }
    std::vector<H::Aff> Aa(count);
    H::batch_to_affine(A, Aa.data());
    // pairs: (A_k, g2), (-pi_ki, s_i g2)
    std::vector<uint64_t> g1(count * per * 12), g2(count * per * 24);
    std::vector<size_t> start(count + 1);
    for (size_t k = 0; k < count; k++) {
        start[k] = k * per;
        uint64_t* r = &g1[12 * k * per];
        H::put_fe(Aa[k].x, r);
        H::put_fe(Aa[k].y, r + 6);
        std::memcpy(&g2[24 * k * per], &vk->g2[0], 192);
        for (size_t i = 0; i < nvars; i++) {
            const H::Aff& p = pi[k * nvars + i];
            r = &g1[12 * (k * per + 1 + i)];
            H::put_fe(p.x, r);
            H::put_fe(H::aff_inf(p) ? p.y : H::neg(p.y), r + 6);
            std::memcpy(&g2[24 * (k * per + 1 + i)], &vk->g2[24 * (1 + i)], 192);
        }
    }
    start[count] = count * per;
    return pairing_run(ctx, count * per, g1.data(), g2.data(), count, start.data(), h_ok);
}

// ---- aggregated verification: any number of openings of mixed variable counts, one product of n_g2 pairings -------------------------
// The G2 arguments of every opening are the fixed keys, so with weights rho_k
//     L   = sum_k rho_k (sum_j e_kj C_kj - v_k g1 + sum_i u_ki pi_ki)
//     M_j = sum_{k uses key j} rho_k pi_{k, j-1-skip_k}                      j = 1 .. n_g2 - 1
//     accept  <=>  e(L, g2) prod_j e(-M_j, powers_g2[j]) == 1.
// When every opening holds the product is 1; when one does not it is 1 with probability about count / 2^128 over the weights, which
// are Fiat-Shamir over the whole batch (pcs_agg_weights): the caller cannot choose the openings after the weights.
// L and the M_j are the segments of ONE zk_g1_lincomb_seg call; the host builds its term list with plain Fr arithmetic.

// the offsets of the commitment terms: from 0, non-decreasing
static bool agg_cstart_ok(size_t count, const size_t* h_cstart) {
    if (h_cstart[0] != 0) return false;
    for (size_t k = 0; k < count; k++)
        if (h_cstart[k + 1] < h_cstart[k]) return false;
    return true;
}

int pcs_agg_weights(size_t count, const size_t* h_nvars, const size_t* h_skip, const size_t* h_cstart, const uint64_t* h_cpoints18,
                    const uint64_t* h_cscalars, const uint64_t* h_values, const uint64_t* h_proofs18, const uint64_t* h_points, uint64_t* h_rho) {
    if (count && !agg_cstart_ok(count, h_cstart)) return ZK_ERR_INVALID;
    H::Sha256 seed;
    seed.update("zkhip-pcs-agg-v1", 16);
    seed.update_u64le(count);
    size_t row = 0;  // proof points / point coordinates before opening k
    for (size_t k = 0; k < count; k++) {
        const size_t c0 = h_cstart[k], J = h_cstart[k + 1] - c0, nv = h_nvars[k];
        seed.update_u64le(nv);
        seed.update_u64le(h_skip[k]);
        seed.update_u64le(J);
        if (J) {
            seed.update(h_cpoints18 + 18 * c0, J * 144);
            seed.update(h_cscalars + 4 * c0, J * 32);
        }
        seed.update(h_values + 4 * k, 32);
        if (nv) {
            seed.update(h_proofs18 + 18 * row, nv * 144);
            seed.update(h_points + 4 * row, nv * 32);
        }
        row += nv;
    }
    uint8_t s32[32], d[32];
    seed.digest(s32);
    for (size_t k = 0; k < count; k++) {
        H::Sha256 h;
        h.update(s32, 32);
        h.update_u64le(k);
        h.digest(d);
        for (int w = 0; w < 2; w++) {
            uint64_t v = 0;
            for (int b = 7; b >= 0; b--) v = v << 8 | d[8 * w + b];
            h_rho[2 * k + w] = v;
        }
    }
    return ZK_OK;
}

int pcs_verify_agg(zk_ctx* ctx, const zk_pcs_vk* vk, size_t count, const size_t* h_nvars, const size_t* h_skip, const size_t* h_cstart,
                   const uint64_t* h_cpoints18, const uint64_t* h_cscalars, const uint64_t* h_values, const uint64_t* h_proofs18,
                   const uint64_t* h_points, const uint64_t* h_rho, uint8_t* h_ok) {
    if (count == 0) {
        h_ok[0] = 1;
        return ZK_OK;
    }
    if (!agg_cstart_ok(count, h_cstart)) return fail(ctx, ZK_ERR_INVALID, "commitment term offsets must start at 0 and not decrease");
    const size_t n_g2 = vk->n_g2;
    size_t rows = 0;
    for (size_t k = 0; k < count; k++) {
        if (h_skip[k] >= n_g2 || h_nvars[k] >= n_g2 || 1 + h_skip[k] + h_nvars[k] > n_g2)
            return fail(ctx, ZK_ERR_INVALID, "opening %zu: 1 + skip + nvars = 1 + %zu + %zu > %zu powers of g2", k, h_skip[k], h_nvars[k], n_g2);
        rows += h_nvars[k];
    }
    const size_t cterms = h_cstart[count];
    if ((cterms && (!h_cpoints18 || !h_cscalars)) || (rows && (!h_proofs18 || !h_points))) return fail(ctx, ZK_ERR_INVALID, "null argument");
    std::vector<uint64_t> rho_buf;
    if (!h_rho) {
        rho_buf.resize(2 * count);
        pcs_agg_weights(count, h_nvars, h_skip, h_cstart, h_cpoints18, h_cscalars, h_values, h_proofs18, h_points, rho_buf.data());
        h_rho = rho_buf.data();
    }
    // the term list: segment 0 is L (every G1 point of the input once, then g1), segment j is M_j
    const size_t l_terms = cterms + rows + 1, terms = l_terms + rows;
    std::vector<uint64_t> pts(terms * 18), ks(terms * 4);
    std::vector<size_t> seg(n_g2 + 1, 0), row0(count);
    for (size_t k = 0, row = 0; k < count; row += h_nvars[k], k++) {
        row0[k] = row;
        for (size_t i = 0; i < h_nvars[k]; i++) seg[1 + h_skip[k] + i + 1]++;  // (counts of segment j at seg[j + 1])
    }
    seg[1] = l_terms;
    for (size_t j = 2; j <= n_g2; j++) seg[j] += seg[j - 1];
    std::vector<size_t> fill(seg.begin(), seg.end() - 1);  // the next free term of every segment
    uint64_t vsum[4] = {0, 0, 0, 0};
    for (size_t k = 0; k < count; k++) {
        const uint64_t rho[4] = {h_rho[2 * k], h_rho[2 * k + 1], 0, 0};
        for (size_t c = h_cstart[k]; c < h_cstart[k + 1]; c++) {
            const size_t t = fill[0]++;
            std::memcpy(&pts[18 * t], h_cpoints18 + 18 * c, 144);
            H::fr::mont_mul(rho, h_cscalars + 4 * c, &ks[4 * t]);
        }
        for (size_t i = 0; i < h_nvars[k]; i++) {
            const uint64_t* pi = h_proofs18 + 18 * (row0[k] + i);
            size_t t = fill[0]++;
            std::memcpy(&pts[18 * t], pi, 144);
            H::fr::mont_mul(rho, h_points + 4 * (row0[k] + i), &ks[4 * t]);
            t = fill[1 + h_skip[k] + i]++;
            std::memcpy(&pts[18 * t], pi, 144);
            std::memcpy(&ks[4 * t], rho, 32);
        }
        uint64_t rv[4];
        H::fr::mont_mul(rho, h_values + 4 * k, rv);
        H::fr::add_canon(vsum, rv, vsum);
    }
    {
        const size_t t = fill[0]++;
        H::put_fe(vk->g1.x, &pts[18 * t]);
        H::put_fe(vk->g1.y, &pts[18 * t + 6]);
        H::put_fe(H::aff_inf(vk->g1) ? H::ZERO : H::ONE, &pts[18 * t + 12]);
        fr_neg_canon(vsum, &ks[4 * t]);
    }
    std::vector<uint64_t> sums(n_g2 * 18);
    size_t bad = 0;
    const char* why = "";
    const int rc = g1_lincomb_seg(ctx, n_g2, seg.data(), pts.data(), ks.data(), sums.data(), &bad, &why);
    if (rc == ZK_ERR_INVALID && bad == cterms + rows) return fail(ctx, ZK_ERR_INVALID, "the key's g1: %s", why);
    if (rc == ZK_ERR_INVALID && bad < cterms + rows) {  // every input point is a term of L, in the caller's order within each opening
        size_t k = 0, t0 = 0;
        for (;; k++) {
            const size_t n = (h_cstart[k + 1] - h_cstart[k]) + h_nvars[k];
            if (bad < t0 + n) break;
            t0 += n;
        }
        const size_t J = h_cstart[k + 1] - h_cstart[k];
        if (bad - t0 < J) return fail(ctx, ZK_ERR_INVALID, "commitment term %zu of opening %zu: %s", bad - t0, k, why);
        return fail(ctx, ZK_ERR_INVALID, "proof point %zu of opening %zu: %s", bad - t0 - J, k, why);
    }
    if (rc) return rc;
    // pairs: (L, g2), (-M_j, powers_g2[j])
    std::vector<uint64_t> g1(n_g2 * 12, 0);
    for (size_t j = 0; j < n_g2; j++) {
        const uint64_t* p = &sums[18 * j];
        H::Fq z, y;
        H::get_fe(z, p + 12);
        if (H::is_zero(z)) continue;  // infinity: x = y = 0, a factor 1
        H::get_fe(y, p + 6);
        std::memcpy(&g1[12 * j], p, 48);
        H::put_fe(j ? H::neg(y) : y, &g1[12 * j + 6]);
    }
    const size_t start[2] = {0, n_g2};
    return pairing_run(ctx, n_g2, g1.data(), vk->g2.data(), 1, start, h_ok);
}

}  // namespace zk

// ---- test hooks (include/zkhip_test.h): the field tower one operation at a time -----------------------------------------------------
// They add kernels only: no function above changes.  One lane per element, kPairBlk lanes per workgroup.
namespace zk {

// x + k q by k carry-normalised additions of the limbs of q (k <= 15): every representative below 16q, also those >= 2^384
__device__ __forceinline__ Fq30 dbg_plus_kq(Fq30 x, u32 k) {
    Fq30 q;
#pragma unroll
    for (int i = 0; i < 13; i++) q.l[i] = Q30::Q(i);
    k = k > 15u ? 15u : k;
    for (u32 j = 0; j < k; j++) x = f30_add(x, q);
    return x;
}
__device__ __forceinline__ bool dbg_normalised(const Fq30& v) {  // limbs 0..11 below 2^30
    u32 o = 0;
#pragma unroll
    for (int i = 0; i < 12; i++) o |= v.l[i];
    return (o >> 30) == 0;
}
__device__ __forceinline__ bool dbg_below_2q(const Fq30& v) {  // the borrow chain of f30_csub_2q (wide: no limb can alias)
    long long bw = 0;
#pragma unroll
    for (int i = 0; i < 13; i++) bw = ((long long)v.l[i] - (long long)Q30::Q2(i) - bw) < 0 ? 1 : 0;
    return bw != 0;
}

// x, y: n x 48-byte integers < q (re-limbed, not converted); kx, ky: n u32 <= 15; a = x + kx q, b = y + ky q.
// out: 13 raw limbs per element at a 64-byte stride; flags: bit 0 = the result's limbs 0..11 are below 2^30.  Unary modes do not read y / ky.
enum {
    kF30CsubQ = 0, kF30Csub2Q, kF30Csub4Q, kF30Csub8Q, kF30Red4, kF30Red8, kF30Red16, kF30Canon8,
    kF30Sub2, kF30Sub4, kF30Sub6, kF30Sub8, kF30Sub12, kF30Add, kF30Add2x, kF30Mul, kF30Sqr, kF30Mul2add, kF30Inv, kF30Modes
};
static __host__ __device__ bool dbg_fq30_binary(int mode) { return mode >= kF30Sub2 && mode <= kF30Mul2add && mode != kF30Sqr; }

__global__ void __launch_bounds__(kPairBlk) k_dbg_fq30(size_t n, int mode, const void* __restrict__ x, const u32* __restrict__ kx,
                                                       const void* __restrict__ y, const u32* __restrict__ ky, u32* __restrict__ out,
                                                       u32* __restrict__ flags) {
    const size_t i = (size_t)blockIdx.x * kPairBlk + threadIdx.x;
    if (i >= n) return;
    const Fq30 a = dbg_plus_kq(f30_load(x, i * 48), kx[i]);
    Fq30 b = f30_zero();
    if (dbg_fq30_binary(mode)) b = dbg_plus_kq(f30_load(y, i * 48), ky[i]);
    Fq30 r = f30_zero();
    switch (mode) {
        case kF30CsubQ: r = f30_csub_q(a); break;
        case kF30Csub2Q: r = f30_csub_2q(a); break;
        case kF30Csub4Q: r = f30_csub_4q(a); break;
        case kF30Csub8Q: r = f30_csub_8q(a); break;
        case kF30Red4: r = f30_red4(a); break;
        case kF30Red8: r = f30_red8(a); break;
        case kF30Red16: r = f30_red16(a); break;
        case kF30Canon8: r = f30_canon8(a); break;
        case kF30Sub2: r = f30_sub2(a, b); break;
        case kF30Sub4: r = f30_sub4(a, b); break;
        case kF30Sub6: r = f30_sub6(a, b); break;
        case kF30Sub8: r = f30_sub8(a, b); break;
        case kF30Sub12: r = f30_sub12(a, b); break;
        case kF30Add: r = f30_add(a, b); break;
        case kF30Add2x: r = f30_add2x(a, b); break;
        case kF30Mul: r = f30_mul(a, b); break;
        case kF30Sqr: r = f30_sqr(a); break;
        case kF30Mul2add: r = f30_mul2add(a, b, b, a); break;
        case kF30Inv: r = f30_inv(a); break;
        default: break;
    }
#pragma unroll
    for (int k = 0; k < 16; k++) out[i * 16 + k] = k < 13 ? r.l[k] : 0u;
    flags[i] = dbg_normalised(r) ? 1u : 0u;
}

// a, b: n x 576 bytes, ark's layout (reference Montgomery form, canonical); lift[i]: bits 0..11 add q to those components of a after
// the conversion, bits 12..23 to those of b (same residue, representative < 2q: still inside the bound rule of fq12.cuh).
// out: ark's layout.  flags, taken on the value the function returned, before the conversion back: bit 0 = limbs 0..11 of every
// component below 2^30, bit 1 = every component below 2q.
enum {
    kF12Mul = 0, kF12Sqr, kF12CycSqr, kF12Inv, kF12Conj, kF12Frob1, kF12Frob2, kF12Frob3, kF12MulBy014, kF12ExpByX, kF12FinalExp,
    kF6Mul, kF6Inv, kF2Mul, kF2Sqr, kF2Inv, kF12Modes
};
static __host__ __device__ bool dbg_fq12_binary(int mode) { return mode == kF12Mul || mode == kF12MulBy014 || mode == kF6Mul || mode == kF2Mul; }

__device__ __forceinline__ Fq12x dbg_f12_in(const void* base, size_t idx, u32 lift) {
    Fq12x a;
#pragma unroll
    for (int k = 0; k < 12; k++) f12_at(a, k) = dbg_plus_kq(f30_from_ref(f30_load(base, idx * 576 + 48 * k)), (lift >> k) & 1u);
    return a;
}
__global__ void __launch_bounds__(kPairBlk) k_dbg_fq12(size_t n, int mode, const void* __restrict__ pa, const void* __restrict__ pb,
                                                       const u32* __restrict__ lift, void* __restrict__ out, u32* __restrict__ flags) {
    const size_t i = (size_t)blockIdx.x * kPairBlk + threadIdx.x;
    if (i >= n) return;
    const u32 lf = lift[i];
    const Fq12x a = dbg_f12_in(pa, i, lf & 0xfffu);
    Fq12x b = Fq12x{f6_zero(), f6_zero()};
    if (dbg_fq12_binary(mode)) b = dbg_f12_in(pb, i, (lf >> 12) & 0xfffu);
    Fq12x r = Fq12x{f6_zero(), f6_zero()};  // Fq6 results in c0, Fq2 results in c0.c0
    switch (mode) {
        case kF12Mul: r = f12_mul(a, b); break;
        case kF12Sqr: r = f12_sqr(a); break;
        case kF12CycSqr: r = f12_cyc_sqr(a); break;
        case kF12Inv: r = f12_inv(a); break;
        case kF12Conj: r = f12_conj(a); break;
        case kF12Frob1: r = f12_frob<1>(a); break;
        case kF12Frob2: r = f12_frob<2>(a); break;
        case kF12Frob3: r = f12_frob<3>(a); break;
        case kF12MulBy014: r = f12_mul_by_014(a, b.c0.c0, b.c0.c1, b.c1.c1); break;
        case kF12ExpByX: r = f12_exp_by_x(a); break;
        case kF12FinalExp: r = final_exp(a); break;
        case kF6Mul: r.c0 = f6_mul(a.c0, b.c0); break;
        case kF6Inv: r.c0 = f6_inv(a.c0); break;
        case kF2Mul: r.c0.c0 = f2_mulr(a.c0.c0, b.c0.c0); break;
        case kF2Sqr: r.c0.c0 = f2_sqrr(a.c0.c0); break;
        case kF2Inv: r.c0.c0 = f2_inv(a.c0.c0); break;
        default: break;
    }
    bool norm = true, lt2q = true;
#pragma unroll
    for (int k = 0; k < 12; k++) {
        const Fq30& c = f12_at(r, k);
        norm = norm && dbg_normalised(c);
        lt2q = lt2q && dbg_below_2q(c);
    }
    flags[i] = (norm ? 1u : 0u) | (lt2q ? 2u : 0u);
#pragma unroll
    for (int k = 0; k < 12; k++) f30_store(out, i * 576 + 48 * k, f30_to_ref(f12_at(r, k)));
}

int dbg_fq30_op(zk_ctx* ctx, int mode, const void* d_x, const void* d_kx, const void* d_y, const void* d_ky, void* d_out, void* d_flags,
                size_t n) {
    if (mode < 0 || mode >= kF30Modes) return fail(ctx, ZK_ERR_INVALID, "zk_dbg_fq30_op: unknown mode %d", mode);
    if (n == 0) return ZK_OK;
    if (!d_x || !d_kx || !d_out || !d_flags || (dbg_fq30_binary(mode) && (!d_y || !d_ky))) return fail(ctx, ZK_ERR_INVALID, "null argument");
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_dbg_fq30, dim3((unsigned)((n + kPairBlk - 1) / kPairBlk)), dim3(kPairBlk), 0, ctx->stream, n, mode, d_x,
                       (const u32*)d_kx, d_y, (const u32*)d_ky, (u32*)d_out, (u32*)d_flags);
    ZK_HIP(ctx, hipGetLastError());
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ZK_OK;
}
int dbg_fq12_op(zk_ctx* ctx, int mode, const void* d_a, const void* d_b, const void* d_lift, void* d_out, void* d_flags, size_t n) {
    if (mode < 0 || mode >= kF12Modes) return fail(ctx, ZK_ERR_INVALID, "zk_dbg_fq12_op: unknown mode %d", mode);
    if (n == 0) return ZK_OK;
    if (!d_a || !d_lift || !d_out || !d_flags || (dbg_fq12_binary(mode) && !d_b)) return fail(ctx, ZK_ERR_INVALID, "null argument");
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_dbg_fq12, dim3((unsigned)((n + kPairBlk - 1) / kPairBlk)), dim3(kPairBlk), 0, ctx->stream, n, mode, d_a, d_b,
                       (const u32*)d_lift, d_out, (u32*)d_flags);
    ZK_HIP(ctx, hipGetLastError());
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ZK_OK;
}

}  // namespace zk
