// zk_jubjub.hip -- the Jubjub curve over BLS12-381 Fr and the Schnorr signature "zkhip-schnorr-v1" on the device, one lane per item.
//   K37  on-curve   counts the points that are not on the curve and takes the minimum of their indices (the atomics of zk_srsio.hip)
//   K38  mul        out[i] = [k_i] P_i (or [k_i] G): 256 double-and-add steps in extended coordinates, ONE inversion at the end
//   K39  check      status per point: 0 in the prime-order subgroup, 2 not on the curve, 3 on the curve but [l] P != O
//   K40  verify     status per signature: the four hashes of the challenge, the subgroup test of PK and ONE joint double-and-add over the
//                   bits of s and e with the table {O, G, -PK, G - PK} (Straus), compared with R projectively
//
// The curve (the same in include/zkhip.h, zkhip/jubjub.py and tests/jubjub_model.py): -x^2 + y^2 = 1 + d x^2 y^2 with
// d = -10240 / 10241, a non-square, so the addition law has no exceptional pair of curve points.  A lane keeps a point as (X, Y, Z, T)
// with x = X / Z, y = Y / Z, T = X Y / Z, and adds with the unified a = -1 formulas of Hisil, Wong, Carter and Dawson (2008):
//     A = (Y1 - X1)(Y2 - X2),  B = (Y1 + X1)(Y2 + X2),  C = 2d T1 T2,  D = 2 Z1 Z2,  E = B - A,  F = D - C,  G = D + C,  H = B + A,
//     X3 = E F,  Y3 = G H,  T3 = E H,  Z3 = F G
// -- 9 multiplications, the same text for an addition and a doubling.  -1 is a square in Fr and d is not: the formulas are complete.
//
// Shape.  Every loop has a trip count fixed by the call: 256 ladder steps in K38, 255 in K39 and in each of the two passes of K40
// (s < l < 2^252 and e < r < 2^255).  A ladder step is two passes through ONE copy of the addition (the doubling, then the table
// entry), so a kernel holds the addition once per ladder.  Scalar bits are taken from the top limb while the scalar is shifted left, and table
// entries are chosen by selects on those bits: no private array is indexed by a lane's data.  A lane whose input is refused runs the same
// code on substituted values (the identity) and writes its status at the end.
//
// Bounds.  Lane i touches points[2i], points[2i + 1], scalars[i], out[2i], out[2i + 1], status[i], pk[2i ..], msg[i], sig[3i ..] for i < n only.
// Order.  All launches go on the ctx stream; no workgroup waits on another; the only atomics are K37's count and minimum.
// Registers: DESIGN.md, section 4.
#include "poseidon.cuh"
#include "zk_ctx.hpp"

#include <algorithm>

namespace zk {

namespace jj {
constexpr int kBlock = 256;
constexpr unsigned kMaxBlocks = 1u << 16;  // a grid-stride loop walks longer inputs
enum : u32 { kOk = 0, kScalarRange = 1, kNotOnCurve = 2, kNotInSubgroup = 3, kEquation = 4 };
// Montgomery forms (re-derived from the integers by tests/test_jubjub.py)
__device__ __forceinline__ constexpr u32 D2(int i) {  // 2 d
    constexpr u32 t[8] = {0x72e9ed5fu, 0x54a448acu, 0x1b373967u, 0xa51befdbu, 0x7b4a799eu, 0xc0d81f21u, 0xd27ecf14u, 0x3c0445feu};
    return t[i];
}
__device__ __forceinline__ constexpr u32 GX(int i) {
    constexpr u32 t[8] = {0x1d9d5f3fu, 0x12fbea18u, 0xc2173c77u, 0xbd5f5accu, 0x604c1d4eu, 0x5c37f81cu, 0xa9f250d7u, 0x05aea62fu};
    return t[i];
}
__device__ __forceinline__ constexpr u32 GY(int i) {
    constexpr u32 t[8] = {0xe82a5cf3u, 0xe2394472u, 0x8ad35d0du, 0xea98a73au, 0x16a20624u, 0xd129c57cu, 0x1530eb56u, 0x376ae9a0u};
    return t[i];
}
__device__ __forceinline__ constexpr u32 GT(int i) {  // G.x G.y
    constexpr u32 t[8] = {0x2eb5c914u, 0x59ac1a96u, 0xe56ac104u, 0x39ca396au, 0x8124028bu, 0xb0abbce8u, 0xe21810bdu, 0x65130a8du};
    return t[i];
}
__device__ __forceinline__ constexpr u32 L(int i) {  // the subgroup order, a plain integer
    constexpr u32 t[8] = {0xd6f72cb7u, 0xd0970e5eu, 0xccc81082u, 0xa6682093u, 0x01343b00u, 0x06673b01u, 0x6533afa9u, 0x0e7db4eau};
    return t[i];
}
}  // namespace jj

#define ZK_JJ_CONST(name, limb)                   \
    __device__ __forceinline__ Fr name() {        \
        Fr r;                                     \
        _Pragma("unroll") for (int i = 0; i < 8; i++) r.l[i] = limb(i); \
        return r;                                 \
    }
ZK_JJ_CONST(jj_d2, jj::D2)
ZK_JJ_CONST(jj_gx, jj::GX)
ZK_JJ_CONST(jj_gy, jj::GY)
ZK_JJ_CONST(jj_gt, jj::GT)
ZK_JJ_CONST(jj_l, jj::L)

struct JjPoint {
    Fr x, y, z, t;
};

__device__ __forceinline__ Fr jj_sel(bool c, const Fr& a, const Fr& b) {  // c ? a : b, limb by limb
    Fr r;
#pragma unroll
    for (int i = 0; i < 8; i++) r.l[i] = c ? a.l[i] : b.l[i];
    return r;
}
__device__ __forceinline__ JjPoint jj_sel(bool c, const JjPoint& a, const JjPoint& b) {
    return JjPoint{jj_sel(c, a.x, b.x), jj_sel(c, a.y, b.y), jj_sel(c, a.z, b.z), jj_sel(c, a.t, b.t)};
}
__device__ __forceinline__ JjPoint jj_identity() { return JjPoint{fp_zero<FrCfg>(), fp_one<FrCfg>(), fp_one<FrCfg>(), fp_zero<FrCfg>()}; }
__device__ __forceinline__ JjPoint jj_affine(const Fr& x, const Fr& y) { return JjPoint{x, y, fp_one<FrCfg>(), fr_mul(x, y)}; }
__device__ __forceinline__ JjPoint jj_neg(const JjPoint& p) { return JjPoint{fp_neg<FrCfg>(p.x), p.y, p.z, fp_neg<FrCfg>(p.t)}; }
// (0 : 1 : 1) in any scaling: X = 0 and Y = Z (Z is never 0: the law is complete).  All values are fully reduced
__device__ __forceinline__ bool jj_is_identity(const JjPoint& p) { return fp_is_zero<FrCfg>(p.x) && fp_eq<FrCfg>(p.y, p.z); }

__device__ __forceinline__ JjPoint jj_add(const JjPoint& p, const JjPoint& q) {
    const Fr a = fr_mul(fr_sub(p.y, p.x), fr_sub(q.y, q.x));
    const Fr b = fr_mul(fr_add(p.y, p.x), fr_add(q.y, q.x));
    const Fr c = fr_mul(fr_mul(p.t, q.t), jj_d2());
    const Fr zz = fr_mul(p.z, q.z);
    const Fr d = fr_add(zz, zz);
    const Fr e = fr_sub(b, a), f = fr_sub(d, c), g = fr_add(d, c), h = fr_add(b, a);
    return JjPoint{fr_mul(e, f), fr_mul(g, h), fr_mul(f, g), fr_mul(e, h)};
}

// a < b on 256-bit integers (limbs little-endian)
__device__ __forceinline__ bool jj_less(const Fr& a, const Fr& b) {
    u32 bw = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) subb(a.l[i], b.l[i], bw);
    return bw != 0;
}
__device__ __forceinline__ bool jj_canonical(const Fr& a) {
    Fr p;
#pragma unroll
    for (int i = 0; i < 8; i++) p.l[i] = FrCfg::P(i);
    return jj_less(a, p);
}
// both coordinates below r and 2 (y^2 - x^2 - 1) = 2d x^2 y^2
__device__ __forceinline__ bool jj_on_curve(const Fr& x, const Fr& y) {
    const Fr x2 = fr_mul(x, x), y2 = fr_mul(y, y);
    const Fr lhs = fr_sub(fr_sub(y2, x2), fp_one<FrCfg>());
    return jj_canonical(x) && jj_canonical(y) && fp_eq<FrCfg>(fr_add(lhs, lhs), fr_mul(jj_d2(), fr_mul(x2, y2)));
}
// the top bit of k, and k shifted left by one
__device__ __forceinline__ bool jj_top_bit(Fr& k) {
    const bool bit = k.l[7] >> 31;
#pragma unroll
    for (int i = 7; i > 0; i--) k.l[i] = (k.l[i] << 1) | (k.l[i - 1] >> 31);
    k.l[0] <<= 1;
    return bit;
}

// [k1] T1 + [k2] T2 over the top `steps` bits of k1 and k2 (consumed from bit 255 down); T3 = T1 + T2.  One copy of the addition: the
// inner loop runs it on (acc, acc) and then on (acc, the selected entry)
__device__ __forceinline__ JjPoint jj_ladder2(const JjPoint& T1, const JjPoint& T2, const JjPoint& T3, Fr k1, Fr k2, int steps) {
    JjPoint acc = jj_identity();
#pragma unroll 1
    for (int i = 0; i < steps; i++) {
        const bool b1 = jj_top_bit(k1), b2 = jj_top_bit(k2);
        const JjPoint entry = jj_sel(b2, jj_sel(b1, T3, T2), jj_sel(b1, T1, jj_identity()));
#pragma unroll 1
        for (int half = 0; half < 2; half++) acc = jj_add(acc, jj_sel(half == 0, acc, entry));
    }
    return acc;
}
// [k] P over the top `steps` bits of k
__device__ __forceinline__ JjPoint jj_ladder1(const JjPoint& P, Fr k, int steps) {
    JjPoint acc = jj_identity();
#pragma unroll 1
    for (int i = 0; i < steps; i++) {
        const JjPoint entry = jj_sel(jj_top_bit(k), P, jj_identity());
#pragma unroll 1
        for (int half = 0; half < 2; half++) acc = jj_add(acc, jj_sel(half == 0, acc, entry));
    }
    return acc;
}

// ---------------------------------------------------------------------------------------
// K37.  res[0]: the number of points not on the curve, res[1]: the smallest of their indices
// ---------------------------------------------------------------------------------------
static __global__ void __launch_bounds__(jj::kBlock) k_jj_on_curve(const void* __restrict__ points, size_t n, unsigned long long* __restrict__ res) {
    for (size_t i = (size_t)blockIdx.x * jj::kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * jj::kBlock)
        if (!jj_on_curve(fr_load(points, 2 * i), fr_load(points, 2 * i + 1))) {
            atomicAdd(&res[0], 1ULL);
            atomicMin(&res[1], (unsigned long long)i);
        }
}
// ---------------------------------------------------------------------------------------
// K38.  points: nullptr for the fixed base G.  out may be points: a lane reads its own point before it writes
// ---------------------------------------------------------------------------------------
static __global__ void __launch_bounds__(jj::kBlock) k_jj_mul(const void* points, const void* __restrict__ scalars, void* out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * jj::kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * jj::kBlock) {
        JjPoint P;
        if (points) P = jj_affine(fr_load(points, 2 * i), fr_load(points, 2 * i + 1));  // (wave-uniform)
        else P = JjPoint{jj_gx(), jj_gy(), fp_one<FrCfg>(), jj_gt()};
        const JjPoint acc = jj_ladder1(P, fr_load(scalars, i), 256);
        const Fr zi = fp_inv<FrCfg>(acc.z);
        fr_store(out, 2 * i, fr_mul(acc.x, zi));
        fr_store(out, 2 * i + 1, fr_mul(acc.y, zi));
    }
}
// ---------------------------------------------------------------------------------------
// K39
// ---------------------------------------------------------------------------------------
static __global__ void __launch_bounds__(jj::kBlock) k_jj_check(const void* __restrict__ points, u32* __restrict__ status, size_t n) {
    for (size_t i = (size_t)blockIdx.x * jj::kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * jj::kBlock) {
        const Fr x = fr_load(points, 2 * i), y = fr_load(points, 2 * i + 1);
        const bool on = jj_on_curve(x, y);
        Fr l = jj_l();
        jj_top_bit(l);  // l < 2^252: bit 255 is dropped, 255 steps take the rest
        const JjPoint acc = jj_ladder1(jj_sel(on, jj_affine(x, y), jj_identity()), l, 255);
        status[i] = !on ? jj::kNotOnCurve : jj_is_identity(acc) ? jj::kOk : jj::kNotInSubgroup;
    }
}
// ---------------------------------------------------------------------------------------
// K40.  sig[3i], sig[3i + 1]: R (Montgomery), sig[3i + 2]: s (a plain integer).  Two passes through ONE ladder: pass 0 is [l] PK (table
// {O, PK, -, -}, the second scalar 0), pass 1 is [s] G + [e] (-PK)
// ---------------------------------------------------------------------------------------
static __global__ void __launch_bounds__(jj::kBlock) k_jj_schnorr(const void* __restrict__ consts, u32 half, u32 rp, const void* __restrict__ pk, const void* __restrict__ msg,
                                                                  const void* __restrict__ sig, u32* __restrict__ status, size_t n) {
    for (size_t i = (size_t)blockIdx.x * jj::kBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * jj::kBlock) {
        Fr px = fr_load(pk, 2 * i), py = fr_load(pk, 2 * i + 1), rx = fr_load(sig, 3 * i), ry = fr_load(sig, 3 * i + 1);
        const Fr s = fr_load(sig, 3 * i + 2);
        Fr m = fr_load(msg, i);
        const bool s_ok = jj_less(s, jj_l());
        const bool on = jj_on_curve(px, py) && jj_on_curve(rx, ry);
        const bool pk_id = fp_is_zero<FrCfg>(px) && fp_eq<FrCfg>(py, fp_one<FrCfg>());
        // a refused lane goes on with the identity and 0 (values the arithmetic is defined on); its status is already decided
        px = jj_sel(on, px, fp_zero<FrCfg>()), py = jj_sel(on, py, fp_one<FrCfg>());
        rx = jj_sel(on, rx, fp_zero<FrCfg>()), ry = jj_sel(on, ry, fp_one<FrCfg>());
        const bool m_ok = jj_canonical(m);  // a message that is no field element is signed by nobody: the equation's status
        m = jj_sel(m_ok, m, fp_zero<FrCfg>());
        // e = hash2(hash2(hash2(R.x, R.y), hash2(PK.x, PK.y)), m): four passes through ONE copy of the permutation
        Fr h0 = fp_zero<FrCfg>(), e = fp_zero<FrCfg>();
#pragma unroll 1
        for (int j = 0; j < 4; j++) {  // (j is wave-uniform)
            const Fr left = j == 0 ? rx : j == 1 ? px : j == 2 ? h0 : e;
            const Fr right = j == 0 ? ry : j == 1 ? py : j == 2 ? e : m;
            const Fr h = pos_hash2(consts, half, rp, left, right);
            if (j == 0) h0 = h;
            else e = h;
        }
        const JjPoint PK = jj_affine(px, py), G = JjPoint{jj_gx(), jj_gy(), fp_one<FrCfg>(), jj_gt()};
        const JjPoint nPK = jj_neg(PK), GnPK = jj_add(G, nPK);
        Fr k_s = s, k_e = fp_from_mont<FrCfg>(e), k_l = jj_l();
        jj_top_bit(k_s), jj_top_bit(k_e), jj_top_bit(k_l);  // bit 255 of each is 0 (s is taken as 0 .. 2^255 - 1 when it is refused anyway)
        bool in_group = false, equal = false;
#pragma unroll 1
        for (int pass = 0; pass < 2; pass++) {  // (wave-uniform)
            const JjPoint acc = jj_ladder2(pass ? G : PK, nPK, GnPK, pass ? k_s : k_l, pass ? k_e : fp_zero<FrCfg>(), 255);
            if (pass == 0) in_group = jj_is_identity(acc);
            else equal = fp_eq<FrCfg>(acc.x, fr_mul(rx, acc.z)) && fp_eq<FrCfg>(acc.y, fr_mul(ry, acc.z));
        }
        status[i] = !s_ok ? jj::kScalarRange : !on ? jj::kNotOnCurve : (pk_id || !in_group) ? jj::kNotInSubgroup : (equal && m_ok) ? jj::kOk : jj::kEquation;
    }
}

static unsigned jj_blocks(size_t n) { return (unsigned)std::min<size_t>((n + jj::kBlock - 1) / jj::kBlock, jj::kMaxBlocks); }

int jubjub_mul(zk_ctx* ctx, const void* d_points, const void* d_scalars, void* d_out, size_t n) {
    if (n == 0) return ZK_OK;
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    if (d_points) {  // the count and the minimum live in scratch arena 11 (zk_srsio.hip): every user synchronises the ctx stream before it returns
        unsigned long long* d_res = static_cast<unsigned long long*>(scratch(ctx, 11, 256));
        if (!d_res) return ZK_ERR_OOM;
        ZK_HIP(ctx, hipMemsetAsync(d_res, 0, 8, ctx->stream));
        ZK_HIP(ctx, hipMemsetAsync(d_res + 1, 0xff, 8, ctx->stream));
        hipLaunchKernelGGL(k_jj_on_curve, dim3(jj_blocks(n)), dim3(jj::kBlock), 0, ctx->stream, d_points, n, d_res);
        ZK_HIP(ctx, hipGetLastError());
        unsigned long long res[2] = {0, 0};
        ZK_HIP(ctx, hipMemcpyAsync(res, d_res, 16, hipMemcpyDeviceToHost, ctx->stream));
        ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (res[0]) return fail(ctx, ZK_ERR_INVALID, "zk_jubjub_mul: %llu of %zu points are not on the curve; the first is %llu", res[0], n, res[1]);
    }
    hipLaunchKernelGGL(k_jj_mul, dim3(jj_blocks(n)), dim3(jj::kBlock), 0, ctx->stream, d_points, d_scalars, d_out, n);
    ZK_HIP(ctx, hipGetLastError());
    return ZK_OK;
}
int jubjub_check(zk_ctx* ctx, const void* d_points, uint32_t* d_status, size_t n) {
    if (n == 0) return ZK_OK;
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_jj_check, dim3(jj_blocks(n)), dim3(jj::kBlock), 0, ctx->stream, d_points, d_status, n);
    ZK_HIP(ctx, hipGetLastError());
    return ZK_OK;
}
int schnorr_verify(zk_ctx* ctx, const zk_poseidon_params* p, const void* d_pk, const void* d_msg, const void* d_sig, uint32_t* d_status, size_t n) {
    if (p->ctx != ctx) return fail(ctx, ZK_ERR_INVALID, "zk_schnorr_verify: the params belong to another ctx");
    if (n == 0) return ZK_OK;
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_jj_schnorr, dim3(jj_blocks(n)), dim3(jj::kBlock), 0, ctx->stream, p->d_consts, p->half, p->rp, d_pk, d_msg, d_sig, d_status, n);
    ZK_HIP(ctx, hipGetLastError());
    return ZK_OK;
}

}  // namespace zk
