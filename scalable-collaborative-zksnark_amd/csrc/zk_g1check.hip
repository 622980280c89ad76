// zk_g1check.hip -- validation of G1 points that come from outside: decompression of the 48-byte zcash / arkworks encoding and
// membership in the prime-order subgroup, one lane per point (zk_g1_decompress_check, zk_g1_check).
//
//   k_g1_decompress  48 bytes -> (x, y): flags, x < q, y = (x^3 + 4)^((q+1)/4), y^2 == x^3 + 4, the root the sign bit names
//   k_g1_load_jac    18 u64 Jacobian (any representative) -> XYZZ: canonical coordinates, Y^2 == X^3 + 4 Z^6
//   k_g1_subgroup    phi(P) == -[x^2]P  (Scott, "A note on group membership tests for G1, G2 and GT on BLS pairing-friendly curves"):
//                    phi(x, y) = (beta x, y) acts on G1 as the root -x^2 of l^2 + l + 1 (x^4 - x^2 + 1 = r), and on no other point of
//                    E(Fq) like it.  [x^2]P is two passes of 63 doublings and 5 additions (|x| = 0xd201000000010000), the comparison
//                    is by cross-multiplication: no inversion.
// The first two write the point as a flat XYZZ record (internal Montgomery form) and a status byte; the third reads both and turns a
// status 0 into 3 when the point is outside G1.  Two kernels, not one: the square root is a chain of field elements (3 live values),
// the scalar multiplication holds three points (12); kept apart each is allocated for what it needs, and zk_g1_check runs the second
// one only.  Every loop has a constant trip count: the exponent and the scalar are constants, no input can make a lane spin.
// The additions are complete (equal operands, opposite operands, infinity on either side): a point of order 3 has 2T = -T and meets
// those cases in the first steps of the ladder.
#include <hip/hip_runtime.h>

#include "g1c.cuh"
#include "zk_ctx.hpp"

namespace zk {

namespace g1c {
constexpr int kBlk = 64;
}  // namespace g1c

#undef ZK_G1C_CONST

__device__ __forceinline__ void g1c_store_words(void* base, size_t byte_off, int nwords16, u32 v) {  // nwords16 x 16 bytes of v
    uint4* p = reinterpret_cast<uint4*>(reinterpret_cast<char*>(base) + byte_off);
    for (int i = 0; i < nwords16; i++) p[i] = make_uint4(v, v, v, v);
}
// the 18-word result record: (x, y, 1), or (1, 1, 0) for infinity, reference Montgomery form
__device__ __forceinline__ void g1c_store_jac(void* out, size_t i, const Fq30& x_ref, const Fq30& y_ref, bool inf) {
    const Fq30 one = g1c_one_ref();
    f30_store(out, i * 144, inf ? one : x_ref);
    f30_store(out, i * 144 + 48, inf ? one : y_ref);
    f30_store(out, i * 144 + 96, inf ? f30_zero() : one);
}

// (the complete doubling and addition g1c_dbl / g1c_add are in g1c.cuh: zk_g1seg.hip uses them too.  Its g1c_load_jac is the rule of
// k_g1_load_jac below for a lane that keeps the point in registers; this kernel stores as it goes and keeps its own text.)

// in48: count x 48 bytes.  pts: count flat XYZZ records (written for status 0 and 3).  out18: count x 144 bytes (zero for status 1, 2).
static __global__ void __launch_bounds__(g1c::kBlk) k_g1_decompress(size_t count, const void* __restrict__ in48, void* __restrict__ pts,
                                                                   void* __restrict__ out18, unsigned char* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * g1c::kBlk + threadIdx.x;
    if (i >= count) return;
    Fq30 x, y;
    bool inf;
    const unsigned char st = g1c_decompress(in48, i, x, y, inf);  // (the rule itself is in g1c.cuh: zk_srsio.hip runs it too)
    if (st != g1c::kOk || inf) {
        status[i] = st;
        if (st != g1c::kOk) {
            g1c_store_words(out18, i * 144, 9, 0u);
        } else {
            g1c_store_jac(out18, i, f30_zero(), f30_zero(), true);
            g1c_store_words(pts, i * 192, 12, 0u);  // ZZ = 0: infinity
        }
        return;
    }
    status[i] = g1c::kOk;
    g1c_store_jac(out18, i, f30_to_ref(x), f30_to_ref(y), false);
    f30_store(pts, i * 192, x);
    f30_store(pts, i * 192 + 48, y);
    f30_store(pts, i * 192 + 96, f30_one());
    f30_store(pts, i * 192 + 144, f30_one());
}

// in18: count x 18 u64 (X, Y, Z), reference Montgomery form.  Z = 0 is infinity whatever X and Y are (as in zk_pcs_verify_batch).
static __global__ void __launch_bounds__(g1c::kBlk) k_g1_load_jac(size_t count, const void* __restrict__ in18, void* __restrict__ pts,
                                                                 unsigned char* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * g1c::kBlk + threadIdx.x;
    if (i >= count) return;
    const Fq30 xr = f30_load(in18, i * 144), yr = f30_load(in18, i * 144 + 48), zr = f30_load(in18, i * 144 + 96);
    if (!g1c_lt_q(xr) || !g1c_lt_q(yr) || !g1c_lt_q(zr)) {
        status[i] = g1c::kBadEncoding;
        return;
    }
    if (f30_all_zero(zr)) {
        status[i] = g1c::kOk;
        g1c_store_words(pts, i * 192, 12, 0u);
        return;
    }
    const Fq30 X = f30_from_ref(xr), Y = f30_from_ref(yr), Z = f30_from_ref(zr);  // canonical
    const Fq30 ZZ = f30_sqr(Z), ZZZ = f30_mul(ZZ, Z);                            // < 2q
    // Y^2 == X^3 + 4 Z^6
    const Fq30 rhs = f30_mul2add(f30_sqr(X), X, f30_sqr(ZZZ), g1c_four());
    if (!g1c_same(f30_canon8(f30_sqr(Y)), f30_canon8(rhs))) {
        status[i] = g1c::kNotOnCurve;
        return;
    }
    status[i] = g1c::kOk;
    f30_store(pts, i * 192, X);  // (X, Y, Z^2, Z^3) is the XYZZ form of the same point
    f30_store(pts, i * 192 + 48, Y);
    f30_store(pts, i * 192 + 96, ZZ);
    f30_store(pts, i * 192 + 144, ZZZ);
}

static __global__ void __launch_bounds__(g1c::kBlk) k_g1_subgroup(size_t count, const void* __restrict__ pts, unsigned char* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * g1c::kBlk + threadIdx.x;
    if (i >= count || status[i] != g1c::kOk) return;
    Xyzz30 P;
    P.x = f30_load(pts, i * 192);
    P.y = f30_load(pts, i * 192 + 48);
    P.zz = f30_load(pts, i * 192 + 96);
    P.zzz = f30_load(pts, i * 192 + 144);
    if (xyzz30_is_inf(P)) return;  // the neutral element is a member
    if (!g1c_in_subgroup(P)) status[i] = g1c::kNotInG1;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
// Both calls stage in scratch arena 11, the one pairing_run (zk_pairing.hip) uses: a verifier calls them back to back with the pairing,
// every user synchronises the ctx stream before it returns, and an arena only ever grows -- so the few KiB needed here are always
// inside what the pairing of the same proof allocates, and no call sees another's data in flight.
static inline size_t g1c_up256(size_t b) { return (b + 255) & ~(size_t)255; }

int g1_decompress_check(zk_ctx* ctx, size_t count, const void* h_in48, uint64_t* h_out18, uint8_t* h_status) {
    if (count == 0) return ZK_OK;
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t o_in = 0, o_pts = o_in + g1c_up256(count * 48), o_out = o_pts + g1c_up256(count * 192), o_st = o_out + g1c_up256(count * 144),
                 total = o_st + g1c_up256(count);
    char* d = static_cast<char*>(scratch(ctx, 11, total));
    if (!d) return ZK_ERR_OOM;
    const dim3 grid((unsigned)((count + g1c::kBlk - 1) / g1c::kBlk)), blk(g1c::kBlk);
    ZK_HIP(ctx, hipMemcpyAsync(d + o_in, h_in48, count * 48, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_g1_decompress, grid, blk, 0, ctx->stream, count, (const void*)(d + o_in), (void*)(d + o_pts), (void*)(d + o_out),
                       (unsigned char*)(d + o_st));
    ZK_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_g1_subgroup, grid, blk, 0, ctx->stream, count, (const void*)(d + o_pts), (unsigned char*)(d + o_st));
    ZK_HIP(ctx, hipGetLastError());
    ZK_HIP(ctx, hipMemcpyAsync(h_out18, d + o_out, count * 144, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(ctx, hipMemcpyAsync(h_status, d + o_st, count, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ZK_OK;
}

int g1_check(zk_ctx* ctx, size_t count, const uint64_t* h_points18, uint8_t* h_status) {
    if (count == 0) return ZK_OK;
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t o_in = 0, o_pts = o_in + g1c_up256(count * 144), o_st = o_pts + g1c_up256(count * 192), total = o_st + g1c_up256(count);
    char* d = static_cast<char*>(scratch(ctx, 11, total));
    if (!d) return ZK_ERR_OOM;
    const dim3 grid((unsigned)((count + g1c::kBlk - 1) / g1c::kBlk)), blk(g1c::kBlk);
    ZK_HIP(ctx, hipMemcpyAsync(d + o_in, h_points18, count * 144, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_g1_load_jac, grid, blk, 0, ctx->stream, count, (const void*)(d + o_in), (void*)(d + o_pts), (unsigned char*)(d + o_st));
    ZK_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_g1_subgroup, grid, blk, 0, ctx->stream, count, (const void*)(d + o_pts), (unsigned char*)(d + o_st));
    ZK_HIP(ctx, hipGetLastError());
    ZK_HIP(ctx, hipMemcpyAsync(h_status, d + o_st, count, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ZK_OK;
}

}  // namespace zk
