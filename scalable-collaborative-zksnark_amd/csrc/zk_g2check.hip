// zk_g2check.hip -- validation of G2 points that come from outside: decompression of the 96-byte zcash / arkworks encoding and
// membership in the prime-order subgroup of the twist E'(Fq2): y^2 = x^3 + 4 (1 + u), one lane per point (zk_g2_decompress_check,
// zk_g2_check).  The shape of zk_g1check.hip:
//
//   k_g2_decompress  96 bytes -> (x, y): flags, x.c0 < q, x.c1 < q, a square root of a = x^3 + 4 (1 + u) in Fq2, y^2 == a, the root the
//                    sign bit names.  The root (q = 3 mod 4; Adj and Rodriguez-Henriquez, "Square root computation over even extension
//                    fields", algorithm 9): a1 = a^((q-3)/4), x0 = a1 a, alpha = a1 x0 = a^((q-1)/2); y = u x0 when alpha = -1, else
//                    y = (1 + alpha)^((q-1)/2) x0.  Two fixed-exponent ladders of 380 steps; the candidate is checked by squaring, which
//                    is also the test for "no root" (the norm test of the algorithm is not needed: a non-square has no candidate that
//                    passes).
//   k_g2_load_aff    24 u64 affine (x.c0 | x.c1 | y.c0 | y.c1, reference Montgomery form, all zero: infinity): canonical coordinates,
//                    y^2 == x^3 + 4 (1 + u)
//   k_g2_subgroup    psi(P) == [x]P = -[|x|]P (Scott, "A note on group membership tests for G1, G2 and GT on BLS pairing-friendly curves"):
//                    psi(x, y) = (c_x conj(x), c_y conj(y)), the untwist-Frobenius-twist map, acts on G2 as q = x (mod r), and on no other
//                    point of the twist like it.  [|x|]P is 63 doublings and 5 additions (|x| = 0xd201000000010000) with the base kept
//                    affine, the comparison is by cross-multiplication: no inversion.
// The first two write the affine point (internal Montgomery form, all zero: infinity) and a status byte; the third reads both and turns a
// status 0 into 3 when the point is outside G2.  Every loop has a constant trip count.
// The group law is xyzz2_dbl / xyzz2_madd of curve30_g2.cuh as they are: both are inlined (G1's doubling sits behind a call, which is why
// g1c.cuh keeps copies) and the mixed addition is complete -- it handles infinity on either side and, when the two x agree, doubles or
// cancels.  A point of order 13 meets those cases inside the ladder; tests/test_gpu_g2check.py holds such points.
#include <hip/hip_runtime.h>

#include <cstring>

#include "g1c.cuh"  // (curve30.cuh first: curve30_g2.cuh builds on it)
#include "curve30_g2.cuh"
#include "zk_ctx.hpp"

namespace zk {

namespace g2c {
// c_x = (1 + u)^(-(q-1)/3) = (0, CX1) and c_y = (1 + u)^(-(q-1)/2) = (CY0, CY1), internal form; derived in tests/g2check_model.py (C_X,
// C_Y), where psi(G2_GEN) == [q mod r] G2_GEN is checked
__host__ __device__ constexpr u32 CX1(int i) {
    constexpr u32 t[13] = {0x1d6270afu, 0x1695e486u, 0x1ad75703u, 0x212543d3u, 0x1e81d8a0u, 0x208dec06u, 0x14cf2934u, 0x35e8c7a0u, 0x2b3f7f82u, 0x2aa53b42u, 0x1c842b9au, 0x06f92997u, 0x000b24beu};
    return t[i];
}
__host__ __device__ constexpr u32 CY0(int i) {
    constexpr u32 t[13] = {0x17305ee1u, 0x27cc5da5u, 0x1dc60d77u, 0x2313e1e6u, 0x01ea792bu, 0x25579b9au, 0x0665f598u, 0x0c4dab7fu, 0x19fe49c7u, 0x1115fea6u, 0x28cdc319u, 0x25b746a4u, 0x000345b7u};
    return t[i];
}
__host__ __device__ constexpr u32 CY1(int i) {
    constexpr u32 t[13] = {0x28cf4bcau, 0x002fa25au, 0x3779f284u, 0x07ec1dc5u, 0x2f0baaf3u, 0x1df2e840u, 0x0ac600dau, 0x06939162u, 0x12d91ab0u, 0x0dc30e88u, 0x00d6eea1u, 0x14d71955u, 0x0016bb5au};
    return t[i];
}
// (q - 3) / 4 (379 bits) and (q - 1) / 2 (380 bits) in 32-bit words; both ladders run 380 steps from 1
__device__ const u32 kSqrtExp[2][12] = {
    {0xffffeaaau, 0xee7fbfffu, 0xac54ffffu, 0x07aaffffu, 0x3dac3d89u, 0xd9cc34a8u, 0x3ce144afu, 0xd91dd2e1u, 0x90d2eb35u, 0x92c6e9edu, 0x8e5ff9a6u, 0x0680447au},
    {0xffffd555u, 0xdcff7fffu, 0x58a9ffffu, 0x0f55ffffu, 0x7b587b12u, 0xb3986950u, 0x79c2895fu, 0xb23ba5c2u, 0x21a5d66bu, 0x258dd3dbu, 0x1cbff34du, 0x0d0088f5u}};
constexpr int kSqrtBits = 380;
constexpr unsigned long long kXAbs = 0xd201000000010000ULL;
constexpr int kBlk = 64;
enum : unsigned char { kOk = 0, kBadEncoding = 1, kNotOnCurve = 2, kNotInG2 = 3 };
}  // namespace g2c

ZK_G1C_CONST(g2c_cx1, g2c::CX1)
ZK_G1C_CONST(g2c_cy0, g2c::CY0)
ZK_G1C_CONST(g2c_cy1, g2c::CY1)
#undef ZK_G1C_CONST

__device__ __forceinline__ bool g2c_same(const Fq2x& a, const Fq2x& b) { return g1c_same(a.c0, b.c0) && g1c_same(a.c1, b.c1); }  // canonical operands
__device__ __forceinline__ Fq2x g2c_b() { return Fq2x{g1c_four(), g1c_four()}; }                                                 // 4 (1 + u)
// x^3 + 4 (1 + u) for a canonical x: < 3q per component
__device__ __forceinline__ Fq2x g2c_rhs(const Fq2x& x) { return f2_add(f2_mul<2>(f2_sqr<2>(x), x), g2c_b()); }
__device__ __forceinline__ void g2c_store_words(void* base, size_t byte_off, int nwords16, u32 v) {  // nwords16 x 16 bytes of v
    uint4* p = reinterpret_cast<uint4*>(reinterpret_cast<char*>(base) + byte_off);
    for (int i = 0; i < nwords16; i++) p[i] = make_uint4(v, v, v, v);
}
// one 192-byte record x.c0 | x.c1 | y.c0 | y.c1
__device__ __forceinline__ void g2c_store_aff(void* out, size_t i, const Fq2x& x, const Fq2x& y) {
    f30_store(out, i * 192, x.c0);
    f30_store(out, i * 192 + 48, x.c1);
    f30_store(out, i * 192 + 96, y.c0);
    f30_store(out, i * 192 + 144, y.c1);
}
// 48 big-endian bytes -> little-endian words: word k of the integer is the byte-swapped word 11 - k of the record
__device__ __forceinline__ void g2c_load_be48(const void* in, size_t byte_off, u32 (&w)[12]) {
    const uint4* p = reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(in) + byte_off);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const uint4 v = p[k];
        w[11 - 4 * k] = __builtin_bswap32(v.x);
        w[10 - 4 * k] = __builtin_bswap32(v.y);
        w[9 - 4 * k] = __builtin_bswap32(v.z);
        w[8 - 4 * k] = __builtin_bswap32(v.w);
    }
}

// in96: count x 96 bytes.  pts: count affine records, internal form (written for status 0 and 3; zero: infinity).  out24: count x 192
// bytes, reference form (zero for status 1, 2 and for infinity).
static __global__ void __launch_bounds__(g2c::kBlk) k_g2_decompress(size_t count, const void* __restrict__ in96, void* __restrict__ pts,
                                                                   void* __restrict__ out24, unsigned char* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * g2c::kBlk + threadIdx.x;
    if (i >= count) return;
    u32 w1[12], w0[12];  // x.c1 comes first
    g2c_load_be48(in96, i * 96, w1);
    g2c_load_be48(in96, i * 96 + 48, w0);
    const bool compressed = (w1[11] >> 31) & 1u, inf = (w1[11] >> 30) & 1u, sign = (w1[11] >> 29) & 1u;
    w1[11] &= 0x1fffffffu;
    u32 any = 0;
#pragma unroll
    for (int k = 0; k < 12; k++) any |= w1[k] | w0[k];
    const Fq2x xc{f30_from_words(w0), f30_from_words(w1)};
    const bool bad = !compressed || (inf ? (sign || any != 0) : !(g1c_lt_q(xc.c0) && g1c_lt_q(xc.c1)));
    if (bad || inf) {
        status[i] = bad ? g2c::kBadEncoding : g2c::kOk;
        g2c_store_words(out24, i * 192, 12, 0u);
        if (!bad) g2c_store_words(pts, i * 192, 12, 0u);
        return;
    }
    const Fq2x x{f30_canon8(f30_mul(xc.c0, g1c_r2())), f30_canon8(f30_mul(xc.c1, g1c_r2()))};  // internal form, canonical
    const Fq2x a = f2_canon8(g2c_rhs(x));
    Fq2x base = a, acc = a, x0 = a;
    bool alpha_is_m1 = false;
#pragma unroll 1
    for (int pass = 0; pass < 2; pass++) {  // acc = base^e: a^((q-3)/4), then (1 + alpha)^((q-1)/2); every value < 2q
        acc = f2_one();
#pragma unroll 1
        for (int b = g2c::kSqrtBits - 1; b >= 0; b--) {
            acc = f2_sqr<2>(acc);
            if ((g2c::kSqrtExp[pass][b >> 5] >> (b & 31)) & 1u) acc = f2_mul<2>(acc, base);  // (the same branch in every lane)
        }
        if (pass == 0) {
            x0 = f2_mul<2>(acc, a);
            const Fq2x alpha = f2_canon8(f2_mul<2>(acc, x0));
            alpha_is_m1 = g1c_same(alpha.c0, f30_neg_canon(f30_one())) && f30_all_zero(alpha.c1);
            base = Fq2x{f30_canon8(f30_add(alpha.c0, f30_one())), alpha.c1};
        }
    }
    Fq2x y = alpha_is_m1 ? Fq2x{f30_negk<2>(x0.c1), x0.c0} : f2_mul<2>(acc, x0);  // u x0, or (1 + alpha)^((q-1)/2) x0
    y = f2_canon8(y);
    if (!g2c_same(f2_canon8(f2_sqr<2>(y)), a)) {
        status[i] = g2c::kNotOnCurve;
        g2c_store_words(out24, i * 192, 12, 0u);
        return;
    }
    // "larger" is a property of the integers: out of Montgomery form; c1 decides, c0 when c1 = 0
    Fq30 unit = f30_zero();
    unit.l[0] = 1;
    const Fq30 p1 = f30_canon8(f30_mul(y.c1, unit)), p0 = f30_canon8(f30_mul(y.c0, unit));
    const bool larger = f30_all_zero(p1) ? g1c_is_larger(p0) : g1c_is_larger(p1);
    if (larger != sign) y = f2_neg_canon(y);
    status[i] = g2c::kOk;
    g2c_store_aff(out24, i, Fq2x{f30_to_ref(x.c0), f30_to_ref(x.c1)}, Fq2x{f30_to_ref(y.c0), f30_to_ref(y.c1)});
    g2c_store_aff(pts, i, x, y);
}

// in24: count x 192 bytes (packed by the host), reference form; all zero is infinity
static __global__ void __launch_bounds__(g2c::kBlk) k_g2_load_aff(size_t count, const void* __restrict__ in24, void* __restrict__ pts,
                                                                 unsigned char* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * g2c::kBlk + threadIdx.x;
    if (i >= count) return;
    const Aff2 r = aff2_load(in24, i);
    if (!(g1c_lt_q(r.x.c0) && g1c_lt_q(r.x.c1) && g1c_lt_q(r.y.c0) && g1c_lt_q(r.y.c1))) {
        status[i] = g2c::kBadEncoding;
        return;
    }
    if (aff2_is_inf(r)) {
        status[i] = g2c::kOk;
        g2c_store_words(pts, i * 192, 12, 0u);
        return;
    }
    const Fq2x x{f30_from_ref(r.x.c0), f30_from_ref(r.x.c1)}, y{f30_from_ref(r.y.c0), f30_from_ref(r.y.c1)};  // canonical
    if (!g2c_same(f2_canon8(f2_sqr<2>(y)), f2_canon8(g2c_rhs(x)))) {
        status[i] = g2c::kNotOnCurve;
        return;
    }
    status[i] = g2c::kOk;
    g2c_store_aff(pts, i, x, y);
}

static __global__ void __launch_bounds__(g2c::kBlk) k_g2_subgroup(size_t count, const void* __restrict__ pts, unsigned char* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * g2c::kBlk + threadIdx.x;
    if (i >= count || status[i] != g2c::kOk) return;
    const Aff2 P = aff2_load(pts, i);
    if (aff2_is_inf(P)) return;  // the neutral element is a member
    Xyzz2 acc;                   // [|x|]P: the top bit, then 63 doublings and 5 additions
    acc.x = P.x;
    acc.y = P.y;
    acc.zz = f2_one();
    acc.zzz = f2_one();
#pragma unroll 1
    for (int b = 62; b >= 0; b--) {
        acc = xyzz2_dbl(acc);
        if ((g2c::kXAbs >> b) & 1ULL) xyzz2_madd(acc, P, false);
    }
    // psi(P) == -acc: (c_x conj(Px), c_y conj(Py)) == (Ax / Azz, -Ay / Azzz), cross-multiplied; infinity is no such point
    bool ok = !xyzz2_is_inf(acc);
    if (ok) {
        const Fq2x cx{f30_zero(), g2c_cx1()}, cy{g2c_cy0(), g2c_cy1()};
        const Fq2x px = f2_mul<2>(cx, Fq2x{P.x.c0, f30_neg_canon(P.x.c1)});    // < 2q
        const Fq2x py = f2_mul<2>(cy, Fq2x{P.y.c0, f30_neg_canon(P.y.c1)});
        const Fq2x l = f2_mul<2>(px, acc.zz);                                  // 2q * (2q + 2q)
        const Fq2x s = f2_add(f2_mul<2>(py, acc.zzz), acc.y);                  // < 2q + 4q
        ok = g2c_same(f2_canon8(l), f2_canon8(acc.x)) && f2_all_zero(f2_canon8(s));
    }
    if (!ok) status[i] = g2c::kNotInG2;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
// Both calls stage in scratch arena 11 like zk_g1check.hip (see there): every user synchronises the ctx stream before it returns.
static inline size_t g2c_up256(size_t b) { return (b + 255) & ~(size_t)255; }

int g2_decompress_check(zk_ctx* ctx, size_t count, const void* h_in96, uint64_t* h_out24, uint8_t* h_status) {
    if (count == 0) return ZK_OK;
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t o_in = 0, o_pts = o_in + g2c_up256(count * 96), o_out = o_pts + g2c_up256(count * 192), o_st = o_out + g2c_up256(count * 192),
                 total = o_st + g2c_up256(count);
    char* d = static_cast<char*>(scratch(ctx, 11, total));
    if (!d) return ZK_ERR_OOM;
    const dim3 grid((unsigned)((count + g2c::kBlk - 1) / g2c::kBlk)), blk(g2c::kBlk);
    ZK_HIP(ctx, hipMemcpyAsync(d + o_in, h_in96, count * 96, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_g2_decompress, grid, blk, 0, ctx->stream, count, (const void*)(d + o_in), (void*)(d + o_pts), (void*)(d + o_out),
                       (unsigned char*)(d + o_st));
    ZK_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_g2_subgroup, grid, blk, 0, ctx->stream, count, (const void*)(d + o_pts), (unsigned char*)(d + o_st));
    ZK_HIP(ctx, hipGetLastError());
    ZK_HIP(ctx, hipMemcpyAsync(h_out24, d + o_out, count * 192, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(ctx, hipMemcpyAsync(h_status, d + o_st, count, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ZK_OK;
}

// records at the caller's stride (192, or the Rust struct's with its flag byte: a nonzero flag marks infinity, as for zk_pairing)
int g2_check(zk_ctx* ctx, size_t count, const void* h_g2, size_t g2_stride, uint8_t* h_status) {
    if (g2_stride < 192) return fail(ctx, ZK_ERR_INVALID, "G2 stride %zu < 192", g2_stride);
    if (count == 0) return ZK_OK;
    const void* src = h_g2;
    std::vector<uint64_t> packed;
    if (g2_stride != 192) {
        packed.assign(count * 24, 0);
        const unsigned char* p = static_cast<const unsigned char*>(h_g2);
        for (size_t i = 0; i < count; i++)
            if (!p[i * g2_stride + 192]) std::memcpy(&packed[24 * i], p + i * g2_stride, 192);
        src = packed.data();
    }
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t o_in = 0, o_pts = o_in + g2c_up256(count * 192), o_st = o_pts + g2c_up256(count * 192), total = o_st + g2c_up256(count);
    char* d = static_cast<char*>(scratch(ctx, 11, total));
    if (!d) return ZK_ERR_OOM;
    const dim3 grid((unsigned)((count + g2c::kBlk - 1) / g2c::kBlk)), blk(g2c::kBlk);
    ZK_HIP(ctx, hipMemcpyAsync(d + o_in, src, count * 192, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_g2_load_aff, grid, blk, 0, ctx->stream, count, (const void*)(d + o_in), (void*)(d + o_pts), (unsigned char*)(d + o_st));
    ZK_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_g2_subgroup, grid, blk, 0, ctx->stream, count, (const void*)(d + o_pts), (unsigned char*)(d + o_st));
    ZK_HIP(ctx, hipGetLastError());
    ZK_HIP(ctx, hipMemcpyAsync(h_status, d + o_st, count, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (packed stays alive until here)
    return ZK_OK;
}

}  // namespace zk
