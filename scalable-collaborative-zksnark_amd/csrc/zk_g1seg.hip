// zk_g1seg.hip -- segmented G1 linear combination on the device (zk_g1_lincomb_seg):
//     out[s] = sum over t in [start[s], start[s+1]) of k_t * P_t
// for a few dozen segments of a few to a few thousand terms: the G1 side of an aggregated PCS verification (zk_pcs_verify_agg).
//
//   k_g1seg_terms  one lane per term, one workgroup of 256 lanes per run of up to 256 terms of ONE segment (the host lays the
//                  workgroups out).  The lane checks its point (canonical, Y^2 == X^3 + 4 Z^6: g1c_load_jac), runs a double-and-add
//                  over the `nbits` low bits of its scalar -- nbits is the length of the largest scalar of the call, so the trip
//                  count is the same in every lane -- and the workgroup sums its lanes by a tree in LDS: one partial per workgroup.
//   k_g1seg_sum    one workgroup per segment: the lanes walk the segment's partials with a stride of 256, the same tree sums the
//                  lanes, lane 0 writes the sum in the reference form.
// No workgroup waits on another and no point is updated atomically.  Every addition is the complete one of g1c.cuh: the tree meets equal
// terms, opposite terms and infinities.  A bad term is a status byte, it enters the sum as infinity, and the host refuses the call.
// The scalar stays in memory and is read one 32-bit word per 32 steps: indexing a register array by the bit counter would put it in
// scratch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "g1c.cuh"
#include "host_curve.hpp"
#include "host_fr.hpp"
#include "zk_ctx.hpp"

namespace zk {

namespace g1s {
constexpr int kBlk = 256;
struct Run {  // the terms [first, first + count) of one segment, 1 <= count <= kBlk
    unsigned long long first;
    u32 count, pad;
};
}  // namespace g1s

// The 256 points of a workgroup in LDS, word w of lane t at [w * kBlk + t]: 48 KiB.
__device__ __forceinline__ void g1s_lds_put(u32* lds, int t, const Xyzz30& p) {
    u32 w[12];
    f30_to_words(p.x, w);
#pragma unroll
    for (int k = 0; k < 12; k++) lds[k * g1s::kBlk + t] = w[k];
    f30_to_words(p.y, w);
#pragma unroll
    for (int k = 0; k < 12; k++) lds[(12 + k) * g1s::kBlk + t] = w[k];
    f30_to_words(p.zz, w);
#pragma unroll
    for (int k = 0; k < 12; k++) lds[(24 + k) * g1s::kBlk + t] = w[k];
    f30_to_words(p.zzz, w);
#pragma unroll
    for (int k = 0; k < 12; k++) lds[(36 + k) * g1s::kBlk + t] = w[k];
}
__device__ __forceinline__ Xyzz30 g1s_lds_get(const u32* lds, int t) {
    Xyzz30 p;
    u32 w[12];
#pragma unroll
    for (int k = 0; k < 12; k++) w[k] = lds[k * g1s::kBlk + t];
    p.x = f30_from_words(w);
#pragma unroll
    for (int k = 0; k < 12; k++) w[k] = lds[(12 + k) * g1s::kBlk + t];
    p.y = f30_from_words(w);
#pragma unroll
    for (int k = 0; k < 12; k++) w[k] = lds[(24 + k) * g1s::kBlk + t];
    p.zz = f30_from_words(w);
#pragma unroll
    for (int k = 0; k < 12; k++) w[k] = lds[(36 + k) * g1s::kBlk + t];
    p.zzz = f30_from_words(w);
    return p;
}
// the sum of the values v of lanes 0 .. width - 1 (width a power of two <= kBlk, the same in every lane; lanes beyond it are ignored),
// returned in lane 0.  Each level: the upper half of the live lanes stores, the lower half adds.
__device__ __forceinline__ Xyzz30 g1s_block_sum(u32* lds, int t, int width, Xyzz30 v) {
#pragma unroll 1
    for (int half = width >> 1; half >= 1; half >>= 1) {
        if (t >= half && t < 2 * half) g1s_lds_put(lds, t, v);
        __syncthreads();
        if (t < half) v = g1c_add(v, g1s_lds_get(lds, t + half));
        __syncthreads();
    }
    return v;
}
__device__ __forceinline__ int g1s_width(u32 live) {  // the smallest power of two >= live (1 <= live <= kBlk)
    int w = 1;
    while ((u32)w < live) w <<= 1;
    return w;
}

// points18: terms x 18 u64; scalars: terms x 8 u32 (canonical, little-endian words); status: one byte per term; partials: one flat
// XYZZ record (internal form) per workgroup
static __global__ void __launch_bounds__(g1s::kBlk) k_g1seg_terms(const g1s::Run* __restrict__ runs, int nbits, const void* __restrict__ points18,
                                                                  const u32* __restrict__ scalars, unsigned char* __restrict__ status,
                                                                  void* __restrict__ partials) {
    __shared__ u32 lds[48 * g1s::kBlk];
    const int t = threadIdx.x;
    const g1s::Run run = runs[blockIdx.x];
    Xyzz30 acc;
    xyzz30_set_inf(acc);
    if ((u32)t < run.count) {
        const size_t i = (size_t)run.first + t;
        Xyzz30 base;
        const unsigned char st = g1c_load_jac(points18, i, base);
        status[i] = st;
        if (st == g1c::kOk && !xyzz30_is_inf(base)) {
            const u32* k = scalars + i * 8;
            u32 word = 0;
#pragma unroll 1
            for (int b = nbits - 1; b >= 0; b--) {
                if (b == nbits - 1 || (b & 31) == 31) word = k[b >> 5];
                acc = g1c_dbl(acc);
                if ((word >> (b & 31)) & 1u) acc = g1c_add(acc, base);
            }
        }
    }
    acc = g1s_block_sum(lds, t, g1s_width(run.count), acc);
    if (t == 0) xyzz30_store_flat(partials, blockIdx.x, acc);
}

// wstart: segments + 1 offsets into partials; out: one flat XYZZ record per segment, every coordinate in the reference form (canonical)
static __global__ void __launch_bounds__(g1s::kBlk) k_g1seg_sum(const u32* __restrict__ wstart, const void* __restrict__ partials, void* __restrict__ out) {
    __shared__ u32 lds[48 * g1s::kBlk];
    const int t = threadIdx.x;
    const u32 w0 = wstart[blockIdx.x], w1 = wstart[blockIdx.x + 1];
    Xyzz30 acc;
    xyzz30_set_inf(acc);
#pragma unroll 1
    for (size_t w = (size_t)w0 + t; w < w1; w += g1s::kBlk) {
        Xyzz30 p;
        p.x = f30_load(partials, w * 192);
        p.y = f30_load(partials, w * 192 + 48);
        p.zz = f30_load(partials, w * 192 + 96);
        p.zzz = f30_load(partials, w * 192 + 144);
        acc = g1c_add(acc, p);
    }
    const u32 live = w1 - w0 < (u32)g1s::kBlk ? w1 - w0 : (u32)g1s::kBlk;
    acc = g1s_block_sum(lds, t, g1s_width(live ? live : 1u), acc);
    if (t == 0) {
        const bool inf = xyzz30_is_inf(acc);
        f30_store(out, (size_t)blockIdx.x * 192, inf ? f30_zero() : f30_to_ref(acc.x));
        f30_store(out, (size_t)blockIdx.x * 192 + 48, inf ? f30_zero() : f30_to_ref(acc.y));
        f30_store(out, (size_t)blockIdx.x * 192 + 96, inf ? f30_zero() : f30_to_ref(acc.zz));
        f30_store(out, (size_t)blockIdx.x * 192 + 144, inf ? f30_zero() : f30_to_ref(acc.zzz));
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
namespace H = zkhost;
static inline size_t g1s_up256(size_t b) { return (b + 255) & ~(size_t)255; }

// Stages in scratch arena 11 like zk_g1check.hip and pairing_run: the verifier calls the three back to back and each synchronises the
// ctx stream before it returns.
// h_bad, h_why (optional): the term a ZK_ERR_INVALID names and what is wrong with it, for a caller that knows what its terms are.
int g1_lincomb_seg(zk_ctx* ctx, size_t segments, const size_t* h_start, const uint64_t* h_points18, const uint64_t* h_scalars, uint64_t* h_out18, size_t* h_bad,
                   const char** h_why) {
    if (h_bad) *h_bad = ~(size_t)0;
    if (segments == 0) return ZK_OK;
    if (h_start[0] != 0) return fail(ctx, ZK_ERR_INVALID, "segment offsets must start at 0");
    for (size_t s = 0; s < segments; s++)
        if (h_start[s + 1] < h_start[s]) return fail(ctx, ZK_ERR_INVALID, "segment offsets decrease at %zu", s);
    const size_t terms = h_start[segments];
    if (terms && (!h_points18 || !h_scalars)) return fail(ctx, ZK_ERR_INVALID, "null argument");
    if (segments > 0x7fffffffu || terms > 0x7fffffffu) return fail(ctx, ZK_ERR_INVALID, "zk_g1_lincomb_seg: %zu segments of %zu terms", segments, terms);
    // the scalars: canonical, and the bit length of the largest
    size_t bad_scalar = terms;
    int nbits = 0;
    for (size_t t = 0; t < terms; t++) {
        const uint64_t* k = h_scalars + 4 * t;
        if (!H::fr::canonical(k)) {
            bad_scalar = t;
            break;
        }
        for (int w = 3; w >= 0; w--)
            if (k[w]) {
                const int len = 64 * w + 64 - __builtin_clzll(k[w]);
                if (len > nbits) nbits = len;
                break;
            }
    }
    // one workgroup per run of up to kBlk terms of a segment
    std::vector<g1s::Run> runs;
    std::vector<u32> wstart(segments + 1);
    const size_t checked = bad_scalar < terms ? bad_scalar : terms;  // a bad scalar: only the points before it matter, and only their status
    for (size_t s = 0; s < segments; s++) {
        wstart[s] = (u32)runs.size();
        for (size_t f = h_start[s]; f < h_start[s + 1] && f < checked; f += g1s::kBlk) {
            const size_t end = std::min(std::min(h_start[s + 1], checked), f + (size_t)g1s::kBlk);
            runs.push_back(g1s::Run{(unsigned long long)f, (u32)(end - f), 0u});
        }
    }
    wstart[segments] = (u32)runs.size();
    const size_t nrun = runs.size();
    std::vector<uint64_t> sums(segments * 24, 0);
    std::vector<uint8_t> status(checked ? checked : 1, 0);
    if (nrun) {
        ZK_HIP(ctx, hipSetDevice(ctx->device));
        const size_t o_pts = 0, o_sc = o_pts + g1s_up256(checked * 144), o_run = o_sc + g1s_up256(checked * 32), o_ws = o_run + g1s_up256(nrun * sizeof(g1s::Run)),
                     o_st = o_ws + g1s_up256((segments + 1) * sizeof(u32)), o_part = o_st + g1s_up256(checked), o_out = o_part + g1s_up256(nrun * 192),
                     total = o_out + g1s_up256(segments * 192);
        char* d = static_cast<char*>(scratch(ctx, 11, total));
        if (!d) return ZK_ERR_OOM;
        ZK_HIP(ctx, hipMemcpyAsync(d + o_pts, h_points18, checked * 144, hipMemcpyHostToDevice, ctx->stream));
        ZK_HIP(ctx, hipMemcpyAsync(d + o_sc, h_scalars, checked * 32, hipMemcpyHostToDevice, ctx->stream));
        ZK_HIP(ctx, hipMemcpyAsync(d + o_run, runs.data(), nrun * sizeof(g1s::Run), hipMemcpyHostToDevice, ctx->stream));
        ZK_HIP(ctx, hipMemcpyAsync(d + o_ws, wstart.data(), (segments + 1) * sizeof(u32), hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(k_g1seg_terms, dim3((unsigned)nrun), dim3(g1s::kBlk), 0, ctx->stream, (const g1s::Run*)(d + o_run), nbits, (const void*)(d + o_pts),
                           (const u32*)(d + o_sc), (unsigned char*)(d + o_st), (void*)(d + o_part));
        ZK_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL(k_g1seg_sum, dim3((unsigned)segments), dim3(g1s::kBlk), 0, ctx->stream, (const u32*)(d + o_ws), (const void*)(d + o_part), (void*)(d + o_out));
        ZK_HIP(ctx, hipGetLastError());
        ZK_HIP(ctx, hipMemcpyAsync(status.data(), d + o_st, checked, hipMemcpyDeviceToHost, ctx->stream));
        ZK_HIP(ctx, hipMemcpyAsync(sums.data(), d + o_out, segments * 192, hipMemcpyDeviceToHost, ctx->stream));
        ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    for (size_t t = 0; t < checked; t++)
        if (status[t] != g1c::kOk) {
            const char* why = status[t] == g1c::kBadEncoding ? "a coordinate is not canonical" : "the point is not on the curve";
            if (h_bad) *h_bad = t;
            if (h_why) *h_why = why;
            return fail(ctx, ZK_ERR_INVALID, "term %zu: %s", t, why);
        }
    if (bad_scalar < terms) {
        if (h_bad) *h_bad = bad_scalar;
        if (h_why) *h_why = "the scalar is not canonical";
        return fail(ctx, ZK_ERR_INVALID, "term %zu: the scalar is not canonical", bad_scalar);
    }
    // normalisation on the host: one inversion for all segments
    std::vector<H::Jac> jac(segments);
    for (size_t s = 0; s < segments; s++) {
        H::Fq X, Y, ZZ, ZZZ;
        H::get_fe(X, &sums[24 * s]);
        H::get_fe(Y, &sums[24 * s + 6]);
        H::get_fe(ZZ, &sums[24 * s + 12]);
        H::get_fe(ZZZ, &sums[24 * s + 18]);
        jac[s] = H::xyzz_to_jac(X, Y, ZZ, ZZZ);
    }
    std::vector<H::Aff> aff(segments);
    H::batch_to_affine(jac, aff.data());
    for (size_t s = 0; s < segments; s++) {
        uint64_t* o = h_out18 + 18 * s;
        if (H::is_zero(jac[s].z)) {
            H::put_fe(H::ONE, o);
            H::put_fe(H::ONE, o + 6);
            H::put_fe(H::ZERO, o + 12);
        } else {
            H::put_fe(aff[s].x, o);
            H::put_fe(aff[s].y, o + 6);
            H::put_fe(H::ONE, o + 12);
        }
    }
    return ZK_OK;
}

}  // namespace zk
