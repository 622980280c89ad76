// zk_gate.cuh -- what the fused sumchecks (zk_gate.hip: gate identity, zk_wiring.hip: wiring identity, zk_batchopen.hip, zk_perm3.hip, zk_lookup.hip, zk_fs.hip) share: launch geometry, the
// argument blocks of their kernels and the 544-bit lazily reduced sums (one 80-byte slot per wave, evaluation and pass).
#pragma once
#include "fp.cuh"
#include "zk_ctx.hpp"

namespace zk {

static constexpr int kGateBlock = 256;
static constexpr unsigned kGateLocalMax = 512;  // 7 x 512 x 32 B = 112 KiB of the CU's 160 KiB
static constexpr int kGateWideBytes = 80;       // 17 limbs + 3 words of padding (the slot of zk_fr.hip's Wide)
static constexpr int kGateMaxPasses = 40;
static constexpr int kGateMaxLog = 35;         // longest table: 2^35 elements (capacity of the 544-bit sums, see k_gate_pass)

struct GateChal {
    Fr r;
};
struct GateTail {
    uint64_t c[10 * 4];  // challenges of the local stage (at most log2(kGateLocalMax) = 9) / the seed levels of the eq table (10)
};
struct GateReducePlan {
    unsigned nbw[kGateMaxPasses];   // 544-bit partials per sum of pass p (one per wave)
    unsigned off[kGateMaxPasses];   // first slot of pass p in the partials block
};

// The table set of a fused identity of NT tables (zk_perm3.hip, zk_fs.hip): table k, element i, is the Fr at t[k] + 32 (i << sh[k]) --
// sh = 1 reads every other element of the product tree (its views v(x,0) and v(x,1)), sh = 0 an ordinary table.
template <int NT>
struct FsIn {
    const void* t[NT];
    unsigned sh[NT];
};
template <int NT>
struct FsOut {
    void* t[NT];
};

// the batch-opening sumcheck (zk_batchopen.hip, its transcript-driven form in zk_fs.hip)
static constexpr int kMultiMax = 16;  // pairs per call (two pointer blocks of kernel arguments)
// Capacity of the shared sums: the factors of t2 are unreduced sums < 2r, so a product is < 4 r^2 < 2^512 (r < 0.4529 * 2^256) and a
// 544-bit integer holds 2^32 of them; k_multi_reduce adds ALL count * len / 2 products of a round into one, hence
// count * len <= 2^33 (t0 and t1, products of factors < r, are below that).  include/zkhip.h states the bound.
static constexpr int kMultiMaxLog = 33;
static constexpr size_t kMultiLdsBytes = 112 * 1024;  // tables of the local stage (the gate's share of the CU's 160 KiB)

struct MultiIn {
    const void* e[kMultiMax];
    const void* f[kMultiMax];
};
// table (j, which) of the folded set: base + (2 j + which) * stride elements
struct MultiOut {
    void* base;
    size_t stride;
};

__device__ __forceinline__ void gate_wide_add(u32 (&a)[17], const u32 (&b)[17]) {
    u32 c = 0;
#pragma unroll
    for (int i = 0; i < 17; i++) a[i] = addc(a[i], b[i], c);
}
__device__ __forceinline__ void gate_wide_store(void* base, size_t slot, const u32 (&v)[17]) {
    uint4* p = reinterpret_cast<uint4*>(reinterpret_cast<char*>(base) + slot * kGateWideBytes);
#pragma unroll
    for (int i = 0; i < 4; i++) p[i] = make_uint4(v[4 * i], v[4 * i + 1], v[4 * i + 2], v[4 * i + 3]);
    p[4] = make_uint4(v[16], 0, 0, 0);
}
__device__ __forceinline__ void gate_wide_load(u32 (&v)[17], const void* base, size_t slot) {
    const uint4* p = reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(base) + slot * kGateWideBytes);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint4 x = p[i];
        v[4 * i] = x.x, v[4 * i + 1] = x.y, v[4 * i + 2] = x.z, v[4 * i + 3] = x.w;
    }
    v[16] = p[4].x;
}

// the brackets of the two identities (zk_gate.hip / zk_wiring.hip and their transcript-driven forms in zk_fs.hip)
// [ q1 (a + b) + (q2 a) b - c + in ] of one point: three multiplications
__device__ __forceinline__ Fr gate_inner(const Fr& q1, const Fr& q2, const Fr& a, const Fr& b, const Fr& c, const Fr& in) {
    const Fr s = fr_mul(q1, fr_add(a, b));
    const Fr p = fr_mul(fr_mul(q2, a), b);
    return fr_add(fr_sub(fr_add(s, p), c), in);
}

// [ v1x - vx0 vx1 + gamma (den h - num) ] of one point: three multiplications
__device__ __forceinline__ Fr wiring_inner(const Fr& gamma, const Fr& v1x, const Fr& vx0, const Fr& vx1, const Fr& h, const Fr& num, const Fr& den) {
    const Fr p = fr_mul(vx0, vx1);
    const Fr q = fr_mul(gamma, fr_sub(fr_mul(den, h), num));
    return fr_add(fr_sub(v1x, p), q);
}

// the three-column wiring identity (zk_perm3.hip, its transcript-driven form in zk_fs.hip): eq, v1x, vx0, vx1, h, n_0..2, d_0..2
static constexpr int kPerm3Tabs = 11;
static constexpr int kPerm3Evals = 6;             // t = 0 .. 5
static constexpr unsigned kPerm3LocalMax = 256;  // 11 x 256 x 32 B = 88 KiB of the CU's 160 KiB (512 elements would be 176 KiB)

// [ v1x - vx0 vx1 + gamma ( h d_0 d_1 d_2 - n_0 n_1 n_2 ) ] of one point, v in the table order above: seven multiplications
__device__ __forceinline__ Fr perm3_inner(const Fr& gamma, const Fr (&v)[kPerm3Tabs]) {
    const Fr p = fr_mul(v[2], v[3]);
    const Fr dd = fr_mul(fr_mul(fr_mul(v[8], v[9]), v[10]), v[4]);
    const Fr nn = fr_mul(fr_mul(v[5], v[6]), v[7]);
    return fr_add(fr_sub(v[1], p), fr_mul(gamma, fr_sub(dd, nn)));
}

// the wide Plonk gate (zk_gatew.hip, its transcript-driven form in zk_fs.hip): eq, qL, qR, qM, qO, qC, qH, a, b, c, in
static constexpr int kGatewTabs = 11;
static constexpr int kGatewEvals = 8;             // t = 0 .. 7: qH a^5 is degree 6, eq adds one
static constexpr unsigned kGatewLocalMax = 256;  // 11 x 256 x 32 B = 88 KiB of the CU's 160 KiB (512 elements would be 176 KiB)

// [ qL a + qR b + qM a b + qH a^5 - qO c + qC + in ] of one point, v in the table order above: nine multiplications (a^5 as a^2, a^4, a^4 a)
__device__ __forceinline__ Fr gatew_inner(const Fr (&v)[kGatewTabs]) {
    const Fr &a = v[7], &b = v[8];
    const Fr a2 = fr_mul(a, a);
    const Fr a5 = fr_mul(fr_mul(a2, a2), a);
    const Fr lin = fr_add(fr_mul(v[1], a), fr_mul(v[2], b));
    const Fr hi = fr_add(fr_mul(fr_mul(v[3], a), b), fr_mul(v[6], a5));
    return fr_add(fr_add(fr_sub(fr_add(lin, hi), fr_mul(v[4], v[9])), v[5]), v[10]);
}

// the lookup identity (zk_lookup.hip, its transcript-driven form in zk_fs.hip): E, df, dt, m, hf, ht
static constexpr int kLookupTabs = 6;
static constexpr int kLookupEvals = 4;  // t = 0 .. 3

// [ hf df - 1 + gamma ( ht dt - m ) ] of one point: three multiplications
__device__ __forceinline__ Fr lookup_inner(const Fr& gamma, const Fr& df, const Fr& dt, const Fr& m, const Fr& hf, const Fr& ht) {
    const Fr p = fr_sub(fr_mul(hf, df), fp_one<FrCfg>());
    const Fr q = fr_mul(gamma, fr_sub(fr_mul(ht, dt), m));
    return fr_add(p, q);
}
// the selector-gated lookup identity of a Plonk circuit (zk_lookup3.hip, its transcript-driven form in zk_fs.hip): the six tables above, then qk
static constexpr int kLookupSelTabs = 7;

// [ hf df - qk + gamma ( ht dt - m ) ] of one point: three multiplications, qk subtracted as a reduced value
__device__ __forceinline__ Fr lookupsel_inner(const Fr& gamma, const Fr& df, const Fr& dt, const Fr& m, const Fr& hf, const Fr& ht, const Fr& qk) {
    const Fr p = fr_sub(fr_mul(hf, df), qk);
    const Fr q = fr_mul(gamma, fr_sub(fr_mul(ht, dt), m));
    return fr_add(p, q);
}
// A sum of the term of an identity that eq does not multiply (the lookup's hf - ht), a canonical g < r, enters a lazily reduced sum
// as g 2^256: its eight limbs are added from limb 8 on, and the one reduction W0 R^-1 + W1 + W2 R of gate_reduce_value gives it back.
__device__ __forceinline__ void gate_wide_add_hi(u32 (&a)[17], const Fr& g) {
    u32 c = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) a[8 + i] = addc(a[8 + i], g.l[i], c);
    a[16] += c;
}

// One workgroup of kGateBlock lanes adds the nbw per-wave partials from slot `base` on and reduces W0 + W1 R + W2 R^2 (a sum of
// integer products of Montgomery forms) to W0 R^-1 + W1 + W2 R mod r, canonical: the value is lane 0's (the other lanes get zero).
// lds: (kGateBlock / 64) slots, free again after the call's barrier.
__device__ __forceinline__ Fr gate_reduce_value(const void* __restrict__ partials, size_t base, unsigned nbw, uint4* lds) {
    u32 v[17];
#pragma unroll
    for (int i = 0; i < 17; i++) v[i] = 0;
    for (unsigned i = threadIdx.x; i < nbw; i += kGateBlock) {
        u32 x[17];
        gate_wide_load(x, partials, base + i);
        gate_wide_add(v, x);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        u32 o[17];
#pragma unroll
        for (int i = 0; i < 17; i++) o[i] = __shfl_down(v[i], off, 64);
        gate_wide_add(v, o);
    }
    if ((threadIdx.x & 63) == 0) gate_wide_store(lds, threadIdx.x >> 6, v);
    __syncthreads();
    if (threadIdx.x != 0) return fp_zero<FrCfg>();
    for (int g = 1; g < kGateBlock / 64; g++) {
        u32 x[17];
        gate_wide_load(x, lds, g);
        gate_wide_add(v, x);
    }
    Fr w0, w1, w2 = fp_zero<FrCfg>(), one = fp_zero<FrCfg>(), r2;
#pragma unroll
    for (int i = 0; i < 8; i++) w0.l[i] = v[i], w1.l[i] = v[8 + i], r2.l[i] = FrCfg::R2(i);
    w2.l[0] = v[16];
    one.l[0] = 1;
    w0 = fp_reduce_once<FrCfg>(fp_reduce_once<FrCfg>(w0));  // 2^256 < 3 r
    w1 = fp_reduce_once<FrCfg>(fp_reduce_once<FrCfg>(w1));
    return fr_add(fr_add(fr_mul(w0, one), w1), fr_mul(w2, r2));
}
// ... into evals[out]
__device__ __forceinline__ void gate_reduce_block(const void* __restrict__ partials, size_t base, unsigned nbw, uint4* lds, void* __restrict__ evals, size_t out) {
    const Fr s = gate_reduce_value(partials, base, nbw, lds);
    if (threadIdx.x == 0) fr_store(evals, out, s);
}

}  // namespace zk
