// zk_gate.cuh -- what the fused sumchecks share (the preset-challenge engine zk_fused.cuh and its six identities zk_gate.hip, zk_wiring.hip,
// zk_perm3.hip, zk_gatew.hip, zk_lookup.hip, zk_lookup3.hip; zk_batchopen.hip; their transcript-driven forms in zk_fs.hip): launch
// geometry, the argument blocks of the kernels, the 544-bit lazily reduced sums (one 80-byte slot per wave, evaluation and pass), the
// brackets of the identities with the Kind structs that describe them, the blocks every pass and every local stage repeat, and (host
// only) the binding of each identity's caller arguments, written once for its preset-challenge and its transcript-driven entry point.
#pragma once
#include <cstring>

#include "fp.cuh"
#include "zk_ctx.hpp"

namespace zk {

static constexpr int kGateBlock = 256;
static constexpr unsigned kGateLocalMax = 512;  // 7 x 512 x 32 B = 112 KiB of the CU's 160 KiB
static constexpr int kGateWideBytes = 80;       // 17 limbs + 3 words of padding (the slot of zk_fr.hip's Wide)
static constexpr int kGateMaxPasses = 40;
static constexpr int kGateMaxLog = 35;         // longest table: 2^35 elements (capacity of the 544-bit sums, see k_sc_pass in zk_fused.cuh)

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

// The table set of a fused identity of NT tables: table k, element i, is the Fr at t[k] + 32 (i << sh[k]) --
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

// the brackets of the identities
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

// ---------------------------------------------------------------------------------------
// An identity eq(x) [ inner(tables 1 .. kTabs - 1) ] as the engines see it (zk_fused.cuh: preset challenges, zk_fs.hip: challenges from
// a transcript): its table count, the evaluations of a round (degree + 1), the longest table of the local stage (kTabs tables of
// kLocalMax elements fit the CU's LDS), its slot of zk_ctx::preset_lds_raised / fs_lds_raised, the waves per SIMD its pass is compiled
// for, the workgroups per CU its pass is launched with, and the bracket.  kViews: the first tables are shifted views of the product
// tree (FsIn::sh); a Kind without views compiles no shift.  kLoadsFirst: the order of loads and folds in the preset-challenge pass
// (k_sc_pass, zk_fused.cuh).  kFree: the identity has a term free(tables), LINEAR in the tables, that
// eq does not multiply; a lane sums it apart from the products (kind_free_wide says why).
// ---------------------------------------------------------------------------------------
struct GateKind {  // eq, q1, q2, a, b, c, in
    static constexpr int kTabs = 7;
    static constexpr int kEvals = 5;
    static constexpr int kSlot = 0;
    static constexpr unsigned kLocalMax = kGateLocalMax;
    static constexpr int kWaves = 2;
    static constexpr int kPerCu = 2;
    static constexpr bool kViews = false;
    static constexpr bool kLoadsFirst = false;
    static constexpr bool kFree = false;
    __device__ static __forceinline__ Fr inner(const Fr&, const Fr (&v)[kTabs]) { return gate_inner(v[1], v[2], v[3], v[4], v[5], v[6]); }
};
struct WireKind {  // eq, v1x, vx0, vx1, h, num, den
    static constexpr int kTabs = 7;
    static constexpr int kEvals = 4;
    static constexpr int kSlot = 1;
    static constexpr unsigned kLocalMax = kGateLocalMax;
    static constexpr int kWaves = 2;
    static constexpr int kPerCu = 2;
    static constexpr bool kViews = true;
    static constexpr bool kLoadsFirst = true;
    static constexpr bool kFree = false;
    __device__ static __forceinline__ Fr inner(const Fr& gamma, const Fr (&v)[kTabs]) { return wiring_inner(gamma, v[1], v[2], v[3], v[4], v[5], v[6]); }
};
struct Perm3Kind {  // eq, v1x, vx0, vx1, h, n_0, n_1, n_2, d_0, d_1, d_2
    static constexpr int kTabs = kPerm3Tabs;
    static constexpr int kEvals = kPerm3Evals;
    static constexpr int kSlot = 3;
    static constexpr unsigned kLocalMax = kPerm3LocalMax;
    static constexpr int kWaves = 1;  // 22 table registers of 8 limbs and six 17-limb sums: the 264 .. 512 register bracket
    static constexpr int kPerCu = 1;  // one wave per SIMD: one workgroup of four waves fills a CU
    static constexpr bool kViews = true;
    static constexpr bool kLoadsFirst = false;
    static constexpr bool kFree = false;
    __device__ static __forceinline__ Fr inner(const Fr& gamma, const Fr (&v)[kTabs]) { return perm3_inner(gamma, v); }
};
struct GatewKind {  // eq, qL, qR, qM, qO, qC, qH, a, b, c, in
    static constexpr int kTabs = kGatewTabs;
    static constexpr int kEvals = kGatewEvals;
    static constexpr int kSlot = 4;
    static constexpr unsigned kLocalMax = kGatewLocalMax;
    static constexpr int kWaves = 1;  // 22 table registers of 8 limbs and eight 17-limb sums: the 264 .. 512 register bracket
    static constexpr int kPerCu = 1;
    static constexpr bool kViews = false;
    static constexpr bool kLoadsFirst = false;
    static constexpr bool kFree = false;
    __device__ static __forceinline__ Fr inner(const Fr&, const Fr (&v)[kTabs]) { return gatew_inner(v); }
};
struct LookupKind {  // E, df, dt, m, hf, ht
    static constexpr int kTabs = kLookupTabs;
    static constexpr int kEvals = kLookupEvals;
    static constexpr int kSlot = 5;
    static constexpr unsigned kLocalMax = kGateLocalMax;
    static constexpr int kWaves = 2;
    static constexpr int kPerCu = 2;
    static constexpr bool kViews = false;
    static constexpr bool kLoadsFirst = true;
    static constexpr bool kFree = true;  // hf - ht
    __device__ static __forceinline__ Fr inner(const Fr& gamma, const Fr (&v)[kTabs]) { return lookup_inner(gamma, v[1], v[2], v[3], v[4], v[5]); }
    __device__ static __forceinline__ Fr free(const Fr (&v)[kTabs]) { return fr_sub(v[4], v[5]); }
};
struct LookupSelKind {  // E, df, dt, m, hf, ht, qk
    static constexpr int kTabs = kLookupSelTabs;
    static constexpr int kEvals = kLookupEvals;
    static constexpr int kSlot = 6;
    static constexpr unsigned kLocalMax = kGateLocalMax;
    // seven (value, difference) pairs are 112 VGPRs (the transcript-driven fold reads four elements per table: 28 table registers of 8
    // limbs), four 17-limb sums 68, the two sums of hf - ht 16: with the temporaries of a multiplication that is past the 256 registers
    // of two waves per SIMD (the six-table pass sits at 249) -- the 264 .. 512 register bracket
    static constexpr int kWaves = 1;
    static constexpr int kPerCu = 1;
    static constexpr bool kViews = false;
    static constexpr bool kLoadsFirst = true;
    static constexpr bool kFree = true;  // hf - ht
    __device__ static __forceinline__ Fr inner(const Fr& gamma, const Fr (&v)[kTabs]) { return lookupsel_inner(gamma, v[1], v[2], v[3], v[4], v[5], v[6]); }
    __device__ static __forceinline__ Fr free(const Fr (&v)[kTabs]) { return fr_sub(v[4], v[5]); }
};

// ---------------------------------------------------------------------------------------
// The blocks every pass and every local stage repeat.
// ---------------------------------------------------------------------------------------
// One index pair of an HBM pass: v = the tables at lo, d = hi - lo.  The values at t = 1 .. kEvals - 1 come from v(t) = v(t-1) + d; per
// t the reduced multiplications of the bracket and the product with eq, left as a 512-bit integer and added to the 17-limb sum w[t].
// v is stepped in place.
template <class K>
__device__ __forceinline__ void kind_sums_wide(u32 (&w)[K::kEvals][17], const Fr& gamma, Fr (&v)[K::kTabs], const Fr (&d)[K::kTabs]) {
#pragma unroll
    for (int t = 0; t < K::kEvals; t++) {
        fp_mac_wide(w[t], v[0], K::inner(gamma, v));
        if (t + 1 < K::kEvals) {
#pragma unroll
            for (int k = 0; k < K::kTabs; k++) v[k] = fr_add(v[k], d[k]);
        }
    }
}
// The same of a local stage: every sum is a reduced one there, so the free term is added to each point's product as it is.
template <class K>
__device__ __forceinline__ void kind_sums_fr(Fr (&acc)[K::kEvals], const Fr& gamma, Fr (&v)[K::kTabs], const Fr (&d)[K::kTabs]) {
#pragma unroll
    for (int t = 0; t < K::kEvals; t++) {
        Fr p = fr_mul(v[0], K::inner(gamma, v));
        if constexpr (K::kFree) p = fr_add(K::free(v), p);  // off the chain of additions into acc
        acc[t] = fr_add(acc[t], p);
        if (t + 1 < K::kEvals) {
#pragma unroll
            for (int k = 0; k < K::kTabs; k++) v[k] = fr_add(v[k], d[k]);
        }
    }
}
// The free term of a pass (the lookups' hf - ht) is linear in the tables: its value at t is g0 + t gd with g0 = free(lo) and
// gd = free(hi - lo).  A lane keeps the modular sums of g0 and gd over its index pairs (two Fr, canonical) and adds g0 + t gd to sum t
// ONCE, after its loop, as an integer times 2^256 (gate_wide_add_hi): the sums hold raw products of Montgomery forms a R b R and are
// divided by R = 2^256 once, so a Montgomery form g R has to enter as g R 2^256.
// Capacity of the sums: a product is < r^2 < 0.83 * 2^510 and the reduce adds ALL N/2 <= 2^34 products of a pass into one 544-bit
// integer, < 0.83 * 2^544; on top come one term < r 2^256 < 2^511 per LANE, at most 2^17 lanes of a grid: < 2^528.  Hence N <= 2^35
// (kGateMaxLog) as for the identities without such a term.  (One such term per index PAIR would not fit: 2^34 (r^2 + r 2^256) > 2^544.)
template <class K>
__device__ __forceinline__ void kind_free_wide(u32 (&w)[K::kEvals][17], Fr g0, const Fr& gd) {
#pragma unroll
    for (int t = 0; t < K::kEvals; t++) {
        gate_wide_add_hi(w[t], g0);
        g0 = fr_add(g0, gd);
    }
}
// The end of a pass: the NE 17-limb sums of a wave by shuffle, lane 0 stores them.  partials: [t * nbw + 4 block + wave], 80-byte slots.
template <int NE>
__device__ __forceinline__ void gate_wave_store_wide(u32 (&w)[NE][17], void* __restrict__ partials) {
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t nbw = (size_t)gridDim.x * (kGateBlock / 64);
#pragma unroll
    for (int t = 0; t < NE; t++) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            u32 o[17];
#pragma unroll
            for (int i = 0; i < 17; i++) o[i] = __shfl_down(w[t][i], off, 64);
            gate_wide_add(w[t], o);
        }
        if (lane == 0) gate_wide_store(partials, (size_t)t * nbw + (size_t)blockIdx.x * (kGateBlock / 64) + wave, w[t]);
    }
}
// The end of a round of a local stage: the NE reduced sums of a wave by shuffle, lane 0 stores them to LDS.  slots: [wave * NE + t] Fr.
template <int NE>
__device__ __forceinline__ void gate_wave_store_fr(Fr (&acc)[NE], uint4* slots) {
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int t = 0; t < NE; t++) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            Fr o;
#pragma unroll
            for (int i = 0; i < 8; i++) o.l[i] = __shfl_down(acc[t].l[i], off, 64);
            acc[t] = fr_add(acc[t], o);
        }
        if (lane == 0) fr_store(slots, (size_t)wave * NE + t, acc[t]);
    }
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

// hand-over point to the local stage, from a *_local_e knob (1 = HBM passes down to the last element)
static inline int local_e(zk_ctx* ctx, long knob, const char* name, size_t& emax, unsigned local_max = kGateLocalMax) {
    emax = (size_t)knob;
    if (emax < 1 || emax > local_max || (emax & (emax - 1))) return fail(ctx, ZK_ERR_INVALID, "%s must be a power of two in [1, %u]", name, local_max);
    return ZK_OK;
}

// ---------------------------------------------------------------------------------------
// Host only.  What the two entry points of an identity -- preset challenges in its own file, challenges from a transcript in
// zk_fs.hip -- hand their engine (run_preset, run_fs), bound ONCE from the caller's arguments: the tables, gamma (zero for an identity
// without one), the identity's *_local_e knob with its name, and the workgroups per CU of its passes.
// ---------------------------------------------------------------------------------------
template <class K>
struct Bound {
    FsIn<K::kTabs> first;
    GateChal gamma;
    long knob;
    const char* knob_name;
    size_t per_cu;
};
static inline GateChal load_gamma(const uint64_t* h_gamma) {  // null: the identity has no gamma
    GateChal g;
    std::memset(&g, 0, sizeof(g));
    if (h_gamma) std::memcpy(&g.r, h_gamma, 32);
    return g;
}
// a *_pass_wg knob, or the Kind's own kPerCu where the knob is 0
static inline size_t pass_wg(long knob, int per_cu) { return knob > 0 ? (size_t)knob : (size_t)per_cu; }
// plain tables, no shift
template <int NT>
static inline FsIn<NT> plain_tables(const void* const* d_tabs) {
    FsIn<NT> in;
    for (int k = 0; k < NT; k++) in.t[k] = d_tabs[k], in.sh[k] = 0;
    return in;
}
// eq, then the views of the tree -- v1x its upper half, (vx0, vx1) every other element from its base / one element on, h its lower
// half -- then the NT - 5 plain tables of `rest`
template <int NT>
static inline FsIn<NT> tree_tables(const void* d_eq, const void* d_tree, size_t N, const void* const (&rest)[NT - 5]) {
    const char* tree = (const char*)d_tree;
    FsIn<NT> in = {{d_eq, tree + N * 32, tree, tree + 32, tree}, {0, 0, 1, 1, 0}};
    for (int k = 5; k < NT; k++) in.t[k] = rest[k - 5], in.sh[k] = 0;
    return in;
}

static inline Bound<GateKind> bind_gate(const void* const* d_tabs) {
    return {plain_tables<GateKind::kTabs>(d_tabs), load_gamma(nullptr), tuning().gate_local_e, "gate_local_e", pass_wg(tuning().gate_pass_wg, GateKind::kPerCu)};
}
static inline Bound<WireKind> bind_wiring(const void* d_eq, const void* d_tree, const void* d_num, const void* d_den, size_t N, const uint64_t* h_gamma) {
    return {tree_tables<WireKind::kTabs>(d_eq, d_tree, N, {d_num, d_den}), load_gamma(h_gamma), tuning().wiring_local_e, "wiring_local_e",
            pass_wg(tuning().wiring_pass_wg, WireKind::kPerCu)};
}
static inline Bound<Perm3Kind> bind_perm3(const void* d_eq, const void* d_tree, const void* const* d_num, const void* const* d_den, size_t N, const uint64_t* h_gamma) {
    return {tree_tables<kPerm3Tabs>(d_eq, d_tree, N, {d_num[0], d_num[1], d_num[2], d_den[0], d_den[1], d_den[2]}), load_gamma(h_gamma), tuning().perm3_local_e,
            "perm3_local_e", (size_t)Perm3Kind::kPerCu};
}
static inline Bound<GatewKind> bind_gate_wide(const void* const* d_tabs) {
    return {plain_tables<kGatewTabs>(d_tabs), load_gamma(nullptr), tuning().gatew_local_e, "gatew_local_e", (size_t)GatewKind::kPerCu};
}
static inline Bound<LookupKind> bind_lookup(const void* const* d_tabs, const uint64_t* h_gamma) {
    return {plain_tables<kLookupTabs>(d_tabs), load_gamma(h_gamma), tuning().lookup_local_e, "lookup_local_e", (size_t)LookupKind::kPerCu};
}
static inline Bound<LookupSelKind> bind_lookup_sel(const void* const* d_tabs, const uint64_t* h_gamma) {
    return {plain_tables<kLookupSelTabs>(d_tabs), load_gamma(h_gamma), tuning().lookupsel_local_e, "lookupsel_local_e", (size_t)LookupSelKind::kPerCu};
}

}  // namespace zk
