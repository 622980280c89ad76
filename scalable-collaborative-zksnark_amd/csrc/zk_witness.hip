// zk_witness.hip -- Plonk witness generation and the witness check on the device, per proof, on the plan of zk_witness.cpp.
//   K22  level   one lane per row of ONE level of more than kWitBlock rows: gather a and b (the c of the source row, or free[s], or 0),
//                evaluate the gate in Montgomery Fr, store a, b, c fully reduced
//   K23  run     the same for a run of consecutive levels of at most kWitBlock rows each: ONE workgroup of kWitBlock lanes walks the
//                levels with a barrier between them
//   K24  fill    the rows that compute nothing (wide gate, qO = 0): their a, b and c take the values of their classes
//   K25  check   every row against the gate identity, every slot against the value of its class: counts and smallest indices
// Both gate kinds share the kernels (KIND 0: q1, q2; KIND 1: qL, qR, qM, qO, qC, qH in the order of the selector block).
//
// Lookup plans (zk_witness_plan_create_lookup; the rules are in include/zkhip.h).  The plan owns a KEY TABLE: the slots of zk_find.cuh over
// the pair (t0, t1), built once at plan creation:
//   K26  key build   K20's walk at NC = 2: every entry y < N inserted by its pair; equal pairs meet in one slot, which ends holding the
//                    smallest of their indices
//   K27  key check   in a launch of its own: every entry walks to the slot of its pair and compares its t2 with the t2 of the index
//                    there -- the FIRST entry of that pair.  The count of entries that differ and the smallest of them are properties
//                    of the table alone.  (Comparing inside K26, against whatever index the CAS returns, would count by thread order.)
// The level kernels K22 / K23 have a variant for the wide gate on a lookup plan (k_wit_level_lk, k_wit_run_lk): a row whose order entry
// carries kWitLookup gathers a and b as every row does, walks the slots with plain loads (find_walk: bounded by the slot count, an index
// read from a slot checked < N before anything is read through it) and stores a, b, t2[y] -- or a, b, 0 on a miss, which the check then
// reports.  The basic gate has no such row (every row is gate-computing), so its lookup plans run the plain kernels.  K25 is followed by
// K25L (k_wit_check_lk, both gate kinds): a row with qk = 1 is good iff the probe of (a, b) hits some y and c == t2[y] -- exact with the
// pair table alone, because the table is a function of its pair.  A walk that passes every slot, or a slot word >= N, sets the internal flag.
// The kernels of plans without a lookup are the ones above, unchanged: the lookup variants are kernels of their own, with an argument
// block of their own (WitLk), and share the row functions.
//
// Advice plans (zk_witness_plan_create_advice with a non-zero code; the rules are in include/zkhip.h).  A row whose order entry carries
// kWitAdvice gathers a and b as every row does and takes its c from its code and a: the inverse (0 for 0), or a field of the bits of a's
// canonical integer.  K22 / K23 have a third variant for such plans, with and without a lookup (k_wit_level_adv<LK>, k_wit_run_adv<LK>):
// gate rows, advice rows and, at LK = 1, lookup rows, on the row functions of the other variants.  The plan puts the advice rows of a
// level behind its other rows, so a wave of a large level pays the inversion only when it holds such rows.  The check does not look at
// the codes: an advice row constrains nothing by itself.
//
// Order.  The launches follow one another on the ctx stream; no host read lies between them.  A row reads only the c of rows of LOWER
// levels: an earlier launch, or an earlier level of the same workgroup, whose stores are complete and visible at workgroup scope after
// the fence and the barrier that close the level.  No kernel ever waits on another workgroup: no ready flags, no spin loops, no
// cooperative launch.  A deep narrow circuit is therefore one long single-workgroup launch (a level costs one gather, one gate and one
// barrier), not one launch per level.
//
// Bounds.  Every index a kernel uses comes from the plan (src < N or kWitFree | slot < 3N, order < N, the level offsets <= N), which the
// library built and owns; the caller's arrays (selectors, free, public inputs) are read only AT such indices and never AS indices.
// free and the public inputs are reduced below r when they are read (a value < 2^256 < 3r needs two conditional subtractions).
//
// Registers (hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): DESIGN.md, section 4.
#include "zk_find.cuh"

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstring>

namespace zk {

struct WitArgs {
    const u32* src;
    const u32* order;
    const u32* lvoff;
    const void* inv;     // KIND 1: 1 / qO
    const void* sel[6];
    const void* pi;      // l Fr
    const void* free_;   // 3N Fr, or null: zeros
    void* w[3];          // a, b, c
    u32 N, l;
};
struct WitStatus {  // 64 bytes in arena 4: zeroed, the three `first` words set to 2^32 - 1
    unsigned long long bad_rows, bad_copies;
    u32 first_row, first_copy;
    u32 first_lookup, bad_lookups;  // lookup plans: the rows with qk = 1 whose triple is no table entry (N <= 2^29: a u32 counts them)
    u32 internal;                   // lookup plans: a walk passed every slot, or a slot held a word >= N
    u32 pad[7];                     // nine words are used; the public inputs follow the block and are loaded as 32-byte elements, so it keeps their alignment
};
struct WitLk {  // what the lookup variants read beside WitArgs
    FindCols<2> key;  // w unused; t = t0, t1
    const void* t2;
    const void* qk;   // K25 only
    const u32* slots;
    u64 mask;         // slots - 1
    long long force;  // the plan's start slot (-1: the hash)
    WitStatus* st;
};

__device__ __forceinline__ Fr wit_canon(const Fr& v) { return fp_reduce_once<FrCfg>(fp_reduce_once<FrCfg>(v)); }

// the value of a class: the c of its source row, or the caller's free value of its smallest slot (absent: 0)
__device__ __forceinline__ Fr wit_value(const WitArgs& w, u32 s) {
    if (s & kWitFree) return w.free_ ? wit_canon(fr_load(w.free_, s & ~kWitFree)) : fp_zero<FrCfg>();
    return fr_load(w.w[2], s);
}
__device__ __forceinline__ Fr wit_in(const WitArgs& w, u32 x) { return x < w.l ? wit_canon(fr_load(w.pi, x)) : fp_zero<FrCfg>(); }

// the c that satisfies row x: basic three multiplications; wide ten (a^5 as a^2, a^4, a^4 a; the last one by 1 / qO)
template <int KIND>
__device__ __forceinline__ Fr wit_out(const WitArgs& w, u32 x, const Fr& a, const Fr& b) {
    const Fr in = wit_in(w, x);
    if (KIND == 0) {
        const Fr s = fr_mul(fr_load(w.sel[0], x), fr_add(a, b));
        const Fr p = fr_mul(fr_mul(fr_load(w.sel[1], x), a), b);
        return fr_add(fr_add(s, p), in);
    }
    const Fr a2 = fr_mul(a, a);
    const Fr a5 = fr_mul(fr_mul(a2, a2), a);
    const Fr lin = fr_add(fr_mul(fr_load(w.sel[0], x), a), fr_mul(fr_load(w.sel[1], x), b));
    const Fr hi = fr_add(fr_mul(fr_mul(fr_load(w.sel[2], x), a), b), fr_mul(fr_load(w.sel[5], x), a5));
    const Fr t = fr_add(fr_add(fr_add(lin, hi), fr_load(w.sel[4], x)), in);
    return fr_mul(t, fr_load(w.inv, x));
}
template <int KIND>
__device__ __forceinline__ void wit_row(const WitArgs& w, u32 x) {
    const Fr a = wit_value(w, w.src[x]), b = wit_value(w, w.src[w.N + x]);
    const Fr c = wit_out<KIND>(w, x, a, b);
    fr_store(w.w[0], x, a);
    fr_store(w.w[1], x, b);
    fr_store(w.w[2], x, c);
}

// the probe of a lookup plan: the smallest y with (t0, t1)[y] == (a, b).  1 hit, 2 miss; 0 (cannot happen) sets the internal flag
__device__ __forceinline__ int wit_probe(const WitLk& lk, u32 N, const Fr& a, const Fr& b, u32& y) {
    const Fr k[2] = {a, b};
    const int end = find_walk<2>(k, lk.key, N, lk.slots, lk.mask, lk.force, y);
    if (end == 0) atomicOr(&lk.st->internal, 1u);
    return end;
}
// a row of a lookup plan (wide gate): e = the order entry, the row and the flag of a lookup-computing row
__device__ __forceinline__ void wit_row_lk(const WitArgs& w, const WitLk& lk, u32 e) {
    const u32 x = e & ~kWitLookup;
    const Fr a = wit_value(w, w.src[x]), b = wit_value(w, w.src[w.N + x]);
    Fr c;
    if (e & kWitLookup) {
        u32 y;
        c = wit_probe(lk, w.N, a, b, y) == 1 ? fr_load(lk.t2, y) : fp_zero<FrCfg>();
    } else {
        c = wit_out<1>(w, x, a, b);
    }
    fr_store(w.w[0], x, a);
    fr_store(w.w[1], x, b);
    fr_store(w.w[2], x, c);
}

// the c of an advice row.  a is fully reduced (wit_value).  INV0: 1 / a by Fermat, and an explicit 0 for 0.  BITS: out of Montgomery
// form, fully reduced, then `width` <= 64 bits from bit `shift` -- a window of three 32-bit limbs (64 bits at any offset; the limbs past
// the eighth are 0, and so is every bit from 255 up) -- and back into Montgomery form by one multiplication with R^2.  The limb is picked
// by compares, not by a dynamic index: the limbs stay in registers.  The plan checked the code.
__device__ __forceinline__ Fr wit_advice(u32 code, const Fr& a) {
    if ((code & 0xff) == 1) {
        if (fp_is_zero(a)) return fp_zero<FrCfg>();
        return fp_inv<FrCfg>(a);
    }
    const u32 shift = (code >> 8) & 0xff, width = (code >> 16) & 0xff;
    const Fr v = wit_canon(fp_from_mont<FrCfg>(a));
    const u32 k0 = shift >> 5, off = shift & 31;
    u32 l0 = 0, l1 = 0, l2 = 0;
#pragma unroll
    for (u32 k = 0; k < 8; k++) {
        l0 = k == k0 ? v.l[k] : l0;
        l1 = k == k0 + 1 ? v.l[k] : l1;
        l2 = k == k0 + 2 ? v.l[k] : l2;
    }
    u64 f = (((u64)l1 << 32) | l0) >> off;
    if (off) f |= (u64)l2 << (64 - off);
    if (width < 64) f &= ((u64)1 << width) - 1;
    Fr t = fp_zero<FrCfg>(), r2;
    t.l[0] = (u32)f, t.l[1] = (u32)(f >> 32);
#pragma unroll
    for (int i = 0; i < 8; i++) r2.l[i] = FrCfg::R2(i);
    return fr_mul(t, r2);
}
// a row of an advice plan (wide gate): e = the order entry, the row and the flag of an advice- or (LK) lookup-computing row
template <int LK>
__device__ __forceinline__ void wit_row_adv(const WitArgs& w, const WitLk& lk, const u32* __restrict__ adv, u32 e) {
    const u32 x = e & ~(kWitLookup | kWitAdvice);
    const Fr a = wit_value(w, w.src[x]), b = wit_value(w, w.src[w.N + x]);
    Fr c;
    if (e & kWitAdvice) {
        c = wit_advice(adv[x], a);
    } else if (LK && (e & kWitLookup)) {
        u32 y;
        c = wit_probe(lk, w.N, a, b, y) == 1 ? fr_load(lk.t2, y) : fp_zero<FrCfg>();
    } else {
        c = wit_out<1>(w, x, a, b);
    }
    fr_store(w.w[0], x, a);
    fr_store(w.w[1], x, b);
    fr_store(w.w[2], x, c);
}

// ---------------------------------------------------------------------------------------
// K22.  order[begin .. end): one level
// ---------------------------------------------------------------------------------------
template <int KIND>
__global__ void __launch_bounds__(kWitBlock) k_wit_level(WitArgs w, u32 begin, u32 end) {
    for (size_t i = (size_t)begin + (size_t)blockIdx.x * kWitBlock + threadIdx.x; i < end; i += (size_t)gridDim.x * kWitBlock) wit_row<KIND>(w, w.order[i]);
}
__global__ void __launch_bounds__(kWitBlock) k_wit_level_lk(WitArgs w, WitLk lk, u32 begin, u32 end) {
    for (size_t i = (size_t)begin + (size_t)blockIdx.x * kWitBlock + threadIdx.x; i < end; i += (size_t)gridDim.x * kWitBlock) wit_row_lk(w, lk, w.order[i]);
}
template <int LK>
__global__ void __launch_bounds__(kWitBlock) k_wit_level_adv(WitArgs w, WitLk lk, const u32* __restrict__ adv, u32 begin, u32 end) {
    for (size_t i = (size_t)begin + (size_t)blockIdx.x * kWitBlock + threadIdx.x; i < end; i += (size_t)gridDim.x * kWitBlock) wit_row_adv<LK>(w, lk, adv, w.order[i]);
}

// ---------------------------------------------------------------------------------------
// K23.  ONE workgroup; levels lv0 .. lv1 - 1, each of at most kWitBlock rows
// ---------------------------------------------------------------------------------------
template <int KIND>
__global__ void __launch_bounds__(kWitBlock) k_wit_run(WitArgs w, u32 lv0, u32 lv1) {
    for (u32 lv = lv0; lv < lv1; lv++) {
        const u32 i = w.lvoff[lv] + threadIdx.x;
        if (i < w.lvoff[lv + 1]) wit_row<KIND>(w, w.order[i]);
        __threadfence_block();
        __syncthreads();
    }
}
__global__ void __launch_bounds__(kWitBlock) k_wit_run_lk(WitArgs w, WitLk lk, u32 lv0, u32 lv1) {
    for (u32 lv = lv0; lv < lv1; lv++) {
        const u32 i = w.lvoff[lv] + threadIdx.x;
        if (i < w.lvoff[lv + 1]) wit_row_lk(w, lk, w.order[i]);  // the probe inside the branch, the barrier outside it
        __threadfence_block();
        __syncthreads();
    }
}
template <int LK>
__global__ void __launch_bounds__(kWitBlock) k_wit_run_adv(WitArgs w, WitLk lk, const u32* __restrict__ adv, u32 lv0, u32 lv1) {
    for (u32 lv = lv0; lv < lv1; lv++) {
        const u32 i = w.lvoff[lv] + threadIdx.x;
        if (i < w.lvoff[lv + 1]) wit_row_adv<LK>(w, lk, adv, w.order[i]);  // the advice and the probe inside the branch, the barrier outside it
        __threadfence_block();
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------
// K24.  order[begin .. N): the rows that compute nothing (neither gate-, lookup- nor advice-computing: their order entries carry no flag)
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kWitBlock) k_wit_fill(WitArgs w, u32 begin) {
    for (size_t i = (size_t)begin + (size_t)blockIdx.x * kWitBlock + threadIdx.x; i < w.N; i += (size_t)gridDim.x * kWitBlock) {
        const u32 x = w.order[i];
        Fr v[3];
#pragma unroll
        for (int j = 0; j < 3; j++) v[j] = wit_value(w, w.src[(size_t)j * w.N + x]);
#pragma unroll
        for (int j = 0; j < 3; j++) fr_store(w.w[j], x, v[j]);
    }
}

// ---------------------------------------------------------------------------------------
// K25.  Row x: the gate identity, then its three slots against the slot that holds the value of their class (the c slot of the source
// row, or the class's smallest slot).  w.w is only read, and is expected fully reduced (include/zkhip.h): copies are compared limb for
// limb, so a wire at or above r counts as a bad copy of its reduced twin.
// ---------------------------------------------------------------------------------------
template <int KIND>
__global__ void __launch_bounds__(kWitBlock) k_wit_check(WitArgs w, WitStatus* __restrict__ st) {
    for (size_t i = (size_t)blockIdx.x * kWitBlock + threadIdx.x; i < w.N; i += (size_t)gridDim.x * kWitBlock) {
        const u32 x = (u32)i;
        Fr v[3];
#pragma unroll
        for (int j = 0; j < 3; j++) v[j] = fr_load(w.w[j], x);
        Fr g;
        if (KIND == 0) {
            g = gate_inner(fr_load(w.sel[0], x), fr_load(w.sel[1], x), v[0], v[1], v[2], wit_in(w, x));
        } else {
            Fr t[kGatewTabs];
            t[0] = fp_zero<FrCfg>();
#pragma unroll
            for (int k = 0; k < 6; k++) t[1 + k] = fr_load(w.sel[k], x);
            t[7] = v[0], t[8] = v[1], t[9] = v[2], t[10] = wit_in(w, x);
            g = gatew_inner(t);
        }
        if (!fp_is_zero(wit_canon(g))) {
            atomicAdd(&st->bad_rows, 1ull);
            atomicMin(&st->first_row, x);
        }
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const u32 s = w.src[(size_t)j * w.N + x];
            const u32 rep = (s & kWitFree) ? (s & ~kWitFree) : 2 * w.N + s;  // < 3N
            const u32 col = rep / w.N;
            const Fr r = fr_load(col == 0 ? w.w[0] : col == 1 ? w.w[1] : w.w[2], rep - col * w.N);
            if (!fp_eq(v[j], r)) {
                atomicAdd(&st->bad_copies, 1ull);
                atomicMin(&st->first_copy, (u32)(j * w.N + x));
            }
        }
    }
}

// ---------------------------------------------------------------------------------------
// K25L.  Lookup plans, after K25: a row with qk = 1 (the Montgomery 1; the plan checked that qk holds nothing but 0 and 1) probes (a, b)
// and is a BAD LOOKUP unless the probe hits some y with c == t2[y].  A kernel of its own and not a branch of K25: the walk is a chain of
// dependent random reads, which wants the eight waves per SIMD this kernel gets and K25 (four to six) does not, and K25 stays as it was.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kWitBlock) k_wit_check_lk(WitArgs w, WitLk lk) {
    for (size_t i = (size_t)blockIdx.x * kWitBlock + threadIdx.x; i < w.N; i += (size_t)gridDim.x * kWitBlock) {
        const u32 x = (u32)i;
        if (!fp_eq(fr_load(lk.qk, x), fp_one<FrCfg>())) continue;
        u32 y;
        const int end = wit_probe(lk, w.N, fr_load(w.w[0], x), fr_load(w.w[1], x), y);
        if (end == 0) continue;  // (the internal flag is set)
        if (end == 2 || !fp_eq(fr_load(w.w[2], x), fr_load(lk.t2, y))) {
            atomicAdd(&lk.st->bad_lookups, 1u);
            atomicMin(&lk.st->first_lookup, x);
        }
    }
}

// ---------------------------------------------------------------------------------------
// K26 / K27.  The key table of a lookup plan: c.t = t0, t1; KeyStatus zeroed, `first` set to 2^32 - 1
// ---------------------------------------------------------------------------------------
struct KeyStatus {
    unsigned long long bad;  // entries whose t2 differs from the t2 of the first entry of their pair
    u32 internal, first;
    u32 pad[4];
};
__global__ void __launch_bounds__(kWitBlock) k_wit_key_build(FindCols<2> c, size_t N, u32* __restrict__ slots, u64 mask, long long force, KeyStatus* __restrict__ st) {
    for (size_t y = (size_t)blockIdx.x * kWitBlock + threadIdx.x; y < N; y += (size_t)gridDim.x * kWitBlock) {
        const Fr k[2] = {fr_load(c.t[0], y), fr_load(c.t[1], y)};
        if (!find_insert<2>(k, c, N, y, slots, mask, force)) atomicOr(&st->internal, 1u);
    }
}
__global__ void __launch_bounds__(kWitBlock) k_wit_key_check(FindCols<2> c, const void* __restrict__ t2, size_t N, const u32* __restrict__ slots, u64 mask, long long force,
                                                             KeyStatus* __restrict__ st) {
    for (size_t y = (size_t)blockIdx.x * kWitBlock + threadIdx.x; y < N; y += (size_t)gridDim.x * kWitBlock) {
        const Fr k[2] = {fr_load(c.t[0], y), fr_load(c.t[1], y)};
        u32 v;
        if (find_walk<2>(k, c, N, slots, mask, force, v) != 1) {  // an inserted pair is always found
            atomicOr(&st->internal, 1u);
            continue;
        }
        if (v != (u32)y && !fp_eq(fr_load(t2, y), fr_load(t2, v))) {
            atomicAdd(&st->bad, 1ull);
            atomicMin(&st->first, (u32)y);
        }
    }
}

// ---------------------------------------------------------------------------------------
// host drivers
// ---------------------------------------------------------------------------------------
int witness_key_table(zk_ctx* ctx, const char* name, const void* const* d_t, size_t N, long force, uint32_t* d_slots) {
    const size_t slots = 2 * N;
    KeyStatus* st = (KeyStatus*)scratch(ctx, 4, sizeof(KeyStatus));
    if (!st) return ZK_ERR_OOM;
    KeyStatus* h_st = (KeyStatus*)pinned(ctx, sizeof(KeyStatus));
    if (!h_st) return ZK_ERR_OOM;
    FindCols<2> c;
    for (int j = 0; j < 2; j++) c.w[j] = nullptr, c.t[j] = d_t[j];
    ZK_HIP(ctx, hipMemsetAsync(st, 0, sizeof(KeyStatus), ctx->stream));
    ZK_HIP(ctx, hipMemsetAsync(&st->first, 0xff, sizeof(u32), ctx->stream));
    ZK_HIP(ctx, hipMemsetAsync(d_slots, 0xff, slots * sizeof(u32), ctx->stream));
    const unsigned blocks = (unsigned)std::min<size_t>((N + kWitBlock - 1) / kWitBlock, (size_t)ctx->cu_count * 8);
    hipLaunchKernelGGL(k_wit_key_build, dim3(blocks), dim3(kWitBlock), 0, ctx->stream, c, N, (u32*)d_slots, (u64)(slots - 1), (long long)force, st);
    ZK_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_wit_key_check, dim3(blocks), dim3(kWitBlock), 0, ctx->stream, c, d_t[2], N, (const u32*)d_slots, (u64)(slots - 1), (long long)force, st);
    ZK_HIP(ctx, hipGetLastError());
    ZK_HIP(ctx, hipMemcpyAsync(h_st, st, sizeof(KeyStatus), hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (h_st->internal) return fail(ctx, ZK_ERR_INTERNAL, "%s: a walk passed all %zu slots of the key table", name, slots);
    if (h_st->bad)
        return fail(ctx, ZK_ERR_INVALID, "%s: %llu of %zu table entries repeat the pair (t0, t1) of an earlier entry with another t2; the first is entry %u", name, h_st->bad, N,
                    h_st->first);
    return ZK_OK;
}

// d_qk, d_t: both null on a plain plan, both given on a lookup plan (lk is filled then)
static int wit_args(zk_ctx* ctx, const char* name, const zk_witness_plan* plan, int gate_kind, const void* const* d_sel, const void* d_qk, const void* const* d_t,
                    const uint64_t* h_pi, size_t l, WitArgs& w, WitLk& lk, WitStatus** d_st) {
    if (plan->ctx != ctx) return fail(ctx, ZK_ERR_INVALID, "%s: the plan belongs to another ctx", name);
    if (plan->lookup != (d_qk != nullptr))
        return fail(ctx, ZK_ERR_INVALID, plan->lookup ? "%s: the plan was built with a lookup; call the _lookup form with the selector and the tables it was built from"
                                                      : "%s: the plan was built without a lookup (zk_witness_plan_create)", name);
    if (gate_kind != 0 && gate_kind != 1) return fail(ctx, ZK_ERR_INVALID, "%s: gate_kind %d is neither 0 (basic) nor 1 (wide)", name, gate_kind);
    if ((gate_kind == 1) != (plan->d_inv != nullptr))
        return fail(ctx, ZK_ERR_INVALID, "%s: the wide gate needs a plan built with its output selector, the basic gate one built without", name);
    const size_t N = plan->N;
    if (l > N) return fail(ctx, ZK_ERR_INVALID, "%s: %zu public inputs on %zu rows", name, l, N);
    for (int k = 0; k < (gate_kind ? 6 : 2); k++)
        if (!d_sel[k]) return fail(ctx, ZK_ERR_INVALID, "null argument");
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    // arena 4: the status, then the public inputs (staged through pinned memory: the status read-back, then the inputs)
    char* s = (char*)scratch(ctx, 4, sizeof(WitStatus) + 32 * l);
    if (!s) return ZK_ERR_OOM;
    char* h = (char*)pinned(ctx, sizeof(WitStatus) + 32 * l);
    if (!h) return ZK_ERR_OOM;
    memset(&w, 0, sizeof(w));
    w.src = plan->d_src, w.order = plan->d_order, w.lvoff = plan->d_lvoff, w.inv = plan->d_inv;
    for (int k = 0; k < (gate_kind ? 6 : 2); k++) w.sel[k] = d_sel[k];
    w.pi = s + sizeof(WitStatus), w.N = (u32)N, w.l = (u32)l;
    if (l) {
        memcpy(h + sizeof(WitStatus), h_pi, 32 * l);
        ZK_HIP(ctx, hipMemcpyAsync(s + sizeof(WitStatus), h + sizeof(WitStatus), 32 * l, hipMemcpyHostToDevice, ctx->stream));
    }
    *d_st = (WitStatus*)s;
    memset(&lk, 0, sizeof(lk));
    if (plan->lookup) {
        lk.key.t[0] = d_t[0], lk.key.t[1] = d_t[1], lk.t2 = d_t[2], lk.qk = d_qk;
        lk.slots = plan->d_slots, lk.mask = 2 * (u64)N - 1, lk.force = plan->force, lk.st = *d_st;
    }
    // the status: zeroed, the three `first` words 2^32 - 1 (before the level launches: those of a lookup plan may set the internal flag)
    static_assert(sizeof(WitStatus) == 64 && offsetof(WitStatus, first_lookup) == offsetof(WitStatus, first_row) + 8, "WitStatus layout");
    ZK_HIP(ctx, hipMemsetAsync(*d_st, 0, sizeof(WitStatus), ctx->stream));
    ZK_HIP(ctx, hipMemsetAsync(&(*d_st)->first_row, 0xff, 3 * sizeof(u32), ctx->stream));
    return ZK_OK;
}

// the check on the ctx stream and its ONE read-back (lk.st set: a lookup plan)
static int wit_check(zk_ctx* ctx, const char* name, int gate_kind, const WitArgs& w, const WitLk& lk, WitStatus* st, WitStatus* h_out) {
    const unsigned blocks = (unsigned)std::min<size_t>(((size_t)w.N + kWitBlock - 1) / kWitBlock, (size_t)ctx->cu_count * 8);
    if (gate_kind) hipLaunchKernelGGL(k_wit_check<1>, dim3(blocks), dim3(kWitBlock), 0, ctx->stream, w, st);
    else hipLaunchKernelGGL(k_wit_check<0>, dim3(blocks), dim3(kWitBlock), 0, ctx->stream, w, st);
    ZK_HIP(ctx, hipGetLastError());
    if (lk.st) {
        hipLaunchKernelGGL(k_wit_check_lk, dim3(blocks), dim3(kWitBlock), 0, ctx->stream, w, lk);
        ZK_HIP(ctx, hipGetLastError());
    }
    WitStatus* h = (WitStatus*)pinned(ctx, sizeof(WitStatus));  // (the head of the block wit_args sized)
    ZK_HIP(ctx, hipMemcpyAsync(h, st, sizeof(WitStatus), hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *h_out = *h;
    if (h_out->internal) return fail(ctx, ZK_ERR_INTERNAL, "%s: a probe walk passed all %llu slots of the key table", name, (unsigned long long)lk.mask + 1);
    return ZK_OK;
}

int plonk_witness_check(zk_ctx* ctx, const zk_witness_plan* plan, int gate_kind, const void* const* d_sel, const void* d_qk, const void* const* d_t, const uint64_t* h_pi,
                        size_t l, const void* d_a, const void* d_b, const void* d_c, uint64_t* h_bad) {
    const char* name = d_qk ? "zk_plonk_witness_check_lookup" : "zk_plonk_witness_check";
    WitArgs w;
    WitLk lk;
    WitStatus *st, r;
    int rc = wit_args(ctx, name, plan, gate_kind, d_sel, d_qk, d_t, h_pi, l, w, lk, &st);
    if (rc != ZK_OK) return rc;
    w.w[0] = const_cast<void*>(d_a), w.w[1] = const_cast<void*>(d_b), w.w[2] = const_cast<void*>(d_c);  // K25 only reads them
    rc = wit_check(ctx, name, gate_kind, w, lk, st, &r);
    if (rc != ZK_OK) return rc;
    h_bad[0] = r.bad_rows, h_bad[1] = r.bad_rows ? r.first_row : ~0ull, h_bad[2] = r.bad_copies, h_bad[3] = r.bad_copies ? r.first_copy : ~0ull;
    if (plan->lookup) h_bad[4] = r.bad_lookups, h_bad[5] = r.bad_lookups ? r.first_lookup : ~0ull;
    return ZK_OK;
}

int plonk_witness(zk_ctx* ctx, const zk_witness_plan* plan, int gate_kind, const void* const* d_sel, const void* d_qk, const void* const* d_t, const uint64_t* h_pi, size_t l,
                  const void* d_free, void* d_a, void* d_b, void* d_c) {
    const char* name = d_qk ? "zk_plonk_witness_lookup" : "zk_plonk_witness";
    if (d_a == d_b || d_a == d_c || d_b == d_c) return fail(ctx, ZK_ERR_INVALID, "%s: a, b and c must be three buffers", name);
    WitArgs w;
    WitLk lk;
    WitStatus *st, r;
    int rc = wit_args(ctx, name, plan, gate_kind, d_sel, d_qk, d_t, h_pi, l, w, lk, &st);
    if (rc != ZK_OK) return rc;
    w.free_ = d_free, w.w[0] = d_a, w.w[1] = d_b, w.w[2] = d_c;
    const size_t N = plan->N;
    const bool lk_rows = plan->lookup && gate_kind;  // the basic gate has no lookup-computing row: its order entries carry no flag
    const u32* adv = plan->d_advice;                 // an advice plan is one of the wide gate (wit_args checked the kind against d_inv)
    for (const zk_witness_plan::Launch& L : plan->launches) {
        if (L.grid) {
            const u32 begin = plan->lvoff[L.lv0], end = plan->lvoff[L.lv1];
            const unsigned blocks = (unsigned)std::min<size_t>(((size_t)(end - begin) + kWitBlock - 1) / kWitBlock, (size_t)ctx->cu_count * 8);
            if (adv && plan->lookup) hipLaunchKernelGGL(k_wit_level_adv<1>, dim3(blocks), dim3(kWitBlock), 0, ctx->stream, w, lk, adv, begin, end);
            else if (adv) hipLaunchKernelGGL(k_wit_level_adv<0>, dim3(blocks), dim3(kWitBlock), 0, ctx->stream, w, lk, adv, begin, end);
            else if (lk_rows) hipLaunchKernelGGL(k_wit_level_lk, dim3(blocks), dim3(kWitBlock), 0, ctx->stream, w, lk, begin, end);
            else if (gate_kind) hipLaunchKernelGGL(k_wit_level<1>, dim3(blocks), dim3(kWitBlock), 0, ctx->stream, w, begin, end);
            else hipLaunchKernelGGL(k_wit_level<0>, dim3(blocks), dim3(kWitBlock), 0, ctx->stream, w, begin, end);
        } else {
            if (adv && plan->lookup) hipLaunchKernelGGL(k_wit_run_adv<1>, dim3(1), dim3(kWitBlock), 0, ctx->stream, w, lk, adv, L.lv0, L.lv1);
            else if (adv) hipLaunchKernelGGL(k_wit_run_adv<0>, dim3(1), dim3(kWitBlock), 0, ctx->stream, w, lk, adv, L.lv0, L.lv1);
            else if (lk_rows) hipLaunchKernelGGL(k_wit_run_lk, dim3(1), dim3(kWitBlock), 0, ctx->stream, w, lk, L.lv0, L.lv1);
            else if (gate_kind) hipLaunchKernelGGL(k_wit_run<1>, dim3(1), dim3(kWitBlock), 0, ctx->stream, w, L.lv0, L.lv1);
            else hipLaunchKernelGGL(k_wit_run<0>, dim3(1), dim3(kWitBlock), 0, ctx->stream, w, L.lv0, L.lv1);
        }
        ZK_HIP(ctx, hipGetLastError());
    }
    if (plan->computing < N) {
        const unsigned blocks = (unsigned)std::min<size_t>((N - plan->computing + kWitBlock - 1) / kWitBlock, (size_t)ctx->cu_count * 8);
        hipLaunchKernelGGL(k_wit_fill, dim3(blocks), dim3(kWitBlock), 0, ctx->stream, w, (u32)plan->computing);
        ZK_HIP(ctx, hipGetLastError());
    }
    rc = wit_check(ctx, name, gate_kind, w, lk, st, &r);
    if (rc != ZK_OK) return rc;
    // the refusals, combined when several fail
    char msg[512];
    int at = 0;
    const char* sep = "";
    if (r.bad_rows) at += snprintf(msg + at, sizeof(msg) - at, "%llu of %zu rows do not satisfy the gate; the first is row %u", r.bad_rows, N, r.first_row), sep = "; ";
    if (r.bad_copies)
        at += snprintf(msg + at, sizeof(msg) - at, "%s%llu of %zu slots differ from the value of their class; the first is slot %u", sep, r.bad_copies, 3 * N, r.first_copy), sep = "; ";
    if (r.bad_lookups) at += snprintf(msg + at, sizeof(msg) - at, "%s%u of %zu rows with qk = 1 hold a triple that is no table entry; the first is row %u", sep, r.bad_lookups, N, r.first_lookup);
    if (at) return fail(ctx, ZK_ERR_INVALID, "%s: %s", name, msg);
    return ZK_OK;
}

}  // namespace zk
