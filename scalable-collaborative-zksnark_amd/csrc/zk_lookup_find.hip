// zk_lookup_find.hip -- lookups without caller indices: the device finds, for every row, the table entry that holds its value.
//   K20  build   every table entry y < N inserted into an open-addressing hash table of u32 slots (linear probing)
//   K21  probe   every row walks the same sequence to the slot of its entry: idx[x] = the slot's index, one more on that entry's u32 counter
// followed by k_lookup_write (zk_lookup.hip), which writes the counters as Montgomery Fr, and ONE status read-back.  Both forms share the
// kernels: NC = 1 column (f against t, four 64-bit limbs) or NC = 3 columns with a selector ((a, b, c) against (t0, t1, t2), twelve limbs).
//
// Conventions of zk_lookup.hip / zk_lookup3.hip: Fr in Montgomery form, 32-byte AoS elements, inputs never written, work on the ctx stream,
// scratch from the ctx arenas.
//
// The slot protocol (its device functions are zk_find.cuh, shared with the key table of zk_witness.hip).  slots = a power of two >= 2N
// (load <= 0.5), filled with kFindEmpty = 2^32 - 1 (N <= 2^31 keeps every index below it).
// Entry y starts at slot mix(limbs of entry y) mod slots and walks upwards, wrapping round the end:
//     prev = atomicCAS(slot, EMPTY, y):   EMPTY           the slot is claimed for the key of entry y; done
//                                         an index v      entry v == entry y in all limbs ?  atomicMin(slot, y), done  :  next slot
// A slot that has been claimed keeps its KEY for good: every index it ever holds names an entry equal to the first one, and only the
// index can fall.  All entries of one key walk one sequence of slots, the slots they pass are held by other keys for good, and exactly one
// CAS wins the first free one: so equal entries meet in ONE slot, and that slot ends holding the smallest of their indices whatever the order
// of the threads.  The table entries themselves are inputs, written before the launch: comparing through an index read from a slot needs no
// hand-off between workgroups, and the slot words are only ever touched by atomics in K20 (the value CAS returns comes from L2).
// K21 runs in a launch of its own, after K20: plain loads of the slots.  A row stops at the slot whose entry equals it (hit) or at EMPTY
// (miss: no entry of its key was inserted, because every inserted key sits before the first EMPTY of its own sequence).
// The RESULT -- the smallest index of an equal entry -- is a property of the table alone: the hash function, the knob find_force_slot and
// the order of the threads change the walks, never idx or m.
//
// Every walk is bounded by the slot count.  At load <= 0.5 a walk that passes every slot cannot happen; one that does sets the internal
// flag (ZK_ERR_INTERNAL).  An index read from a slot is checked to be < N before anything is read through it (the slots hold nothing else,
// so this cannot fire either: internal flag).
//
// Registers and occupancy (hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): the key of a thread is 8 (NC = 1) or 24
// (NC = 3) VGPRs, the candidate entry is loaded and compared one column at a time; K20 takes 30 / 48 VGPRs, K21 26 / 44, no scratch, no
// LDS: eight waves per SIMD for all four, which is what a walk of dependent random reads wants.  Grid: 8 workgroups of 256 per CU.
#include "zk_find.cuh"

#include <algorithm>
#include <cstring>

namespace zk {

// status of a call, 32 bytes in arena 4 before the counters: zeroed, `first` set to 2^32 - 1
struct FindStatus {
    unsigned long long bad;  // rows that are not in the table, or whose qk is neither 0 nor 1
    u32 internal;            // a walk passed every slot, or a slot held an index >= N
    u32 pad0;
    u32 first;               // the smallest bad row
    u32 pad1[3];
};

// ---------------------------------------------------------------------------------------
// K20.  mask = slots - 1; force >= 0: every key starts at slot force & mask (knob find_force_slot).
// ---------------------------------------------------------------------------------------
template <int NC>
__global__ void __launch_bounds__(kGateBlock) k_find_build(FindCols<NC> c, size_t N, u32* __restrict__ slots, u64 mask, long long force, FindStatus* __restrict__ st) {
    for (size_t y = (size_t)blockIdx.x * kGateBlock + threadIdx.x; y < N; y += (size_t)gridDim.x * kGateBlock) {
        Fr k[NC];
#pragma unroll
        for (int j = 0; j < NC; j++) k[j] = fr_load(c.t[j], y);
        if (!find_insert<NC>(k, c, N, y, slots, mask, force)) atomicOr(&st->internal, 1u);
    }
}

// ---------------------------------------------------------------------------------------
// K21.  SEL: rows gated by qk as in K17 (0: idx = 0 and nothing else read; the Montgomery 1: looked up; anything else: a bad row).
// idx, cnt: either may be null.
// ---------------------------------------------------------------------------------------
template <int NC, bool SEL>
__global__ void __launch_bounds__(kGateBlock) k_find_probe(FindCols<NC> c, const void* __restrict__ qk, size_t N, const u32* __restrict__ slots, u64 mask, long long force,
                                                          u32* __restrict__ idx, u32* __restrict__ cnt, FindStatus* __restrict__ st) {
    for (size_t x = (size_t)blockIdx.x * kGateBlock + threadIdx.x; x < N; x += (size_t)gridDim.x * kGateBlock) {
        if (SEL) {
            const Fr q = fr_load(qk, x);
            if (fp_eq(q, fp_zero<FrCfg>())) {
                if (idx) idx[x] = 0;
                continue;
            }
            if (!fp_eq(q, fp_one<FrCfg>())) {  // neither 0 nor 1: a bad row, and nothing of it is read
                atomicAdd(&st->bad, 1ull);
                atomicMin(&st->first, (u32)x);
                continue;
            }
        }
        Fr k[NC];
#pragma unroll
        for (int j = 0; j < NC; j++) k[j] = fr_load(c.w[j], x);
        u32 v;
        const int end = find_walk<NC>(k, c, N, slots, mask, force, v);  // 1 hit, 2 miss
        if (end == 1) {
            if (idx) idx[x] = v;
            if (cnt) atomicAdd(&cnt[v], 1u);
        } else if (end == 2) {
            atomicAdd(&st->bad, 1ull);
            atomicMin(&st->first, (u32)x);
        } else {
            atomicOr(&st->internal, 1u);
        }
    }
}

// ---------------------------------------------------------------------------------------
// host driver of both forms
// ---------------------------------------------------------------------------------------
template <int NC, bool SEL>
static int find_run(zk_ctx* ctx, const char* name, const FindCols<NC>& c, const void* d_qk, size_t N, uint32_t* d_idx, void* d_m, const char* what) {
    if (N < 2 || (N & (N - 1)) || N > ((size_t)1 << 31)) return fail(ctx, ZK_ERR_INVALID, "%s: N = %zu is not a power of two in [2, 2^31]", name, N);
    long force = tuning().find_force_slot;
    if (force < -1) return fail(ctx, ZK_ERR_INVALID, "find_force_slot must be -1 or a slot number");
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t slots = 2 * N;
    // arena 4 (the partials of the sumchecks): the status, then the N counters; arena 0 (the tables of the sumchecks): the slots
    const size_t head = sizeof(FindStatus), cnt_bytes = d_m ? N * sizeof(u32) : 0;
    char* s = (char*)scratch(ctx, 4, head + cnt_bytes);
    if (!s) return ZK_ERR_OOM;
    u32* d_slots = (u32*)scratch(ctx, 0, slots * sizeof(u32));
    if (!d_slots) return ZK_ERR_OOM;
    FindStatus* h_st = (FindStatus*)pinned(ctx, sizeof(FindStatus));
    if (!h_st) return ZK_ERR_OOM;
    FindStatus* st = (FindStatus*)s;
    u32* cnt = d_m ? (u32*)(s + head) : nullptr;
    ZK_HIP(ctx, hipMemsetAsync(s, 0, head + cnt_bytes, ctx->stream));
    ZK_HIP(ctx, hipMemsetAsync(&st->first, 0xff, sizeof(u32), ctx->stream));
    ZK_HIP(ctx, hipMemsetAsync(d_slots, 0xff, slots * sizeof(u32), ctx->stream));
    const unsigned blocks = (unsigned)std::min<size_t>((N + kGateBlock - 1) / kGateBlock, (size_t)ctx->cu_count * 8);
    hipLaunchKernelGGL(k_find_build<NC>, dim3(blocks), dim3(kGateBlock), 0, ctx->stream, c, N, d_slots, (u64)(slots - 1), (long long)force, st);
    ZK_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL((k_find_probe<NC, SEL>), dim3(blocks), dim3(kGateBlock), 0, ctx->stream, c, d_qk, N, (const u32*)d_slots, (u64)(slots - 1), (long long)force,
                       (u32*)d_idx, cnt, st);
    ZK_HIP(ctx, hipGetLastError());
    if (d_m) {
        const int rc = lookup_write_counts(ctx, cnt, N, d_m);
        if (rc != ZK_OK) return rc;
    }
    ZK_HIP(ctx, hipMemcpyAsync(h_st, st, sizeof(FindStatus), hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (h_st->internal) return fail(ctx, ZK_ERR_INTERNAL, "%s: a probe walk passed all %zu slots of the hash table", name, slots);
    if (h_st->bad) return fail(ctx, ZK_ERR_INVALID, "%s: %llu of %zu rows are not in the table (%s); the first is row %u", name, h_st->bad, N, what, h_st->first);
    return ZK_OK;
}

int lookup_find(zk_ctx* ctx, const void* d_f, const void* d_t, size_t N, uint32_t* d_idx, void* d_m) {
    FindCols<1> c;
    c.w[0] = d_f, c.t[0] = d_t;
    return find_run<1, false>(ctx, "zk_lookup_find", c, nullptr, N, d_idx, d_m, "f[x] is no entry of t");
}

int lookup3_find(zk_ctx* ctx, const void* const* d_w, const void* const* d_t, const void* d_qk, size_t N, uint32_t* d_idx, void* d_m) {
    FindCols<3> c;
    for (int j = 0; j < 3; j++) c.w[j] = d_w[j], c.t[j] = d_t[j];
    return find_run<3, true>(ctx, "zk_lookup3_find", c, d_qk, N, d_idx, d_m, "qk neither 0 nor 1, or (a, b, c)[x] no entry of (t0, t1, t2)");
}

}  // namespace zk
