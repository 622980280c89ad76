// zk_witness.hip -- Plonk witness generation and the witness check on the device, per proof, on the plan of zk_witness.cpp.
//   K22  level   one lane per row of ONE level of more than kWitBlock rows: gather a and b (the c of the source row, or free[s], or 0),
//                evaluate the gate in Montgomery Fr, store a, b, c fully reduced
//   K23  run     the same for a run of consecutive levels of at most kWitBlock rows each: ONE workgroup of kWitBlock lanes walks the
//                levels with a barrier between them
//   K24  fill    the rows that compute nothing (wide gate, qO = 0): their a, b and c take the values of their classes
//   K25  check   every row against the gate identity, every slot against the value of its class: counts and smallest indices
// Both gate kinds share the kernels (KIND 0: q1, q2; KIND 1: qL, qR, qM, qO, qC, qH in the order of the selector block).
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
#include "zk_gate.cuh"

#include <algorithm>
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
struct WitStatus {  // 32 bytes in arena 4: zeroed, the two `first` words set to 2^32 - 1
    unsigned long long bad_rows, bad_copies;
    u32 first_row, first_copy;
    u32 pad[2];
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

// ---------------------------------------------------------------------------------------
// K22.  order[begin .. end): one level
// ---------------------------------------------------------------------------------------
template <int KIND>
__global__ void __launch_bounds__(kWitBlock) k_wit_level(WitArgs w, u32 begin, u32 end) {
    for (size_t i = (size_t)begin + (size_t)blockIdx.x * kWitBlock + threadIdx.x; i < end; i += (size_t)gridDim.x * kWitBlock) wit_row<KIND>(w, w.order[i]);
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

// ---------------------------------------------------------------------------------------
// K24.  order[begin .. N): the rows that compute nothing
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
// host drivers
// ---------------------------------------------------------------------------------------
static int wit_args(zk_ctx* ctx, const char* name, const zk_witness_plan* plan, int gate_kind, const void* const* d_sel, const uint64_t* h_pi, size_t l, WitArgs& w,
                    WitStatus** d_st) {
    if (plan->ctx != ctx) return fail(ctx, ZK_ERR_INVALID, "%s: the plan belongs to another ctx", name);
    if (gate_kind != 0 && gate_kind != 1) return fail(ctx, ZK_ERR_INVALID, "%s: gate_kind %d is neither 0 (basic) nor 1 (wide)", name, gate_kind);
    if ((gate_kind == 1) != (plan->d_inv != nullptr))
        return fail(ctx, ZK_ERR_INVALID, "%s: the wide gate needs a plan built with its output selector, the basic gate one built without", name);
    const size_t N = plan->N;
    if (l > N) return fail(ctx, ZK_ERR_INVALID, "%s: %zu public inputs on %zu rows", name, l, N);
    for (int k = 0; k < (gate_kind ? 6 : 2); k++)
        if (!d_sel[k]) return fail(ctx, ZK_ERR_INVALID, "null argument");
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    // arena 4: the status, then the public inputs (staged through pinned memory: 64 bytes for the status read-back, then the inputs)
    char* s = (char*)scratch(ctx, 4, sizeof(WitStatus) + 32 * l);
    if (!s) return ZK_ERR_OOM;
    char* h = (char*)pinned(ctx, 64 + 32 * l);
    if (!h) return ZK_ERR_OOM;
    memset(&w, 0, sizeof(w));
    w.src = plan->d_src, w.order = plan->d_order, w.lvoff = plan->d_lvoff, w.inv = plan->d_inv;
    for (int k = 0; k < (gate_kind ? 6 : 2); k++) w.sel[k] = d_sel[k];
    w.pi = s + sizeof(WitStatus), w.N = (u32)N, w.l = (u32)l;
    if (l) {
        memcpy(h + 64, h_pi, 32 * l);
        ZK_HIP(ctx, hipMemcpyAsync(s + sizeof(WitStatus), h + 64, 32 * l, hipMemcpyHostToDevice, ctx->stream));
    }
    *d_st = (WitStatus*)s;
    return ZK_OK;
}

// the check on the ctx stream and its ONE read-back
static int wit_check(zk_ctx* ctx, int gate_kind, const WitArgs& w, WitStatus* st, WitStatus* h_out) {
    ZK_HIP(ctx, hipMemsetAsync(st, 0, sizeof(WitStatus), ctx->stream));
    ZK_HIP(ctx, hipMemsetAsync(&st->first_row, 0xff, 2 * sizeof(u32), ctx->stream));
    const unsigned blocks = (unsigned)std::min<size_t>(((size_t)w.N + kWitBlock - 1) / kWitBlock, (size_t)ctx->cu_count * 8);
    if (gate_kind) hipLaunchKernelGGL(k_wit_check<1>, dim3(blocks), dim3(kWitBlock), 0, ctx->stream, w, st);
    else hipLaunchKernelGGL(k_wit_check<0>, dim3(blocks), dim3(kWitBlock), 0, ctx->stream, w, st);
    ZK_HIP(ctx, hipGetLastError());
    WitStatus* h = (WitStatus*)pinned(ctx, 64);  // (the block wit_args sized)
    ZK_HIP(ctx, hipMemcpyAsync(h, st, sizeof(WitStatus), hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *h_out = *h;
    return ZK_OK;
}

int plonk_witness_check(zk_ctx* ctx, const zk_witness_plan* plan, int gate_kind, const void* const* d_sel, const uint64_t* h_pi, size_t l, const void* d_a, const void* d_b,
                        const void* d_c, uint64_t* h_bad) {
    WitArgs w;
    WitStatus *st, r;
    int rc = wit_args(ctx, "zk_plonk_witness_check", plan, gate_kind, d_sel, h_pi, l, w, &st);
    if (rc != ZK_OK) return rc;
    w.w[0] = const_cast<void*>(d_a), w.w[1] = const_cast<void*>(d_b), w.w[2] = const_cast<void*>(d_c);  // K25 only reads them
    rc = wit_check(ctx, gate_kind, w, st, &r);
    if (rc != ZK_OK) return rc;
    h_bad[0] = r.bad_rows, h_bad[1] = r.bad_rows ? r.first_row : ~0ull, h_bad[2] = r.bad_copies, h_bad[3] = r.bad_copies ? r.first_copy : ~0ull;
    return ZK_OK;
}

int plonk_witness(zk_ctx* ctx, const zk_witness_plan* plan, int gate_kind, const void* const* d_sel, const uint64_t* h_pi, size_t l, const void* d_free, void* d_a, void* d_b,
                  void* d_c) {
    static const char* name = "zk_plonk_witness";
    if (d_a == d_b || d_a == d_c || d_b == d_c) return fail(ctx, ZK_ERR_INVALID, "%s: a, b and c must be three buffers", name);
    WitArgs w;
    WitStatus *st, r;
    int rc = wit_args(ctx, name, plan, gate_kind, d_sel, h_pi, l, w, &st);
    if (rc != ZK_OK) return rc;
    w.free_ = d_free, w.w[0] = d_a, w.w[1] = d_b, w.w[2] = d_c;
    const size_t N = plan->N;
    for (const zk_witness_plan::Launch& L : plan->launches) {
        if (L.grid) {
            const u32 begin = plan->lvoff[L.lv0], end = plan->lvoff[L.lv1];
            const unsigned blocks = (unsigned)std::min<size_t>(((size_t)(end - begin) + kWitBlock - 1) / kWitBlock, (size_t)ctx->cu_count * 8);
            if (gate_kind) hipLaunchKernelGGL(k_wit_level<1>, dim3(blocks), dim3(kWitBlock), 0, ctx->stream, w, begin, end);
            else hipLaunchKernelGGL(k_wit_level<0>, dim3(blocks), dim3(kWitBlock), 0, ctx->stream, w, begin, end);
        } else {
            if (gate_kind) hipLaunchKernelGGL(k_wit_run<1>, dim3(1), dim3(kWitBlock), 0, ctx->stream, w, L.lv0, L.lv1);
            else hipLaunchKernelGGL(k_wit_run<0>, dim3(1), dim3(kWitBlock), 0, ctx->stream, w, L.lv0, L.lv1);
        }
        ZK_HIP(ctx, hipGetLastError());
    }
    if (plan->computing < N) {
        const unsigned blocks = (unsigned)std::min<size_t>((N - plan->computing + kWitBlock - 1) / kWitBlock, (size_t)ctx->cu_count * 8);
        hipLaunchKernelGGL(k_wit_fill, dim3(blocks), dim3(kWitBlock), 0, ctx->stream, w, (u32)plan->computing);
        ZK_HIP(ctx, hipGetLastError());
    }
    rc = wit_check(ctx, gate_kind, w, st, &r);
    if (rc != ZK_OK) return rc;
    if (r.bad_rows && r.bad_copies)
        return fail(ctx, ZK_ERR_INVALID, "%s: %llu of %zu rows do not satisfy the gate; the first is row %u; %llu of %zu slots differ from the value of their class; the first is slot %u",
                    name, r.bad_rows, N, r.first_row, r.bad_copies, 3 * N, r.first_copy);
    if (r.bad_rows) return fail(ctx, ZK_ERR_INVALID, "%s: %llu of %zu rows do not satisfy the gate; the first is row %u", name, r.bad_rows, N, r.first_row);
    if (r.bad_copies)
        return fail(ctx, ZK_ERR_INVALID, "%s: %llu of %zu slots differ from the value of their class; the first is slot %u", name, r.bad_copies, 3 * N, r.first_copy);
    return ZK_OK;
}

}  // namespace zk
