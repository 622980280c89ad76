// zk_fused.cuh -- the preset-challenge engine of the fused identity sumchecks: ONE pass kernel, reduce kernel, local-stage kernel and
// host driver for every Kind of zk_gate.cuh.  Each identity's file (zk_gate.hip, zk_wiring.hip, zk_perm3.hip, zk_gatew.hip,
// zk_lookup.hip, zk_lookup3.hip) includes this header and instantiates the engine for its own Kind only, so every kernel lives in
// exactly one translation unit.  The transcript-driven engine is zk_fs.hip.
//
// Conventions of zk_fr.hip: Fr in Montgomery form, 32-byte AoS elements, round i binds the TOP index bit (lo = tab[..m/2],
// hi = tab[m/2..]), inputs are never written, all sums are exact modular sums (any association order gives the same bits).
//
// Shape: one HBM pass per round while the tables are longer than the hand-over length (k_sc_pass: a lane owns output index j, reads
// the lo / hi halves of the kTabs tables, writes the folded elements to ping-pong scratch and adds its kEvals products eq(t) * [..](t)
// as 512-bit integers into kEvals 544-bit sums), one Montgomery reduction per sum and call in one launch (k_sc_reduce), then every
// remaining round in one workgroup on tables held in LDS (k_sc_local).  One stream synchronisation per call.
#pragma once
#include "zk_gate.cuh"

#include <algorithm>
#include <cstring>

namespace zk {

// ---------------------------------------------------------------------------------------
// One round over tables of length 2 * half living in HBM.  partials: [t * nbw + 4 block + wave], 80-byte slots.
// Per index pair kTabs multiplications for the folds and kEvals x (those of the bracket + 1).  A product of two elements < r is
// < r^2 < 2^510, so a 544-bit sum holds 2^34 of them; k_sc_reduce adds ALL len/2 products of a pass into one such value, hence
// len <= 2^35 (kGateMaxLog: run_preset refuses longer tables -- they are beyond any HBM anyway).
// K::kViews: element i of table k is read at i << in.sh[k], in every pass (the folded tables have sh = 0), so the first pass reads
// the four views of the product tree in place and nobody makes deinterleaved copies.
// K::kLoadsFirst: all 2 kTabs loads of an index pair stand before its first subtraction; otherwise a table is loaded, subtracted and
// folded before the next is touched.  Each Kind keeps the order its pass was written and measured with.
// ---------------------------------------------------------------------------------------
template <class K>
__global__ void __launch_bounds__(kGateBlock) __attribute__((amdgpu_waves_per_eu(1, K::kWaves)))
k_sc_pass(FsIn<K::kTabs> in, FsOut<K::kTabs> out, size_t half, GateChal ch, GateChal gamma, void* __restrict__ partials) {
    u32 w[K::kEvals][17];
#pragma unroll
    for (int t = 0; t < K::kEvals; t++)
#pragma unroll
        for (int i = 0; i < 17; i++) w[t][i] = 0;
    Fr g0 = fp_zero<FrCfg>(), gd = fp_zero<FrCfg>();  // kFree: the lane's sums of free(lo) and free(hi - lo)
    for (size_t j = (size_t)blockIdx.x * kGateBlock + threadIdx.x; j < half; j += (size_t)gridDim.x * kGateBlock) {
        Fr v[K::kTabs], d[K::kTabs];
#pragma unroll
        for (int k = 0; k < K::kTabs; k++) {
            size_t lo = j, hi = j + half;
            if constexpr (K::kViews) lo <<= in.sh[k], hi <<= in.sh[k];
            v[k] = fr_load(in.t[k], lo), d[k] = fr_load(in.t[k], hi);
            if constexpr (!K::kLoadsFirst) {
                d[k] = fr_sub(d[k], v[k]);
                fr_store(out.t[k], j, fr_add(v[k], fr_mul(ch.r, d[k])));  // lo + r (hi - lo)   dsumcheck.rs:14-19
            }
        }
        if constexpr (K::kLoadsFirst) {
#pragma unroll
            for (int k = 0; k < K::kTabs; k++) {
                d[k] = fr_sub(d[k], v[k]);
                fr_store(out.t[k], j, fr_add(v[k], fr_mul(ch.r, d[k])));
            }
        }
        if constexpr (K::kFree) g0 = fr_add(g0, K::free(v)), gd = fr_add(gd, K::free(d));
        kind_sums_wide<K>(w, gamma.r, v, d);
    }
    if constexpr (K::kFree) kind_free_wide<K>(w, g0, gd);
    gate_wave_store_wide(w, partials);
}

// The sums of all passes of a call in one launch: block (t, p) adds the per-wave partials of evaluation t of pass p and reduces them
// (gate_reduce_block, zk_gate.cuh).
template <class K>
__global__ void __launch_bounds__(kGateBlock) k_sc_reduce(const void* __restrict__ partials, GateReducePlan plan, void* __restrict__ evals) {
    __shared__ uint4 lds[(kGateBlock / 64) * (kGateWideBytes / 16)];
    const unsigned t = blockIdx.x, p = blockIdx.y, nbw = plan.nbw[p];
    gate_reduce_block(partials, (size_t)plan.off[p] + (size_t)t * nbw, nbw, lds, evals, (size_t)p * K::kEvals + t);
}

// ---------------------------------------------------------------------------------------
// Local stage: all remaining rounds of tables of E <= K::kLocalMax elements in one workgroup.  The tables sit in LDS and are folded
// in place (a lane reads elements j and j + h of each and writes j: no other lane touches either before the round's barrier).  Sums
// of a round: wave shuffle, one LDS slot per wave (two sets, by round parity), kEvals lanes finish them.
// K::kViews: the load honours in.sh, so a call whose tables are at most the hand-over length reads the tree's views here.
// ---------------------------------------------------------------------------------------
template <class K>
__global__ void __launch_bounds__(kGateBlock) k_sc_local(FsIn<K::kTabs> in, unsigned E, int rounds, GateTail chal, GateChal gamma, void* __restrict__ evals,
                                                        void* __restrict__ last) {
    extern __shared__ uint4 sclds[];
    uint4* red = sclds + 2 * (size_t)K::kTabs * E;  // [parity][wave][t] Fr
    const unsigned tid = threadIdx.x;
    for (unsigned i = tid; i < E; i += kGateBlock)
#pragma unroll
        for (int k = 0; k < K::kTabs; k++) {
            size_t at = i;
            if constexpr (K::kViews) at <<= in.sh[k];
            fr_store(sclds, (size_t)k * E + i, fr_load(in.t[k], at));
        }
    __syncthreads();
    unsigned L = E;
    for (int rd = 0; rd < rounds; rd++) {
        const unsigned h = L >> 1;
        const Fr r = fr_load(chal.c, rd);
        Fr acc[K::kEvals];
#pragma unroll
        for (int t = 0; t < K::kEvals; t++) acc[t] = fp_zero<FrCfg>();
        for (unsigned j = tid; j < h; j += kGateBlock) {
            Fr v[K::kTabs], d[K::kTabs];
#pragma unroll
            for (int k = 0; k < K::kTabs; k++) {
                v[k] = fr_load(sclds, (size_t)k * E + j);
                d[k] = fr_sub(fr_load(sclds, (size_t)k * E + j + h), v[k]);
                fr_store(sclds, (size_t)k * E + j, fr_add(v[k], fr_mul(r, d[k])));
            }
            kind_sums_fr<K>(acc, gamma.r, v, d);
        }
        uint4* rs = red + 2 * (size_t)(rd & 1) * (kGateBlock / 64) * K::kEvals;
        gate_wave_store_fr(acc, rs);
        __syncthreads();
        if (tid < K::kEvals) {
            Fr s = fr_load(rs, tid);
            for (int g = 1; g < kGateBlock / 64; g++) s = fr_add(s, fr_load(rs, (size_t)g * K::kEvals + tid));
            fr_store(evals, (size_t)rd * K::kEvals + tid, s);
        }
        L = h;
    }
    if (tid < K::kTabs) fr_store(last, tid, fr_load(sclds, (size_t)tid * E));
}

// ---------------------------------------------------------------------------------------
// The host driver of a call.  who: the C ABI's name of the call, noun: how its refusal names the length ("table length ", "N = ").
// b: the identity's binding of the caller's arguments (Bound, zk_gate.cuh); its *_local_e knob, the hand-over length, is checked after
// the length, as every refusal of the length names the call.  h_chal: one challenge per round.
// ---------------------------------------------------------------------------------------
template <class K>
static int run_preset(zk_ctx* ctx, const char* who, const char* noun, const Bound<K>& b, size_t len, const uint64_t* h_chal, uint64_t* h_out_evals, uint64_t* h_last) {
    const GateChal& gamma = b.gamma;
    const size_t per_cu = b.per_cu;
    if (len < 2 || (len & (len - 1))) return fail(ctx, ZK_ERR_INVALID, "%s: %s%zu is not a power of two >= 2", who, noun, len);
    size_t rounds = 0;
    while (((size_t)1 << rounds) < len) rounds++;
    if (rounds > (size_t)kGateMaxLog) return fail(ctx, ZK_ERR_INVALID, "%s: tables longer than 2^%d elements", who, kGateMaxLog);
    size_t emax;
    const int rc = local_e(ctx, b.knob, b.knob_name, emax, K::kLocalMax);
    if (rc) return rc;
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    // plan: passes while the tables are longer than emax
    size_t npass = 0, part_slots = 0;
    GateReducePlan rp;
    std::memset(&rp, 0, sizeof(rp));
    size_t blocks_of[kGateMaxPasses];
    for (size_t m = len; m > emax; m >>= 1) {
        if (npass == (size_t)kGateMaxPasses) return fail(ctx, ZK_ERR_INVALID, "%s: table too long", who);
        const size_t blocks = std::min<size_t>(((m >> 1) + kGateBlock - 1) / kGateBlock, (size_t)ctx->cu_count * per_cu);
        blocks_of[npass] = blocks;
        rp.nbw[npass] = (unsigned)(blocks * (kGateBlock / 64));
        rp.off[npass] = (unsigned)part_slots;
        part_slots += (size_t)K::kEvals * rp.nbw[npass];
        npass++;
    }
    const size_t fr = 32;
    char* res = (char*)pinned(ctx, (rounds * K::kEvals + K::kTabs) * fr);  // evaluations | last: the kernels write them straight into pinned host memory
    if (!res) return ZK_ERR_OOM;
    char* res_last = res + rounds * K::kEvals * fr;
    char* buf[2] = {nullptr, nullptr};
    char* part = nullptr;
    if (npass) {
        // ping-pong tables: kTabs of len/2 and kTabs of len/4 elements; one 544-bit partial per wave, evaluation and pass
        if (!(buf[0] = (char*)scratch(ctx, 0, K::kTabs * (len / 2) * fr))) return ZK_ERR_OOM;
        if (npass > 1 && !(buf[1] = (char*)scratch(ctx, 1, K::kTabs * (len / 4) * fr))) return ZK_ERR_OOM;
        if (!(part = (char*)scratch(ctx, 4, part_slots * kGateWideBytes))) return ZK_ERR_OOM;
    }
    FsIn<K::kTabs> cur = b.first;
    for (size_t p = 0; p < npass; p++) {
        FsOut<K::kTabs> o;
        for (int k = 0; k < K::kTabs; k++) o.t[k] = buf[p & 1] + (size_t)k * ((p & 1) ? len / 4 : len / 2) * fr;
        GateChal ch;
        std::memcpy(&ch.r, h_chal + 4 * p, 32);
        hipLaunchKernelGGL(k_sc_pass<K>, dim3((unsigned)blocks_of[p]), dim3(kGateBlock), 0, ctx->stream, cur, o, len >> (p + 1), ch, gamma,
                           (void*)(part + (size_t)rp.off[p] * kGateWideBytes));
        ZK_HIP(ctx, hipGetLastError());
        for (int k = 0; k < K::kTabs; k++) cur.t[k] = o.t[k], cur.sh[k] = 0;
    }
    if (npass) {
        hipLaunchKernelGGL(k_sc_reduce<K>, dim3(K::kEvals, (unsigned)npass), dim3(kGateBlock), 0, ctx->stream, (const void*)part, rp, (void*)res);
        ZK_HIP(ctx, hipGetLastError());
    }
    {
        const size_t E = len >> npass;
        const int rl = (int)(rounds - npass);
        GateTail tl;
        std::memset(&tl, 0, sizeof(tl));
        std::memcpy(tl.c, h_chal + 4 * npass, (size_t)rl * 32);
        const size_t lds = (2 * (size_t)K::kTabs * E + 2 * 2 * (kGateBlock / 64) * K::kEvals) * sizeof(uint4);
        if (lds > 64 * 1024 && !ctx->preset_lds_raised[K::kSlot]) {  // once per ctx (= per device)
            ZK_HIP(ctx, hipFuncSetAttribute((const void*)k_sc_local<K>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            ctx->preset_lds_raised[K::kSlot] = true;
        }
        hipLaunchKernelGGL(k_sc_local<K>, dim3(1), dim3(kGateBlock), lds, ctx->stream, cur, (unsigned)E, rl, tl, gamma, (void*)(res + npass * K::kEvals * fr),
                           (void*)res_last);
        ZK_HIP(ctx, hipGetLastError());
    }
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(h_out_evals, res, rounds * K::kEvals * fr);
    std::memcpy(h_last, res_last, K::kTabs * fr);
    return ZK_OK;
}

}  // namespace zk
