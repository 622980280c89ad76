// zk_gatew.hip -- the WIDE Plonk gate as one ZeroCheck sumcheck.  With N = 2^mu rows, six selectors and the three wires
//   W(x) = eq(x) [ qL a + qR b + qM a b + qH a^5 - qO c + qC + in ],
//   K14  wide gate sumcheck   degree 7 per variable (qH a^5 is degree 6, eq adds one): EIGHT evaluations of the round polynomial
//                             (t = 0 .. 7) per round, eleven tables folded (eq, qL, qR, qM, qO, qC, qH, a, b, c, in).
// A constant selector, separate weights of the two additive wires, an output selector and a fifth-power term: an S-box row
// c = a^5 + const (Poseidon, Rescue) is ONE row, and the sumcheck prover pays for the degree with evaluations, not with a larger FFT.
//
// Conventions and shape of zk_perm3.hip: Fr in Montgomery form, 32-byte AoS elements, round i binds the TOP index bit, inputs are
// never written, all sums are exact modular sums; one HBM pass per round while the tables are long (k_gatew_pass), the eight sums of a
// pass as 544-bit integers reduced in one launch per call (k_gatew_reduce), then every remaining round in one workgroup on tables
// held in LDS (k_gatew_local).  Eleven tables of 512 elements would be 176 KiB, more than the CU's 160 KiB of LDS: the hand-over is
// at most kGatewLocalMax = 256 elements (88 KiB).
//
// Registers of k_gatew_pass: eleven (value, difference) pairs are 176 VGPRs and eight 17-limb sums 136 more, so the kernel is compiled
// for one wave per SIMD (the 264 .. 512 register bracket) and launched with one workgroup per CU.  It does not spill.
#include "zk_gate.cuh"

#include <algorithm>
#include <cstring>

namespace zk {

using GatewIn = FsIn<kGatewTabs>;
using GatewOut = FsOut<kGatewTabs>;

// ---------------------------------------------------------------------------------------
// One round over tables of length 2 * half living in HBM.  partials: [t * nbw + 4 block + wave], 80-byte slots.
// The values at t = 1 .. 7 come from v(t) = v(t-1) + (hi - lo): per t ten multiplications (nine reduced ones inside the bracket,
// the product with eq left as an integer for the lazily reduced sum), with the eleven folds 11 + 8 x 10 = 91 per index pair.
// Capacity of the sums as in k_gate_pass: a product eq x (reduced bracket) is < r^2 < 2^510, a 544-bit sum holds 2^34 of them,
// hence len <= 2^35.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kGateBlock) __attribute__((amdgpu_waves_per_eu(1, 1)))
k_gatew_pass(GatewIn in, GatewOut out, size_t half, GateChal ch, void* __restrict__ partials) {
    u32 w[kGatewEvals][17];
#pragma unroll
    for (int t = 0; t < kGatewEvals; t++)
#pragma unroll
        for (int i = 0; i < 17; i++) w[t][i] = 0;
    for (size_t j = (size_t)blockIdx.x * kGateBlock + threadIdx.x; j < half; j += (size_t)gridDim.x * kGateBlock) {
        Fr v[kGatewTabs], d[kGatewTabs];
#pragma unroll
        for (int k = 0; k < kGatewTabs; k++) {
            v[k] = fr_load(in.t[k], j);
            d[k] = fr_sub(fr_load(in.t[k], j + half), v[k]);
            fr_store(out.t[k], j, fr_add(v[k], fr_mul(ch.r, d[k])));  // lo + r (hi - lo)   dsumcheck.rs:14-19
        }
#pragma unroll
        for (int t = 0; t < kGatewEvals; t++) {
            fp_mac_wide(w[t], v[0], gatew_inner(v));
            if (t + 1 < kGatewEvals) {
#pragma unroll
                for (int k = 0; k < kGatewTabs; k++) v[k] = fr_add(v[k], d[k]);
            }
        }
    }
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t nbw = (size_t)gridDim.x * (kGateBlock / 64);
#pragma unroll
    for (int t = 0; t < kGatewEvals; t++) {
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

// The sums of all passes of a call in one launch: block (t, p) = evaluation t of pass p (gate_reduce_block, zk_gate.cuh).
__global__ void __launch_bounds__(kGateBlock) k_gatew_reduce(const void* __restrict__ partials, GateReducePlan plan, void* __restrict__ evals) {
    __shared__ uint4 lds[(kGateBlock / 64) * (kGateWideBytes / 16)];
    const unsigned t = blockIdx.x, p = blockIdx.y, nbw = plan.nbw[p];
    gate_reduce_block(partials, (size_t)plan.off[p] + (size_t)t * nbw, nbw, lds, evals, (size_t)p * kGatewEvals + t);
}

// ---------------------------------------------------------------------------------------
// Local stage: all remaining rounds of tables of E <= 256 elements in one workgroup, as k_perm3_local: the eleven tables sit in
// LDS and are folded in place (a lane reads elements j and j + h of each and writes j: no other lane touches either before the
// round's barrier).  Sums of a round: wave shuffle, one LDS slot per wave (two sets, by round parity), eight lanes finish them.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kGateBlock) k_gatew_local(GatewIn in, unsigned E, int rounds, GateTail chal, void* __restrict__ evals, void* __restrict__ last) {
    extern __shared__ uint4 wlds[];
    uint4* red = wlds + 2 * (size_t)kGatewTabs * E;  // [parity][wave][t] Fr
    const unsigned tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (unsigned i = tid; i < E; i += kGateBlock)
#pragma unroll
        for (int k = 0; k < kGatewTabs; k++) fr_store(wlds, (size_t)k * E + i, fr_load(in.t[k], i));
    __syncthreads();
    unsigned L = E;
    for (int rd = 0; rd < rounds; rd++) {
        const unsigned h = L >> 1;
        const Fr r = fr_load(chal.c, rd);
        Fr acc[kGatewEvals];
#pragma unroll
        for (int t = 0; t < kGatewEvals; t++) acc[t] = fp_zero<FrCfg>();
        for (unsigned j = tid; j < h; j += kGateBlock) {
            Fr v[kGatewTabs], d[kGatewTabs];
#pragma unroll
            for (int k = 0; k < kGatewTabs; k++) {
                v[k] = fr_load(wlds, (size_t)k * E + j);
                d[k] = fr_sub(fr_load(wlds, (size_t)k * E + j + h), v[k]);
                fr_store(wlds, (size_t)k * E + j, fr_add(v[k], fr_mul(r, d[k])));
            }
#pragma unroll
            for (int t = 0; t < kGatewEvals; t++) {
                acc[t] = fr_add(acc[t], fr_mul(v[0], gatew_inner(v)));
                if (t + 1 < kGatewEvals) {
#pragma unroll
                    for (int k = 0; k < kGatewTabs; k++) v[k] = fr_add(v[k], d[k]);
                }
            }
        }
        uint4* rs = red + 2 * (size_t)(rd & 1) * (kGateBlock / 64) * kGatewEvals;
#pragma unroll
        for (int t = 0; t < kGatewEvals; t++) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                Fr o;
#pragma unroll
                for (int i = 0; i < 8; i++) o.l[i] = __shfl_down(acc[t].l[i], off, 64);
                acc[t] = fr_add(acc[t], o);
            }
            if (lane == 0) fr_store(rs, (size_t)wave * kGatewEvals + t, acc[t]);
        }
        __syncthreads();
        if (tid < kGatewEvals) {
            Fr s = fr_load(rs, tid);
            for (int g = 1; g < kGateBlock / 64; g++) s = fr_add(s, fr_load(rs, (size_t)g * kGatewEvals + tid));
            fr_store(evals, (size_t)rd * kGatewEvals + tid, s);
        }
        L = h;
    }
    if (tid < kGatewTabs) fr_store(last, tid, fr_load(wlds, (size_t)tid * E));
}

// ---------------------------------------------------------------------------------------
// host driver
// ---------------------------------------------------------------------------------------
int sumcheck_gate_wide(zk_ctx* ctx, const void* const* d_tabs, size_t len, const uint64_t* h_chal, uint64_t* h_out_evals, uint64_t* h_last) {
    if (len < 2 || (len & (len - 1))) return fail(ctx, ZK_ERR_INVALID, "zk_sumcheck_gate_wide: table length %zu is not a power of two >= 2", len);
    size_t rounds = 0;
    while (((size_t)1 << rounds) < len) rounds++;
    if (rounds > (size_t)kGateMaxLog) return fail(ctx, ZK_ERR_INVALID, "zk_sumcheck_gate_wide: tables longer than 2^%d elements", kGateMaxLog);
    // hand-over point to the local stage (knob gatew_local_e: 1 = HBM passes down to the last element)
    size_t emax = (size_t)tuning().gatew_local_e;
    if (emax < 1 || emax > kGatewLocalMax || (emax & (emax - 1))) return fail(ctx, ZK_ERR_INVALID, "gatew_local_e must be a power of two in [1, %u]", kGatewLocalMax);
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    // plan: passes while the tables are longer than emax
    size_t npass = 0, part_slots = 0;
    GateReducePlan rp;
    std::memset(&rp, 0, sizeof(rp));
    size_t blocks_of[kGateMaxPasses];
    const size_t per_cu = 1;  // the pass is compiled for one wave per SIMD: one workgroup of four waves fills a CU
    for (size_t m = len; m > emax; m >>= 1) {
        if (npass == (size_t)kGateMaxPasses) return fail(ctx, ZK_ERR_INVALID, "zk_sumcheck_gate_wide: table too long");
        const size_t half = m >> 1;
        const size_t blocks = std::min<size_t>((half + kGateBlock - 1) / kGateBlock, (size_t)ctx->cu_count * per_cu);
        blocks_of[npass] = blocks;
        rp.nbw[npass] = (unsigned)(blocks * (kGateBlock / 64));
        rp.off[npass] = (unsigned)part_slots;
        part_slots += (size_t)kGatewEvals * rp.nbw[npass];
        npass++;
    }
    const size_t fr = 32;
    const size_t res_bytes = (rounds * kGatewEvals + kGatewTabs) * fr;
    char* res = (char*)pinned(ctx, res_bytes);  // the kernels write the results straight into pinned host memory
    if (!res) return ZK_ERR_OOM;
    char* buf[2] = {nullptr, nullptr};
    char* part = nullptr;
    if (npass) {
        // the arenas of the gate sumcheck: ping-pong tables (eleven of len/2 and eleven of len/4 elements) and the 544-bit partials
        if (!(buf[0] = (char*)scratch(ctx, 0, kGatewTabs * (len / 2) * fr))) return ZK_ERR_OOM;
        if (npass > 1 && !(buf[1] = (char*)scratch(ctx, 1, kGatewTabs * (len / 4) * fr))) return ZK_ERR_OOM;
        if (!(part = (char*)scratch(ctx, 4, part_slots * kGateWideBytes))) return ZK_ERR_OOM;
    }
    GatewIn cur;
    for (int k = 0; k < kGatewTabs; k++) cur.t[k] = d_tabs[k], cur.sh[k] = 0;
    size_t m = len;
    for (size_t p = 0; p < npass; p++) {
        const size_t half = m >> 1;
        GatewOut o;
        for (int k = 0; k < kGatewTabs; k++) o.t[k] = buf[p & 1] + (size_t)k * ((p & 1) ? len / 4 : len / 2) * fr;
        GateChal ch;
        std::memcpy(&ch.r, h_chal + 4 * p, 32);
        hipLaunchKernelGGL(k_gatew_pass, dim3((unsigned)blocks_of[p]), dim3(kGateBlock), 0, ctx->stream, cur, o, half, ch, (void*)(part + (size_t)rp.off[p] * kGateWideBytes));
        ZK_HIP(ctx, hipGetLastError());
        for (int k = 0; k < kGatewTabs; k++) cur.t[k] = o.t[k];
        m = half;
    }
    if (npass) {
        hipLaunchKernelGGL(k_gatew_reduce, dim3(kGatewEvals, (unsigned)npass), dim3(kGateBlock), 0, ctx->stream, (const void*)part, rp, (void*)res);
        ZK_HIP(ctx, hipGetLastError());
    }
    {
        const int rl = (int)(rounds - npass);
        GateTail tl;
        std::memset(&tl, 0, sizeof(tl));
        std::memcpy(tl.c, h_chal + 4 * npass, (size_t)rl * 32);
        const size_t lds = (2 * (size_t)kGatewTabs * m + 2 * 2 * (kGateBlock / 64) * kGatewEvals) * sizeof(uint4);
        if (lds > 64 * 1024 && !ctx->gatew_lds_raised) {  // once per ctx (= per device)
            ZK_HIP(ctx, hipFuncSetAttribute((const void*)k_gatew_local, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            ctx->gatew_lds_raised = true;
        }
        hipLaunchKernelGGL(k_gatew_local, dim3(1), dim3(kGateBlock), lds, ctx->stream, cur, (unsigned)m, rl, tl, (void*)(res + npass * kGatewEvals * fr),
                           (void*)(res + rounds * kGatewEvals * fr));
        ZK_HIP(ctx, hipGetLastError());
    }
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(h_out_evals, res, rounds * kGatewEvals * fr);
    std::memcpy(h_last, res + rounds * kGatewEvals * fr, kGatewTabs * fr);
    return ZK_OK;
}

}  // namespace zk
