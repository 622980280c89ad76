// zk_perm3.hip -- HyperPlonk's wiring identity over the THREE wire columns of a Plonk gate as ONE sumcheck.  With N = 2^mu rows and
// columns j = 0, 1, 2 (a, b, c), slot j N + x is wire j of row x and
//   n_j(x) = w_j(x) + alpha (j N + x) + beta,   d_j(x) = w_j(x) + alpha ssigma_j(x) + beta,   h = (n_0 n_1 n_2) / (d_0 d_1 d_2),
//   K12  derived tables      the six linear tables and P = n_0 n_1 n_2, Q = d_0 d_1 d_2 in one pass (k_perm3_terms); the slot number is
//                            formed in the kernel, no table of slot numbers exists.  h = zk_fr_batch_div(P, Q), v = zk_product_tree(h).
//   K13  perm3 sumcheck      F(x) = eq(x) [ v(1,x) - v(x,0) v(x,1) + gamma ( h(x) d_0 d_1 d_2 - n_0 n_1 n_2 ) ], degree 5 per variable:
//                            six evaluations of the round polynomial (t = 0 .. 5) per round, eleven tables folded
//                            (eq, v1x, vx0, vx1, h, n_0, n_1, n_2, d_0, d_1, d_2).
// The single-column form (zk_wiring.hip) needs the 3N slots laid out as one table of 4N elements: four times the index pairs and a
// product tree of 8N elements.  Here the tables keep N rows and the three columns are multiplied inside the bracket.
//
// Conventions and shape of zk_wiring.hip: Fr in Montgomery form, 32-byte AoS elements, round i binds the TOP index bit, inputs are
// never written, all sums are exact modular sums; one HBM pass per round while the tables are long (k_perm3_pass), the six sums of a
// pass as 544-bit integers reduced in one launch per call (k_perm3_reduce), then every remaining round in one workgroup on tables
// held in LDS (k_perm3_local).  The first pass reads the four views of v in place out of the tree (element i of a table is the Fr at
// t + 32 (i << sh): sh = 1 reads every other element).  Eleven tables of 512 elements would be 176 KiB, more than the CU's 160 KiB of
// LDS: the hand-over is at most kPerm3LocalMax = 256 elements (88 KiB).
//
// Registers of k_perm3_pass: eleven (value, difference) pairs are 176 VGPRs and six 17-limb sums 102 more, so the kernel is compiled
// for one wave per SIMD (the 264 .. 512 register bracket) and launched with one workgroup per CU.
#include "zk_gate.cuh"

#include <algorithm>
#include <cstring>

namespace zk {

using Perm3In = FsIn<kPerm3Tabs>;
using Perm3Out = FsOut<kPerm3Tabs>;
struct Perm3Cols {
    const void* w[3];
    const void* s[3];
    void* num[3];
    void* den[3];
};

// ---------------------------------------------------------------------------------------
// The derived tables in one pass: per row three w, three ssigma read; six linear tables, P and Q written.  alpha2 = alpha R (the
// Montgomery form of alpha's Montgomery form): its Montgomery product with the INTEGER j N + x is the Montgomery form of
// alpha (j N + x), one multiplication per slot.  j N + x < 3 * 2^35 sits in two limbs.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kGateBlock) k_perm3_terms(Perm3Cols c, size_t N, GateChal alpha, GateChal beta, void* __restrict__ P, void* __restrict__ Q) {
    Fr r2;
#pragma unroll
    for (int i = 0; i < 8; i++) r2.l[i] = FrCfg::R2(i);
    const Fr alpha2 = fr_mul(alpha.r, r2);
    for (size_t x = (size_t)blockIdx.x * kGateBlock + threadIdx.x; x < N; x += (size_t)gridDim.x * kGateBlock) {
        Fr n[3], d[3];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const Fr wb = fr_add(fr_load(c.w[j], x), beta.r);
            const unsigned long long slot = (unsigned long long)j * N + x;
            Fr id = fp_zero<FrCfg>();
            id.l[0] = (u32)slot, id.l[1] = (u32)(slot >> 32);
            n[j] = fr_add(wb, fr_mul(alpha2, id));
            d[j] = fr_add(wb, fr_mul(alpha.r, fr_load(c.s[j], x)));
            fr_store(c.num[j], x, n[j]);
            fr_store(c.den[j], x, d[j]);
        }
        fr_store(P, x, fr_mul(fr_mul(n[0], n[1]), n[2]));
        fr_store(Q, x, fr_mul(fr_mul(d[0], d[1]), d[2]));
    }
}

// ---------------------------------------------------------------------------------------
// One round over tables of length 2 * half living in HBM.  partials: [t * nbw + 4 block + wave], 80-byte slots.
// The values at t = 1 .. 5 come from v(t) = v(t-1) + (hi - lo): per t eight multiplications (seven reduced ones inside the bracket,
// the product with eq left as an integer for the lazily reduced sum), with the eleven folds 11 + 6 x 8 = 59 per index pair.
// Capacity of the sums as in k_wiring_pass: a product is < r^2 < 2^510, a 544-bit sum holds 2^34 of them, hence N <= 2^35.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kGateBlock) __attribute__((amdgpu_waves_per_eu(1, 1)))
k_perm3_pass(Perm3In in, Perm3Out out, size_t half, GateChal ch, GateChal gamma, void* __restrict__ partials) {
    u32 w[kPerm3Evals][17];
#pragma unroll
    for (int t = 0; t < kPerm3Evals; t++)
#pragma unroll
        for (int i = 0; i < 17; i++) w[t][i] = 0;
    for (size_t j = (size_t)blockIdx.x * kGateBlock + threadIdx.x; j < half; j += (size_t)gridDim.x * kGateBlock) {
        Fr v[kPerm3Tabs], d[kPerm3Tabs];
#pragma unroll
        for (int k = 0; k < kPerm3Tabs; k++) {
            const unsigned sh = in.sh[k];
            v[k] = fr_load(in.t[k], j << sh);
            d[k] = fr_sub(fr_load(in.t[k], (j + half) << sh), v[k]);
            fr_store(out.t[k], j, fr_add(v[k], fr_mul(ch.r, d[k])));  // lo + r (hi - lo)   dsumcheck.rs:14-19
        }
#pragma unroll
        for (int t = 0; t < kPerm3Evals; t++) {
            fp_mac_wide(w[t], v[0], perm3_inner(gamma.r, v));
            if (t + 1 < kPerm3Evals) {
#pragma unroll
                for (int k = 0; k < kPerm3Tabs; k++) v[k] = fr_add(v[k], d[k]);
            }
        }
    }
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t nbw = (size_t)gridDim.x * (kGateBlock / 64);
#pragma unroll
    for (int t = 0; t < kPerm3Evals; t++) {
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
__global__ void __launch_bounds__(kGateBlock) k_perm3_reduce(const void* __restrict__ partials, GateReducePlan plan, void* __restrict__ evals) {
    __shared__ uint4 lds[(kGateBlock / 64) * (kGateWideBytes / 16)];
    const unsigned t = blockIdx.x, p = blockIdx.y, nbw = plan.nbw[p];
    gate_reduce_block(partials, (size_t)plan.off[p] + (size_t)t * nbw, nbw, lds, evals, (size_t)p * kPerm3Evals + t);
}

// ---------------------------------------------------------------------------------------
// Local stage: all remaining rounds of tables of E <= 256 elements in one workgroup, as k_wiring_local: the eleven tables sit in
// LDS and are folded in place (a lane reads elements j and j + h of each and writes j: no other lane touches either before the
// round's barrier).  Sums of a round: wave shuffle, one LDS slot per wave (two sets, by round parity), six lanes finish them.
// The load honours in.sh, so a call whose N is at most the hand-over length reads the tree's views here.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kGateBlock) k_perm3_local(Perm3In in, unsigned E, int rounds, GateTail chal, GateChal gamma, void* __restrict__ evals,
                                                           void* __restrict__ last) {
    extern __shared__ uint4 plds[];
    uint4* red = plds + 2 * (size_t)kPerm3Tabs * E;  // [parity][wave][t] Fr
    const unsigned tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (unsigned i = tid; i < E; i += kGateBlock)
#pragma unroll
        for (int k = 0; k < kPerm3Tabs; k++) fr_store(plds, (size_t)k * E + i, fr_load(in.t[k], (size_t)i << in.sh[k]));
    __syncthreads();
    unsigned L = E;
    for (int rd = 0; rd < rounds; rd++) {
        const unsigned h = L >> 1;
        const Fr r = fr_load(chal.c, rd);
        Fr acc[kPerm3Evals];
#pragma unroll
        for (int t = 0; t < kPerm3Evals; t++) acc[t] = fp_zero<FrCfg>();
        for (unsigned j = tid; j < h; j += kGateBlock) {
            Fr v[kPerm3Tabs], d[kPerm3Tabs];
#pragma unroll
            for (int k = 0; k < kPerm3Tabs; k++) {
                v[k] = fr_load(plds, (size_t)k * E + j);
                d[k] = fr_sub(fr_load(plds, (size_t)k * E + j + h), v[k]);
                fr_store(plds, (size_t)k * E + j, fr_add(v[k], fr_mul(r, d[k])));
            }
#pragma unroll
            for (int t = 0; t < kPerm3Evals; t++) {
                acc[t] = fr_add(acc[t], fr_mul(v[0], perm3_inner(gamma.r, v)));
                if (t + 1 < kPerm3Evals) {
#pragma unroll
                    for (int k = 0; k < kPerm3Tabs; k++) v[k] = fr_add(v[k], d[k]);
                }
            }
        }
        uint4* rs = red + 2 * (size_t)(rd & 1) * (kGateBlock / 64) * kPerm3Evals;
#pragma unroll
        for (int t = 0; t < kPerm3Evals; t++) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                Fr o;
#pragma unroll
                for (int i = 0; i < 8; i++) o.l[i] = __shfl_down(acc[t].l[i], off, 64);
                acc[t] = fr_add(acc[t], o);
            }
            if (lane == 0) fr_store(rs, (size_t)wave * kPerm3Evals + t, acc[t]);
        }
        __syncthreads();
        if (tid < kPerm3Evals) {
            Fr s = fr_load(rs, tid);
            for (int g = 1; g < kGateBlock / 64; g++) s = fr_add(s, fr_load(rs, (size_t)g * kPerm3Evals + tid));
            fr_store(evals, (size_t)rd * kPerm3Evals + tid, s);
        }
        L = h;
    }
    if (tid < kPerm3Tabs) fr_store(last, tid, fr_load(plds, (size_t)tid * E));
}

// ---------------------------------------------------------------------------------------
// host drivers
// ---------------------------------------------------------------------------------------
int perm3_terms(zk_ctx* ctx, const void* const* d_w, const void* const* d_ssigma, size_t N, const uint64_t* h_alpha, const uint64_t* h_beta, void* const* d_num,
                void* const* d_den, void* d_P, void* d_Q) {
    if (N < 2 || (N & (N - 1))) return fail(ctx, ZK_ERR_INVALID, "zk_perm3_terms: N = %zu is not a power of two >= 2", N);
    if (N > ((size_t)1 << kGateMaxLog)) return fail(ctx, ZK_ERR_INVALID, "zk_perm3_terms: tables longer than 2^%d elements", kGateMaxLog);
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    Perm3Cols c;
    for (int j = 0; j < 3; j++) c.w[j] = d_w[j], c.s[j] = d_ssigma[j], c.num[j] = d_num[j], c.den[j] = d_den[j];
    GateChal al, be;
    std::memcpy(&al.r, h_alpha, 32);
    std::memcpy(&be.r, h_beta, 32);
    const size_t blocks = std::min<size_t>((N + kGateBlock - 1) / kGateBlock, (size_t)ctx->cu_count * 8);
    hipLaunchKernelGGL(k_perm3_terms, dim3((unsigned)blocks), dim3(kGateBlock), 0, ctx->stream, c, N, al, be, d_P, d_Q);
    ZK_HIP(ctx, hipGetLastError());
    return ZK_OK;
}

int sumcheck_perm3(zk_ctx* ctx, const void* d_eq, const void* d_tree, const void* const* d_num, const void* const* d_den, size_t N, const uint64_t* h_gamma,
                   const uint64_t* h_chal, uint64_t* h_out_evals, uint64_t* h_last) {
    if (N < 2 || (N & (N - 1))) return fail(ctx, ZK_ERR_INVALID, "zk_sumcheck_perm3: N = %zu is not a power of two >= 2", N);
    size_t rounds = 0;
    while (((size_t)1 << rounds) < N) rounds++;
    if (rounds > (size_t)kGateMaxLog) return fail(ctx, ZK_ERR_INVALID, "zk_sumcheck_perm3: tables longer than 2^%d elements", kGateMaxLog);
    // hand-over point to the local stage (knob perm3_local_e: 1 = HBM passes down to the last element)
    size_t emax = (size_t)tuning().perm3_local_e;
    if (emax < 1 || emax > kPerm3LocalMax || (emax & (emax - 1))) return fail(ctx, ZK_ERR_INVALID, "perm3_local_e must be a power of two in [1, %u]", kPerm3LocalMax);
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    // plan: passes while the tables are longer than emax
    size_t npass = 0, part_slots = 0;
    GateReducePlan rp;
    std::memset(&rp, 0, sizeof(rp));
    size_t blocks_of[kGateMaxPasses];
    const size_t per_cu = 1;  // the pass is compiled for one wave per SIMD: one workgroup of four waves fills a CU
    for (size_t m = N; m > emax; m >>= 1) {
        if (npass == (size_t)kGateMaxPasses) return fail(ctx, ZK_ERR_INVALID, "zk_sumcheck_perm3: table too long");
        const size_t half = m >> 1;
        const size_t blocks = std::min<size_t>((half + kGateBlock - 1) / kGateBlock, (size_t)ctx->cu_count * per_cu);
        blocks_of[npass] = blocks;
        rp.nbw[npass] = (unsigned)(blocks * (kGateBlock / 64));
        rp.off[npass] = (unsigned)part_slots;
        part_slots += (size_t)kPerm3Evals * rp.nbw[npass];
        npass++;
    }
    const size_t fr = 32;
    const size_t res_bytes = (rounds * kPerm3Evals + kPerm3Tabs) * fr;
    char* res = (char*)pinned(ctx, res_bytes);  // the kernels write the results straight into pinned host memory
    if (!res) return ZK_ERR_OOM;
    char* buf[2] = {nullptr, nullptr};
    char* part = nullptr;
    if (npass) {
        // the arenas of the gate sumcheck: ping-pong tables (eleven of N/2 and eleven of N/4 elements) and the 544-bit partials
        if (!(buf[0] = (char*)scratch(ctx, 0, kPerm3Tabs * (N / 2) * fr))) return ZK_ERR_OOM;
        if (npass > 1 && !(buf[1] = (char*)scratch(ctx, 1, kPerm3Tabs * (N / 4) * fr))) return ZK_ERR_OOM;
        if (!(part = (char*)scratch(ctx, 4, part_slots * kGateWideBytes))) return ZK_ERR_OOM;
    }
    GateChal gamma;
    std::memcpy(&gamma.r, h_gamma, 32);
    // the views of the tree: v1x its upper half, (vx0, vx1) every other element from its base / one element on, h its lower half
    const char* tree = (const char*)d_tree;
    Perm3In cur = {{d_eq, tree + N * fr, tree, tree + fr, tree, d_num[0], d_num[1], d_num[2], d_den[0], d_den[1], d_den[2]}, {0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0}};
    size_t m = N;
    for (size_t p = 0; p < npass; p++) {
        const size_t half = m >> 1;
        Perm3Out o;
        for (int k = 0; k < kPerm3Tabs; k++) o.t[k] = buf[p & 1] + (size_t)k * ((p & 1) ? N / 4 : N / 2) * fr;
        GateChal ch;
        std::memcpy(&ch.r, h_chal + 4 * p, 32);
        hipLaunchKernelGGL(k_perm3_pass, dim3((unsigned)blocks_of[p]), dim3(kGateBlock), 0, ctx->stream, cur, o, half, ch, gamma,
                           (void*)(part + (size_t)rp.off[p] * kGateWideBytes));
        ZK_HIP(ctx, hipGetLastError());
        for (int k = 0; k < kPerm3Tabs; k++) cur.t[k] = o.t[k], cur.sh[k] = 0;
        m = half;
    }
    if (npass) {
        hipLaunchKernelGGL(k_perm3_reduce, dim3(kPerm3Evals, (unsigned)npass), dim3(kGateBlock), 0, ctx->stream, (const void*)part, rp, (void*)res);
        ZK_HIP(ctx, hipGetLastError());
    }
    {
        const int rl = (int)(rounds - npass);
        GateTail tl;
        std::memset(&tl, 0, sizeof(tl));
        std::memcpy(tl.c, h_chal + 4 * npass, (size_t)rl * 32);
        const size_t lds = (2 * (size_t)kPerm3Tabs * m + 2 * 2 * (kGateBlock / 64) * kPerm3Evals) * sizeof(uint4);
        if (lds > 64 * 1024 && !ctx->perm3_lds_raised) {  // once per ctx (= per device)
            ZK_HIP(ctx, hipFuncSetAttribute((const void*)k_perm3_local, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            ctx->perm3_lds_raised = true;
        }
        hipLaunchKernelGGL(k_perm3_local, dim3(1), dim3(kGateBlock), lds, ctx->stream, cur, (unsigned)m, rl, tl, gamma,
                           (void*)(res + npass * kPerm3Evals * fr), (void*)(res + rounds * kPerm3Evals * fr));
        ZK_HIP(ctx, hipGetLastError());
    }
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(h_out_evals, res, rounds * kPerm3Evals * fr);
    std::memcpy(h_last, res + rounds * kPerm3Evals * fr, kPerm3Tabs * fr);
    return ZK_OK;
}

}  // namespace zk
