// zk_gate.hip -- the gate identity of HyperPlonk as ONE sumcheck (the virtual circuit the reference simulates with six
// independent product sumchecks, hyperplonk/src/hyperplonk.rs:66-93, dhyperplonk.rs:218-260):
//   K9   eq table            out[x] = prod_i (x_i ? tau_i : 1 - tau_i), built by doubling,
//   K10  gate sumcheck       G(x) = eq(x) [ q1(x) (a(x) + b(x)) + q2(x) a(x) b(x) - c(x) + in(x) ], degree 4 per variable:
//                            five evaluations of the round polynomial (t = 0 .. 4) per round, seven tables folded.
//
// Conventions of zk_fr.hip: Fr in Montgomery form, 32-byte AoS elements, round i binds the TOP index bit (lo = tab[..m/2],
// hi = tab[m/2..]), inputs are never written, all sums are exact modular sums (any association order gives the same bits).
//
// Shape: one HBM pass per round while the tables are long (k_gate_pass: a lane owns output index j, reads the lo / hi halves
// of the seven tables, writes the seven folded elements to ping-pong scratch and adds its five products eq(t) * [..](t) as
// 512-bit integers into five 544-bit sums -- one Montgomery reduction per sum and call, in k_gate_reduce), then every
// remaining round in one workgroup on tables held in LDS (k_gate_local).
#include "zk_gate.cuh"

#include <algorithm>
#include <cstring>

namespace zk {

static constexpr int kGateTabs = 7;     // eq, q1, q2, a, b, c, in
static constexpr int kGateEvals = 5;    // t = 0 .. 4

struct GateIn {
    const void* t[kGateTabs];
};
struct GateOut {
    void* t[kGateTabs];
};

// ---------------------------------------------------------------------------------------
// One round over tables of length 2 * half living in HBM.  partials: [t * nbw + 4 block + wave], 80-byte slots.
// The values at t = 1 .. 4 come from v(t) = v(t-1) + (hi - lo): per t four multiplications (three reduced ones inside the
// bracket, the product with eq left as an integer for the lazily reduced sum).  A product of two elements < r is < r^2 < 2^510, so a
// 544-bit sum holds 2^34 of them; k_gate_reduce adds ALL len/2 products of a pass into one such value, hence len <= 2^35
// (kGateMaxLog: sumcheck_gate refuses longer tables -- 7 x 32 B x 2^35 is beyond any HBM anyway).
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kGateBlock) __attribute__((amdgpu_waves_per_eu(1, 2)))
k_gate_pass(GateIn in, GateOut out, size_t half, GateChal ch, void* __restrict__ partials) {
    u32 w[kGateEvals][17];
#pragma unroll
    for (int t = 0; t < kGateEvals; t++)
#pragma unroll
        for (int i = 0; i < 17; i++) w[t][i] = 0;
    for (size_t j = (size_t)blockIdx.x * kGateBlock + threadIdx.x; j < half; j += (size_t)gridDim.x * kGateBlock) {
        Fr v[kGateTabs], d[kGateTabs];
#pragma unroll
        for (int k = 0; k < kGateTabs; k++) {
            v[k] = fr_load(in.t[k], j);
            d[k] = fr_sub(fr_load(in.t[k], j + half), v[k]);
            fr_store(out.t[k], j, fr_add(v[k], fr_mul(ch.r, d[k])));  // lo + r (hi - lo)   dsumcheck.rs:14-19
        }
#pragma unroll
        for (int t = 0; t < kGateEvals; t++) {
            fp_mac_wide(w[t], v[0], gate_inner(v[1], v[2], v[3], v[4], v[5], v[6]));
            if (t + 1 < kGateEvals) {
#pragma unroll
                for (int k = 0; k < kGateTabs; k++) v[k] = fr_add(v[k], d[k]);
            }
        }
    }
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t nbw = (size_t)gridDim.x * (kGateBlock / 64);
#pragma unroll
    for (int t = 0; t < kGateEvals; t++) {
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

// The sums of all passes of a call in one launch: block (t, p) adds the per-wave partials of evaluation t of pass p and
// reduces them (gate_reduce_block, zk_gate.cuh).
__global__ void __launch_bounds__(kGateBlock) k_gate_reduce(const void* __restrict__ partials, GateReducePlan plan, void* __restrict__ evals) {
    __shared__ uint4 lds[(kGateBlock / 64) * (kGateWideBytes / 16)];
    const unsigned t = blockIdx.x, p = blockIdx.y, nbw = plan.nbw[p];
    gate_reduce_block(partials, (size_t)plan.off[p] + (size_t)t * nbw, nbw, lds, evals, (size_t)p * kGateEvals + t);
}

// ---------------------------------------------------------------------------------------
// Local stage: all remaining rounds of tables of E <= 512 elements in one workgroup.  The seven tables sit in LDS and are
// folded in place (a lane reads elements t and t + h of each and writes t: no other lane touches either before the round's
// barrier).  Sums of a round: wave shuffle, one LDS slot per wave (two sets, by round parity), five lanes finish them.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kGateBlock) k_gate_local(GateIn in, unsigned E, int rounds, GateTail chal, void* __restrict__ evals,
                                                          void* __restrict__ last) {
    extern __shared__ uint4 glds[];
    uint4* red = glds + 2 * (size_t)kGateTabs * E;  // [parity][wave][t] Fr
    const unsigned tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (unsigned t = tid; t < E; t += kGateBlock)
#pragma unroll
        for (int k = 0; k < kGateTabs; k++) fr_store(glds, (size_t)k * E + t, fr_load(in.t[k], t));
    __syncthreads();
    unsigned L = E;
    for (int rd = 0; rd < rounds; rd++) {
        const unsigned h = L >> 1;
        const Fr r = fr_load(chal.c, rd);
        Fr acc[kGateEvals];
#pragma unroll
        for (int t = 0; t < kGateEvals; t++) acc[t] = fp_zero<FrCfg>();
        for (unsigned j = tid; j < h; j += kGateBlock) {
            Fr v[kGateTabs], d[kGateTabs];
#pragma unroll
            for (int k = 0; k < kGateTabs; k++) {
                v[k] = fr_load(glds, (size_t)k * E + j);
                d[k] = fr_sub(fr_load(glds, (size_t)k * E + j + h), v[k]);
                fr_store(glds, (size_t)k * E + j, fr_add(v[k], fr_mul(r, d[k])));
            }
#pragma unroll
            for (int t = 0; t < kGateEvals; t++) {
                acc[t] = fr_add(acc[t], fr_mul(v[0], gate_inner(v[1], v[2], v[3], v[4], v[5], v[6])));
                if (t + 1 < kGateEvals) {
#pragma unroll
                    for (int k = 0; k < kGateTabs; k++) v[k] = fr_add(v[k], d[k]);
                }
            }
        }
        uint4* rs = red + 2 * (size_t)(rd & 1) * (kGateBlock / 64) * kGateEvals;
#pragma unroll
        for (int t = 0; t < kGateEvals; t++) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                Fr o;
#pragma unroll
                for (int i = 0; i < 8; i++) o.l[i] = __shfl_down(acc[t].l[i], off, 64);
                acc[t] = fr_add(acc[t], o);
            }
            if (lane == 0) fr_store(rs, (size_t)wave * kGateEvals + t, acc[t]);
        }
        __syncthreads();
        if (tid < kGateEvals) {
            Fr s = fr_load(rs, tid);
            for (int g = 1; g < kGateBlock / 64; g++) s = fr_add(s, fr_load(rs, (size_t)g * kGateEvals + tid));
            fr_store(evals, (size_t)rd * kGateEvals + tid, s);
        }
        L = h;
    }
    if (tid < kGateTabs) fr_store(last, tid, fr_load(glds, (size_t)tid * E));
}

// ---------------------------------------------------------------------------------------
// eq table by doubling, from the LAST variable to the first: the table of (tau_k .. tau_{n-1}) has 2^(n-k) entries, and
// taking tau_{k-1} in as the new top bit is  out[j + size] = out[j] tau,  out[j] = out[j] - out[j + size]  -- in place, one
// multiplication per two outputs.  k_eq_seed builds the first levels (up to 2^10 entries) in one workgroup.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(1024) k_eq_seed(void* __restrict__ out, GateTail tau, int levels, GateChal seed) {
    const unsigned tid = threadIdx.x;
    if (tid == 0) fr_store(out, 0, seed.r);  // 1 (zk_eq_table), or the weight of zk_eq_table_acc (zk_batchopen.hip)
    __syncthreads();
    for (int k = 0; k < levels; k++) {  // tau.c[k]: the variable taken in at level k (the last one first)
        const unsigned size = 1u << k;
        if (tid < size) {
            const Fr lo = fr_load(out, tid), hi = fr_mul(lo, fr_load(tau.c, k));
            fr_store(out, tid + size, hi);
            fr_store(out, tid, fr_sub(lo, hi));
        }
        __syncthreads();
    }
}
__global__ void __launch_bounds__(kGateBlock) k_eq_double(void* __restrict__ out, size_t size, GateChal tau) {
    for (size_t j = (size_t)blockIdx.x * kGateBlock + threadIdx.x; j < size; j += (size_t)gridDim.x * kGateBlock) {
        const Fr lo = fr_load(out, j), hi = fr_mul(lo, tau.r);
        fr_store(out, j + size, hi);
        fr_store(out, j, fr_sub(lo, hi));
    }
}

// ---------------------------------------------------------------------------------------
// host drivers
// ---------------------------------------------------------------------------------------
static const uint64_t kFrOneMont[4] = {0x00000001fffffffeULL, 0x5884b7fa00034802ULL, 0x998c4fefecbc4ff5ULL, 0x1824b159acc5056fULL};  // R mod r

int eq_table(zk_ctx* ctx, const uint64_t* h_point, size_t n, void* d_out) { return eq_table_seeded(ctx, h_point, n, kFrOneMont, d_out); }

// d_out[x] = seed * eq(point, x): the doubling scheme started from `seed` instead of 1
int eq_table_seeded(zk_ctx* ctx, const uint64_t* h_point, size_t n, const uint64_t* h_seed, void* d_out) {
    if (n > 40) return fail(ctx, ZK_ERR_INVALID, "eq table of %zu variables (at most 40)", n);
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    GateChal sd;
    std::memcpy(&sd.r, h_seed, 32);
    const int seed = (int)(n < 10 ? n : 10);
    GateTail tl;
    std::memset(&tl, 0, sizeof(tl));
    for (int k = 0; k < seed; k++) std::memcpy(tl.c + 4 * k, h_point + 4 * (n - 1 - k), 32);
    hipLaunchKernelGGL(k_eq_seed, dim3(1), dim3(1024), 0, ctx->stream, d_out, tl, seed, sd);
    ZK_HIP(ctx, hipGetLastError());
    for (size_t k = seed; k < n; k++) {
        const size_t size = (size_t)1 << k;
        GateChal t;
        std::memcpy(&t.r, h_point + 4 * (n - 1 - k), 32);
        const size_t blocks = std::min<size_t>((size + kGateBlock - 1) / kGateBlock, (size_t)ctx->cu_count * 16);
        hipLaunchKernelGGL(k_eq_double, dim3((unsigned)blocks), dim3(kGateBlock), 0, ctx->stream, d_out, size, t);
        ZK_HIP(ctx, hipGetLastError());
    }
    return ZK_OK;
}

int sumcheck_gate(zk_ctx* ctx, const void* const* d_tabs, size_t len, const uint64_t* h_chal, uint64_t* h_out_evals, uint64_t* h_last) {
    if (len < 2 || (len & (len - 1))) return fail(ctx, ZK_ERR_INVALID, "zk_sumcheck_gate: table length %zu is not a power of two >= 2", len);
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    size_t rounds = 0;
    while (((size_t)1 << rounds) < len) rounds++;
    if (rounds > (size_t)kGateMaxLog) return fail(ctx, ZK_ERR_INVALID, "zk_sumcheck_gate: tables longer than 2^%d elements", kGateMaxLog);
    // hand-over point to the local stage (knob gate_local_e: 1 = HBM passes down to the last element)
    size_t emax = (size_t)tuning().gate_local_e;
    if (emax < 1 || emax > kGateLocalMax || (emax & (emax - 1))) return fail(ctx, ZK_ERR_INVALID, "gate_local_e must be a power of two in [1, %u]", kGateLocalMax);
    // plan: passes while the tables are longer than emax
    size_t npass = 0, part_slots = 0;
    GateReducePlan rp;
    std::memset(&rp, 0, sizeof(rp));
    size_t blocks_of[kGateMaxPasses];
    const size_t per_cu = tuning().gate_pass_wg > 0 ? (size_t)tuning().gate_pass_wg : 2;
    for (size_t m = len; m > emax; m >>= 1) {
        if (npass == (size_t)kGateMaxPasses) return fail(ctx, ZK_ERR_INVALID, "zk_sumcheck_gate: table too long");
        const size_t half = m >> 1;
        const size_t blocks = std::min<size_t>((half + kGateBlock - 1) / kGateBlock, (size_t)ctx->cu_count * per_cu);
        blocks_of[npass] = blocks;
        rp.nbw[npass] = (unsigned)(blocks * (kGateBlock / 64));
        rp.off[npass] = (unsigned)part_slots;
        part_slots += (size_t)kGateEvals * rp.nbw[npass];
        npass++;
    }
    const size_t fr = 32;
    const size_t res_bytes = (rounds * kGateEvals + kGateTabs) * fr;
    char* res = (char*)pinned(ctx, res_bytes);  // the kernels write the results straight into pinned host memory
    if (!res) return ZK_ERR_OOM;
    char* buf[2] = {nullptr, nullptr};
    char* part = nullptr;
    if (npass) {
        // ping-pong tables: seven of len/2 and seven of len/4 elements; one 544-bit partial per wave, evaluation and pass
        if (!(buf[0] = (char*)scratch(ctx, 0, kGateTabs * (len / 2) * fr))) return ZK_ERR_OOM;
        if (npass > 1 && !(buf[1] = (char*)scratch(ctx, 1, kGateTabs * (len / 4) * fr))) return ZK_ERR_OOM;
        if (!(part = (char*)scratch(ctx, 4, part_slots * kGateWideBytes))) return ZK_ERR_OOM;
    }
    GateIn cur;
    for (int k = 0; k < kGateTabs; k++) cur.t[k] = d_tabs[k];
    size_t m = len;
    for (size_t p = 0; p < npass; p++) {
        const size_t half = m >> 1;
        GateOut o;
        for (int k = 0; k < kGateTabs; k++) o.t[k] = buf[p & 1] + (size_t)k * ((p & 1) ? len / 4 : len / 2) * fr;
        GateChal ch;
        std::memcpy(&ch.r, h_chal + 4 * p, 32);
        hipLaunchKernelGGL(k_gate_pass, dim3((unsigned)blocks_of[p]), dim3(kGateBlock), 0, ctx->stream, cur, o, half, ch,
                           (void*)(part + (size_t)rp.off[p] * kGateWideBytes));
        ZK_HIP(ctx, hipGetLastError());
        for (int k = 0; k < kGateTabs; k++) cur.t[k] = o.t[k];
        m = half;
    }
    if (npass) {
        hipLaunchKernelGGL(k_gate_reduce, dim3(kGateEvals, (unsigned)npass), dim3(kGateBlock), 0, ctx->stream, (const void*)part, rp, (void*)res);
        ZK_HIP(ctx, hipGetLastError());
    }
    {
        const int rl = (int)(rounds - npass);
        GateTail tl;
        std::memset(&tl, 0, sizeof(tl));
        std::memcpy(tl.c, h_chal + 4 * npass, (size_t)rl * 32);
        const size_t lds = (2 * (size_t)kGateTabs * m + 2 * 2 * (kGateBlock / 64) * kGateEvals) * sizeof(uint4);
        if (lds > 64 * 1024 && !ctx->gate_lds_raised) {  // once per ctx (= per device)
            ZK_HIP(ctx, hipFuncSetAttribute((const void*)k_gate_local, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            ctx->gate_lds_raised = true;
        }
        hipLaunchKernelGGL(k_gate_local, dim3(1), dim3(kGateBlock), lds, ctx->stream, cur, (unsigned)m, rl, tl, (void*)(res + npass * kGateEvals * fr),
                           (void*)(res + rounds * kGateEvals * fr));
        ZK_HIP(ctx, hipGetLastError());
    }
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(h_out_evals, res, rounds * kGateEvals * fr);
    std::memcpy(h_last, res + rounds * kGateEvals * fr, kGateTabs * fr);
    return ZK_OK;
}

}  // namespace zk
