// zk_lookup.hip -- the lookup argument (LogUp): every value of a column f of N rows lies in a table t of N entries.
//   K15  multiplicities      m[y] = #{x : idx[x] = y} from the caller's row-to-table indices, checked against f and t on the way
//   K16  lookup sumcheck     L(x) = hf(x) - ht(x) + E(x) [ hf(x) df(x) - 1 + gamma ( ht(x) dt(x) - m(x) ) ], degree 3 per variable:
//                            four evaluations of the round polynomial (t = 0 .. 3) per round, six tables folded
//                            (E, df, dt, m, hf, ht).
// With df = beta + f, dt = beta + t, hf = 1 / df, ht = m / dt and E = lambda eq(tau, .), sum_x L(x) = 0 states the LogUp sum
// sum_x 1 / (beta + f(x)) = sum_y m(y) / (beta + t(y)) and, through the random point tau, the definitions of the two helper columns.
//
// Conventions of zk_fr.hip / zk_gate.hip: Fr in Montgomery form, 32-byte AoS elements, round i binds the TOP index bit, inputs are
// never written, all sums are exact modular sums.
//
// Shape (that of zk_wiring.hip): one HBM pass per round while the tables are long (k_lookup_pass), the four sums of a pass as 544-bit
// integers reduced once per sum and call (k_lookup_reduce), then every remaining round in one workgroup on tables held in LDS
// (k_lookup_local).
#include "zk_gate.cuh"

#include <algorithm>
#include <cstring>

namespace zk {

using LookupIn = FsIn<kLookupTabs>;  // sh is 0 throughout: six ordinary tables
using LookupOut = FsOut<kLookupTabs>;

// ---------------------------------------------------------------------------------------
// K15.  Row x is good when idx[x] < N -- checked BEFORE anything is read through it -- and f[x] and t[idx[x]] agree in all four
// 64-bit limbs; a good row adds one to the u32 counter of its entry, any other one to the count of bad rows (status).
// A counter holds up to 2^32 - 1 rows: N = 2^32 rows that ALL name one entry are out of its range (such tables, 128 GiB each,
// do not fit a device).
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kGateBlock) k_lookup_count(const void* __restrict__ f, const void* __restrict__ tab, const u32* __restrict__ idx, size_t N,
                                                            u32* __restrict__ cnt, unsigned long long* __restrict__ status) {
    for (size_t x = (size_t)blockIdx.x * kGateBlock + threadIdx.x; x < N; x += (size_t)gridDim.x * kGateBlock) {
        const size_t y = idx[x];
        bool ok = y < N;
        if (ok) ok = fp_eq(fr_load(f, x), fr_load(tab, y));
        if (ok)
            atomicAdd(&cnt[y], 1u);
        else
            atomicAdd(status, 1ull);
    }
}
// the counters as Montgomery Fr: integer x R^2, one multiplication per entry (as the slot numbers of k_perm3_terms)
__global__ void __launch_bounds__(kGateBlock) k_lookup_write(const u32* __restrict__ cnt, size_t N, void* __restrict__ m) {
    Fr r2;
#pragma unroll
    for (int i = 0; i < 8; i++) r2.l[i] = FrCfg::R2(i);
    for (size_t y = (size_t)blockIdx.x * kGateBlock + threadIdx.x; y < N; y += (size_t)gridDim.x * kGateBlock) {
        Fr c = fp_zero<FrCfg>();
        c.l[0] = cnt[y];
        fr_store(m, y, fr_mul(c, r2));
    }
}

int lookup_multiplicities(zk_ctx* ctx, const void* d_f, const void* d_t, const uint32_t* d_idx, size_t N, void* d_m) {
    if (N < 2 || (N & (N - 1)) || N > ((size_t)1 << 32)) return fail(ctx, ZK_ERR_INVALID, "zk_lookup_multiplicities: N = %zu is not a power of two in [2, 2^32]", N);
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    // arena 4 (the partials of the sumchecks): the status word, then the N counters
    char* s = (char*)scratch(ctx, 4, 16 + N * sizeof(u32));
    if (!s) return ZK_ERR_OOM;
    unsigned long long* h_bad = (unsigned long long*)pinned(ctx, sizeof(unsigned long long));
    if (!h_bad) return ZK_ERR_OOM;
    ZK_HIP(ctx, hipMemsetAsync(s, 0, 16 + N * sizeof(u32), ctx->stream));
    const unsigned blocks = (unsigned)std::min<size_t>((N + kGateBlock - 1) / kGateBlock, (size_t)ctx->cu_count * 8);
    hipLaunchKernelGGL(k_lookup_count, dim3(blocks), dim3(kGateBlock), 0, ctx->stream, d_f, d_t, (const u32*)d_idx, N, (u32*)(s + 16), (unsigned long long*)s);
    ZK_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_lookup_write, dim3(blocks), dim3(kGateBlock), 0, ctx->stream, (const u32*)(s + 16), N, d_m);
    ZK_HIP(ctx, hipGetLastError());
    ZK_HIP(ctx, hipMemcpyAsync(h_bad, s, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (*h_bad) return fail(ctx, ZK_ERR_INVALID, "zk_lookup_multiplicities: %llu of %zu rows are not in the table (index out of range or f[x] != t[idx[x]])", *h_bad, N);
    return ZK_OK;
}

// the second launch alone, for zk_lookup_find.hip, which counts on its own
int lookup_write_counts(zk_ctx* ctx, const uint32_t* d_cnt, size_t N, void* d_m) {
    const unsigned blocks = (unsigned)std::min<size_t>((N + kGateBlock - 1) / kGateBlock, (size_t)ctx->cu_count * 8);
    hipLaunchKernelGGL(k_lookup_write, dim3(blocks), dim3(kGateBlock), 0, ctx->stream, (const u32*)d_cnt, N, d_m);
    ZK_HIP(ctx, hipGetLastError());
    return ZK_OK;
}

// ---------------------------------------------------------------------------------------
// K16.  One round over tables of length 2 * half living in HBM.  partials: [t * nbw + 4 block + wave], 80-byte slots.
// The values at t = 1 .. 3 come from v(t) = v(t-1) + (hi - lo): per t four multiplications (three reduced ones inside the
// bracket, the product with E left as an integer for the lazily reduced sum), with the six folds 6 + 4 x 4 = 22 per index pair.
// The term hf - ht, which E does not multiply, is linear in the tables: its value at t is g0 + t gd with g0 = hf_lo - ht_lo and
// gd = (hf_hi - hf_lo) - (ht_hi - ht_lo).  A lane keeps the modular sums of g0 and gd over its index pairs (two Fr, canonical) and
// adds g0 + t gd to sum t ONCE, after its loop, as an integer times 2^256 (gate_wide_add_hi): the sums hold raw products of
// Montgomery forms a R b R and are divided by R = 2^256 once, so a Montgomery form g R has to enter as g R 2^256.
// Capacity of the sums as in k_gate_pass: a product is < r^2 < 0.83 * 2^510 and k_lookup_reduce adds ALL N/2 <= 2^34 products of a
// pass into one 544-bit integer, < 0.83 * 2^544; on top come one term < r 2^256 < 2^511 per LANE, at most 2^17 lanes of a grid:
// < 2^528.  Hence N <= 2^35 (kGateMaxLog) as for the siblings.  (One such term per index PAIR would not fit: 2^34 (r^2 + r 2^256)
// > 2^544.)
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kGateBlock) __attribute__((amdgpu_waves_per_eu(1, 2)))
k_lookup_pass(LookupIn in, LookupOut out, size_t half, GateChal ch, GateChal gamma, void* __restrict__ partials) {
    u32 w[kLookupEvals][17];
#pragma unroll
    for (int t = 0; t < kLookupEvals; t++)
#pragma unroll
        for (int i = 0; i < 17; i++) w[t][i] = 0;
    Fr g0 = fp_zero<FrCfg>(), gd = fp_zero<FrCfg>();
    for (size_t j = (size_t)blockIdx.x * kGateBlock + threadIdx.x; j < half; j += (size_t)gridDim.x * kGateBlock) {
        Fr v[kLookupTabs], d[kLookupTabs];
#pragma unroll
        for (int k = 0; k < kLookupTabs; k++) v[k] = fr_load(in.t[k], j), d[k] = fr_load(in.t[k], j + half);
#pragma unroll
        for (int k = 0; k < kLookupTabs; k++) {
            d[k] = fr_sub(d[k], v[k]);
            fr_store(out.t[k], j, fr_add(v[k], fr_mul(ch.r, d[k])));  // lo + r (hi - lo)   dsumcheck.rs:14-19
        }
        g0 = fr_add(g0, fr_sub(v[4], v[5]));
        gd = fr_add(gd, fr_sub(d[4], d[5]));
#pragma unroll
        for (int t = 0; t < kLookupEvals; t++) {
            fp_mac_wide(w[t], v[0], lookup_inner(gamma.r, v[1], v[2], v[3], v[4], v[5]));
            if (t + 1 < kLookupEvals) {
#pragma unroll
                for (int k = 0; k < kLookupTabs; k++) v[k] = fr_add(v[k], d[k]);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < kLookupEvals; t++) {  // hf - ht at t = g0 + t gd
        gate_wide_add_hi(w[t], g0);
        g0 = fr_add(g0, gd);
    }
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t nbw = (size_t)gridDim.x * (kGateBlock / 64);
#pragma unroll
    for (int t = 0; t < kLookupEvals; t++) {
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
__global__ void __launch_bounds__(kGateBlock) k_lookup_reduce(const void* __restrict__ partials, GateReducePlan plan, void* __restrict__ evals) {
    __shared__ uint4 lds[(kGateBlock / 64) * (kGateWideBytes / 16)];
    const unsigned t = blockIdx.x, p = blockIdx.y, nbw = plan.nbw[p];
    gate_reduce_block(partials, (size_t)plan.off[p] + (size_t)t * nbw, nbw, lds, evals, (size_t)p * kLookupEvals + t);
}

// ---------------------------------------------------------------------------------------
// Local stage: all remaining rounds of tables of E <= 512 elements in one workgroup, as k_wiring_local: the six tables sit in
// LDS (6 x 512 x 32 B = 96 KiB) and are folded in place (a lane reads elements j and j + h of each and writes j: no other lane
// touches either before the round's barrier).  Sums of a round: wave shuffle, one LDS slot per wave (two sets, by round parity),
// four lanes finish them.  Every sum is a reduced one here, so hf - ht is added to each point's product as it is.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kGateBlock) k_lookup_local(LookupIn in, unsigned E, int rounds, GateTail chal, GateChal gamma, void* __restrict__ evals,
                                                            void* __restrict__ last) {
    extern __shared__ uint4 llds[];
    uint4* red = llds + 2 * (size_t)kLookupTabs * E;  // [parity][wave][t] Fr
    const unsigned tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (unsigned i = tid; i < E; i += kGateBlock)
#pragma unroll
        for (int k = 0; k < kLookupTabs; k++) fr_store(llds, (size_t)k * E + i, fr_load(in.t[k], i));
    __syncthreads();
    unsigned L = E;
    for (int rd = 0; rd < rounds; rd++) {
        const unsigned h = L >> 1;
        const Fr r = fr_load(chal.c, rd);
        Fr acc[kLookupEvals];
#pragma unroll
        for (int t = 0; t < kLookupEvals; t++) acc[t] = fp_zero<FrCfg>();
        for (unsigned j = tid; j < h; j += kGateBlock) {
            Fr v[kLookupTabs], d[kLookupTabs];
#pragma unroll
            for (int k = 0; k < kLookupTabs; k++) {
                v[k] = fr_load(llds, (size_t)k * E + j);
                d[k] = fr_sub(fr_load(llds, (size_t)k * E + j + h), v[k]);
                fr_store(llds, (size_t)k * E + j, fr_add(v[k], fr_mul(r, d[k])));
            }
#pragma unroll
            for (int t = 0; t < kLookupEvals; t++) {
                const Fr p = fr_mul(v[0], lookup_inner(gamma.r, v[1], v[2], v[3], v[4], v[5]));
                acc[t] = fr_add(acc[t], fr_add(fr_sub(v[4], v[5]), p));
                if (t + 1 < kLookupEvals) {
#pragma unroll
                    for (int k = 0; k < kLookupTabs; k++) v[k] = fr_add(v[k], d[k]);
                }
            }
        }
        uint4* rs = red + 2 * (size_t)(rd & 1) * (kGateBlock / 64) * kLookupEvals;
#pragma unroll
        for (int t = 0; t < kLookupEvals; t++) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                Fr o;
#pragma unroll
                for (int i = 0; i < 8; i++) o.l[i] = __shfl_down(acc[t].l[i], off, 64);
                acc[t] = fr_add(acc[t], o);
            }
            if (lane == 0) fr_store(rs, (size_t)wave * kLookupEvals + t, acc[t]);
        }
        __syncthreads();
        if (tid < kLookupEvals) {
            Fr s = fr_load(rs, tid);
            for (int g = 1; g < kGateBlock / 64; g++) s = fr_add(s, fr_load(rs, (size_t)g * kLookupEvals + tid));
            fr_store(evals, (size_t)rd * kLookupEvals + tid, s);
        }
        L = h;
    }
    if (tid < kLookupTabs) fr_store(last, tid, fr_load(llds, (size_t)tid * E));
}

// ---------------------------------------------------------------------------------------
// host driver
// ---------------------------------------------------------------------------------------
int sumcheck_lookup(zk_ctx* ctx, const void* const* d_tabs, size_t len, const uint64_t* h_gamma, const uint64_t* h_chal, uint64_t* h_out_evals, uint64_t* h_last) {
    if (len < 2 || (len & (len - 1))) return fail(ctx, ZK_ERR_INVALID, "zk_sumcheck_lookup: len = %zu is not a power of two >= 2", len);
    size_t rounds = 0;
    while (((size_t)1 << rounds) < len) rounds++;
    if (rounds > (size_t)kGateMaxLog) return fail(ctx, ZK_ERR_INVALID, "zk_sumcheck_lookup: tables longer than 2^%d elements", kGateMaxLog);
    // hand-over point to the local stage (knob lookup_local_e: 1 = HBM passes down to the last element)
    size_t emax = (size_t)tuning().lookup_local_e;
    if (emax < 1 || emax > kGateLocalMax || (emax & (emax - 1))) return fail(ctx, ZK_ERR_INVALID, "lookup_local_e must be a power of two in [1, %u]", kGateLocalMax);
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    // plan: passes while the tables are longer than emax
    size_t npass = 0, part_slots = 0;
    GateReducePlan rp;
    std::memset(&rp, 0, sizeof(rp));
    size_t blocks_of[kGateMaxPasses];
    for (size_t m = len; m > emax; m >>= 1) {
        if (npass == (size_t)kGateMaxPasses) return fail(ctx, ZK_ERR_INVALID, "zk_sumcheck_lookup: table too long");
        const size_t half = m >> 1;
        const size_t blocks = std::min<size_t>((half + kGateBlock - 1) / kGateBlock, (size_t)ctx->cu_count * 2);
        blocks_of[npass] = blocks;
        rp.nbw[npass] = (unsigned)(blocks * (kGateBlock / 64));
        rp.off[npass] = (unsigned)part_slots;
        part_slots += (size_t)kLookupEvals * rp.nbw[npass];
        npass++;
    }
    const size_t fr = 32;
    const size_t res_bytes = (rounds * kLookupEvals + kLookupTabs) * fr;
    char* res = (char*)pinned(ctx, res_bytes);  // the kernels write the results straight into pinned host memory
    if (!res) return ZK_ERR_OOM;
    char* buf[2] = {nullptr, nullptr};
    char* part = nullptr;
    if (npass) {
        // the arenas of the gate sumcheck: ping-pong tables (six of len/2 and six of len/4 elements) and the 544-bit partials
        if (!(buf[0] = (char*)scratch(ctx, 0, kLookupTabs * (len / 2) * fr))) return ZK_ERR_OOM;
        if (npass > 1 && !(buf[1] = (char*)scratch(ctx, 1, kLookupTabs * (len / 4) * fr))) return ZK_ERR_OOM;
        if (!(part = (char*)scratch(ctx, 4, part_slots * kGateWideBytes))) return ZK_ERR_OOM;
    }
    GateChal gamma;
    std::memcpy(&gamma.r, h_gamma, 32);
    LookupIn cur;
    for (int k = 0; k < kLookupTabs; k++) cur.t[k] = d_tabs[k], cur.sh[k] = 0;
    size_t m = len;
    for (size_t p = 0; p < npass; p++) {
        const size_t half = m >> 1;
        LookupOut o;
        for (int k = 0; k < kLookupTabs; k++) o.t[k] = buf[p & 1] + (size_t)k * ((p & 1) ? len / 4 : len / 2) * fr;
        GateChal ch;
        std::memcpy(&ch.r, h_chal + 4 * p, 32);
        hipLaunchKernelGGL(k_lookup_pass, dim3((unsigned)blocks_of[p]), dim3(kGateBlock), 0, ctx->stream, cur, o, half, ch, gamma,
                           (void*)(part + (size_t)rp.off[p] * kGateWideBytes));
        ZK_HIP(ctx, hipGetLastError());
        for (int k = 0; k < kLookupTabs; k++) cur.t[k] = o.t[k];
        m = half;
    }
    if (npass) {
        hipLaunchKernelGGL(k_lookup_reduce, dim3(kLookupEvals, (unsigned)npass), dim3(kGateBlock), 0, ctx->stream, (const void*)part, rp, (void*)res);
        ZK_HIP(ctx, hipGetLastError());
    }
    {
        const int rl = (int)(rounds - npass);
        GateTail tl;
        std::memset(&tl, 0, sizeof(tl));
        std::memcpy(tl.c, h_chal + 4 * npass, (size_t)rl * 32);
        const size_t lds = (2 * (size_t)kLookupTabs * m + 2 * 2 * (kGateBlock / 64) * kLookupEvals) * sizeof(uint4);
        if (lds > 64 * 1024 && !ctx->lookup_lds_raised) {  // once per ctx (= per device)
            ZK_HIP(ctx, hipFuncSetAttribute((const void*)k_lookup_local, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            ctx->lookup_lds_raised = true;
        }
        hipLaunchKernelGGL(k_lookup_local, dim3(1), dim3(kGateBlock), lds, ctx->stream, cur, (unsigned)m, rl, tl, gamma,
                           (void*)(res + npass * kLookupEvals * fr), (void*)(res + rounds * kLookupEvals * fr));
        ZK_HIP(ctx, hipGetLastError());
    }
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(h_out_evals, res, rounds * kLookupEvals * fr);
    std::memcpy(h_last, res + rounds * kLookupEvals * fr, kLookupTabs * fr);
    return ZK_OK;
}

}  // namespace zk
