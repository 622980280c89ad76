// zk_wiring.hip -- the wiring identity of HyperPlonk (the ProductCheck of its PermCheck) as ONE sumcheck; the reference simulates it
// with six independent product sumchecks on six unrelated polynomials (hyperplonk/src/hyperplonk.rs:94-141):
//   K11  wiring sumcheck     F(x) = eq(x) [ v(1,x) - v(x,0) v(x,1) + gamma ( den(x) h(x) - num(x) ) ], degree 3 per variable:
//                            four evaluations of the round polynomial (t = 0 .. 3) per round, seven tables folded
//                            (eq, v1x, vx0, vx1, h, num, den).
// v is the product tree of h = num / den (zk_product_tree: tree[0..N) = h, tree[N + j] = tree[2j] tree[2j+1], tree[2N-1] = 0); with
// index bit 0 the TOP bit, v(0,x) = tree[x], v(1,x) = tree[N + x], v(x,0) = tree[2x], v(x,1) = tree[2x + 1].
//
// Conventions of zk_fr.hip / zk_gate.hip: Fr in Montgomery form, 32-byte AoS elements, round i binds the TOP index bit, inputs are
// never written, all sums are exact modular sums.
//
// Shape (that of zk_gate.hip): one HBM pass per round while the tables are long (k_wiring_pass), the four sums of a pass as 544-bit
// integers reduced once per sum and call (k_wiring_reduce), then every remaining round in one workgroup on tables held in LDS
// (k_wiring_local).  The FIRST pass reads the four views straight out of the tree -- h and v1x are its halves, vx0 | vx1 one
// 64-byte pair per index -- so nobody makes deinterleaved copies; later passes read the folded ping-pong tables.
#include "zk_gate.cuh"

#include <algorithm>
#include <cstring>

namespace zk {

static constexpr int kWireTabs = 7;   // eq, v1x, vx0, vx1, h, num, den
static constexpr int kWireEvals = 4;  // t = 0 .. 3

// Table k, element i, is the Fr at t[k] + 32 (i << sh[k]): sh = 1 reads every other element of the tree (vx0 from the tree's
// base, vx1 from one element further), sh = 0 an ordinary table.
struct WireIn {
    const void* t[kWireTabs];
    unsigned sh[kWireTabs];
};
struct WireOut {
    void* t[kWireTabs];
};

// ---------------------------------------------------------------------------------------
// One round over tables of length 2 * half living in HBM.  partials: [t * nbw + 4 block + wave], 80-byte slots.
// TREE (the first pass of a call): in.t[1] is the tree; table 4 (h) is its lower half, table 1 (v1x) its upper half, and the
// pair (vx0, vx1) of index i is the 64 bytes at element 2i.  Otherwise seven ordinary tables.
// The values at t = 1 .. 3 come from v(t) = v(t-1) + (hi - lo): per t four multiplications (three reduced ones inside the
// bracket, the product with eq left as an integer for the lazily reduced sum), with the seven folds 7 + 4 x 4 = 23 per index pair.
// Capacity of the sums as in k_gate_pass: a product is < r^2 < 2^510, a 544-bit sum holds 2^34 of them and k_wiring_reduce adds
// ALL N/2 products of a pass into one, hence N <= 2^35 (kGateMaxLog; the tree of such an N would be 2 TiB).
// ---------------------------------------------------------------------------------------
template <bool TREE>
__global__ void __launch_bounds__(kGateBlock) __attribute__((amdgpu_waves_per_eu(1, 2)))
k_wiring_pass(WireIn in, WireOut out, size_t half, GateChal ch, GateChal gamma, void* __restrict__ partials) {
    u32 w[kWireEvals][17];
#pragma unroll
    for (int t = 0; t < kWireEvals; t++)
#pragma unroll
        for (int i = 0; i < 17; i++) w[t][i] = 0;
    for (size_t j = (size_t)blockIdx.x * kGateBlock + threadIdx.x; j < half; j += (size_t)gridDim.x * kGateBlock) {
        Fr v[kWireTabs], d[kWireTabs];
        if (TREE) {
            const void* tree = in.t[1];
            const size_t N = 2 * half;
            v[0] = fr_load(in.t[0], j), d[0] = fr_load(in.t[0], j + half);
            v[1] = fr_load(tree, N + j), d[1] = fr_load(tree, N + j + half);
            v[2] = fr_load(tree, 2 * j), v[3] = fr_load(tree, 2 * j + 1);  // one 64-byte pair
            d[2] = fr_load(tree, 2 * (j + half)), d[3] = fr_load(tree, 2 * (j + half) + 1);
            v[4] = fr_load(tree, j), d[4] = fr_load(tree, j + half);
            v[5] = fr_load(in.t[5], j), d[5] = fr_load(in.t[5], j + half);
            v[6] = fr_load(in.t[6], j), d[6] = fr_load(in.t[6], j + half);
        } else {
#pragma unroll
            for (int k = 0; k < kWireTabs; k++) v[k] = fr_load(in.t[k], j), d[k] = fr_load(in.t[k], j + half);
        }
#pragma unroll
        for (int k = 0; k < kWireTabs; k++) {
            d[k] = fr_sub(d[k], v[k]);
            fr_store(out.t[k], j, fr_add(v[k], fr_mul(ch.r, d[k])));  // lo + r (hi - lo)   dsumcheck.rs:14-19
        }
#pragma unroll
        for (int t = 0; t < kWireEvals; t++) {
            fp_mac_wide(w[t], v[0], wiring_inner(gamma.r, v[1], v[2], v[3], v[4], v[5], v[6]));
            if (t + 1 < kWireEvals) {
#pragma unroll
                for (int k = 0; k < kWireTabs; k++) v[k] = fr_add(v[k], d[k]);
            }
        }
    }
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t nbw = (size_t)gridDim.x * (kGateBlock / 64);
#pragma unroll
    for (int t = 0; t < kWireEvals; t++) {
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
__global__ void __launch_bounds__(kGateBlock) k_wiring_reduce(const void* __restrict__ partials, GateReducePlan plan, void* __restrict__ evals) {
    __shared__ uint4 lds[(kGateBlock / 64) * (kGateWideBytes / 16)];
    const unsigned t = blockIdx.x, p = blockIdx.y, nbw = plan.nbw[p];
    gate_reduce_block(partials, (size_t)plan.off[p] + (size_t)t * nbw, nbw, lds, evals, (size_t)p * kWireEvals + t);
}

// ---------------------------------------------------------------------------------------
// Local stage: all remaining rounds of tables of E <= 512 elements in one workgroup, as k_gate_local: the seven tables sit in
// LDS and are folded in place (a lane reads elements j and j + h of each and writes j: no other lane touches either before the
// round's barrier).  Sums of a round: wave shuffle, one LDS slot per wave (two sets, by round parity), four lanes finish them.
// The load honours in.sh, so a call whose N is at most the hand-over length reads the tree's views here.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kGateBlock) k_wiring_local(WireIn in, unsigned E, int rounds, GateTail chal, GateChal gamma, void* __restrict__ evals,
                                                            void* __restrict__ last) {
    extern __shared__ uint4 wlds[];
    uint4* red = wlds + 2 * (size_t)kWireTabs * E;  // [parity][wave][t] Fr
    const unsigned tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (unsigned i = tid; i < E; i += kGateBlock)
#pragma unroll
        for (int k = 0; k < kWireTabs; k++) fr_store(wlds, (size_t)k * E + i, fr_load(in.t[k], (size_t)i << in.sh[k]));
    __syncthreads();
    unsigned L = E;
    for (int rd = 0; rd < rounds; rd++) {
        const unsigned h = L >> 1;
        const Fr r = fr_load(chal.c, rd);
        Fr acc[kWireEvals];
#pragma unroll
        for (int t = 0; t < kWireEvals; t++) acc[t] = fp_zero<FrCfg>();
        for (unsigned j = tid; j < h; j += kGateBlock) {
            Fr v[kWireTabs], d[kWireTabs];
#pragma unroll
            for (int k = 0; k < kWireTabs; k++) {
                v[k] = fr_load(wlds, (size_t)k * E + j);
                d[k] = fr_sub(fr_load(wlds, (size_t)k * E + j + h), v[k]);
                fr_store(wlds, (size_t)k * E + j, fr_add(v[k], fr_mul(r, d[k])));
            }
#pragma unroll
            for (int t = 0; t < kWireEvals; t++) {
                acc[t] = fr_add(acc[t], fr_mul(v[0], wiring_inner(gamma.r, v[1], v[2], v[3], v[4], v[5], v[6])));
                if (t + 1 < kWireEvals) {
#pragma unroll
                    for (int k = 0; k < kWireTabs; k++) v[k] = fr_add(v[k], d[k]);
                }
            }
        }
        uint4* rs = red + 2 * (size_t)(rd & 1) * (kGateBlock / 64) * kWireEvals;
#pragma unroll
        for (int t = 0; t < kWireEvals; t++) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                Fr o;
#pragma unroll
                for (int i = 0; i < 8; i++) o.l[i] = __shfl_down(acc[t].l[i], off, 64);
                acc[t] = fr_add(acc[t], o);
            }
            if (lane == 0) fr_store(rs, (size_t)wave * kWireEvals + t, acc[t]);
        }
        __syncthreads();
        if (tid < kWireEvals) {
            Fr s = fr_load(rs, tid);
            for (int g = 1; g < kGateBlock / 64; g++) s = fr_add(s, fr_load(rs, (size_t)g * kWireEvals + tid));
            fr_store(evals, (size_t)rd * kWireEvals + tid, s);
        }
        L = h;
    }
    if (tid < kWireTabs) fr_store(last, tid, fr_load(wlds, (size_t)tid * E));
}

// ---------------------------------------------------------------------------------------
// host driver
// ---------------------------------------------------------------------------------------
int sumcheck_wiring(zk_ctx* ctx, const void* d_eq, const void* d_tree, const void* d_num, const void* d_den, size_t N, const uint64_t* h_gamma,
                    const uint64_t* h_chal, uint64_t* h_out_evals, uint64_t* h_last) {
    if (N < 2 || (N & (N - 1))) return fail(ctx, ZK_ERR_INVALID, "zk_sumcheck_wiring: N = %zu is not a power of two >= 2", N);
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    size_t rounds = 0;
    while (((size_t)1 << rounds) < N) rounds++;
    if (rounds > (size_t)kGateMaxLog) return fail(ctx, ZK_ERR_INVALID, "zk_sumcheck_wiring: tables longer than 2^%d elements", kGateMaxLog);
    // hand-over point to the local stage (knob wiring_local_e: 1 = HBM passes down to the last element)
    size_t emax = (size_t)tuning().wiring_local_e;
    if (emax < 1 || emax > kGateLocalMax || (emax & (emax - 1))) return fail(ctx, ZK_ERR_INVALID, "wiring_local_e must be a power of two in [1, %u]", kGateLocalMax);
    // plan: passes while the tables are longer than emax
    size_t npass = 0, part_slots = 0;
    GateReducePlan rp;
    std::memset(&rp, 0, sizeof(rp));
    size_t blocks_of[kGateMaxPasses];
    const size_t per_cu = tuning().wiring_pass_wg > 0 ? (size_t)tuning().wiring_pass_wg : 2;
    for (size_t m = N; m > emax; m >>= 1) {
        if (npass == (size_t)kGateMaxPasses) return fail(ctx, ZK_ERR_INVALID, "zk_sumcheck_wiring: table too long");
        const size_t half = m >> 1;
        const size_t blocks = std::min<size_t>((half + kGateBlock - 1) / kGateBlock, (size_t)ctx->cu_count * per_cu);
        blocks_of[npass] = blocks;
        rp.nbw[npass] = (unsigned)(blocks * (kGateBlock / 64));
        rp.off[npass] = (unsigned)part_slots;
        part_slots += (size_t)kWireEvals * rp.nbw[npass];
        npass++;
    }
    const size_t fr = 32;
    const size_t res_bytes = (rounds * kWireEvals + kWireTabs) * fr;
    char* res = (char*)pinned(ctx, res_bytes);  // the kernels write the results straight into pinned host memory
    if (!res) return ZK_ERR_OOM;
    char* buf[2] = {nullptr, nullptr};
    char* part = nullptr;
    if (npass) {
        // the arenas of the gate sumcheck: ping-pong tables (seven of N/2 and seven of N/4 elements) and the 544-bit partials
        if (!(buf[0] = (char*)scratch(ctx, 0, kWireTabs * (N / 2) * fr))) return ZK_ERR_OOM;
        if (npass > 1 && !(buf[1] = (char*)scratch(ctx, 1, kWireTabs * (N / 4) * fr))) return ZK_ERR_OOM;
        if (!(part = (char*)scratch(ctx, 4, part_slots * kGateWideBytes))) return ZK_ERR_OOM;
    }
    GateChal gamma;
    std::memcpy(&gamma.r, h_gamma, 32);
    // the views of the tree (k_wiring_pass<true> only looks at t[0], t[1], t[5], t[6])
    const char* tree = (const char*)d_tree;
    WireIn cur = {{d_eq, tree + N * fr, tree, tree + fr, tree, d_num, d_den}, {0, 0, 1, 1, 0, 0, 0}};
    size_t m = N;
    for (size_t p = 0; p < npass; p++) {
        const size_t half = m >> 1;
        WireOut o;
        for (int k = 0; k < kWireTabs; k++) o.t[k] = buf[p & 1] + (size_t)k * ((p & 1) ? N / 4 : N / 2) * fr;
        GateChal ch;
        std::memcpy(&ch.r, h_chal + 4 * p, 32);
        void* pp = (void*)(part + (size_t)rp.off[p] * kGateWideBytes);
        if (p == 0) {
            WireIn first = cur;
            first.t[1] = tree;
            hipLaunchKernelGGL(k_wiring_pass<true>, dim3((unsigned)blocks_of[p]), dim3(kGateBlock), 0, ctx->stream, first, o, half, ch, gamma, pp);
        } else {
            hipLaunchKernelGGL(k_wiring_pass<false>, dim3((unsigned)blocks_of[p]), dim3(kGateBlock), 0, ctx->stream, cur, o, half, ch, gamma, pp);
        }
        ZK_HIP(ctx, hipGetLastError());
        for (int k = 0; k < kWireTabs; k++) cur.t[k] = o.t[k], cur.sh[k] = 0;
        m = half;
    }
    if (npass) {
        hipLaunchKernelGGL(k_wiring_reduce, dim3(kWireEvals, (unsigned)npass), dim3(kGateBlock), 0, ctx->stream, (const void*)part, rp, (void*)res);
        ZK_HIP(ctx, hipGetLastError());
    }
    {
        const int rl = (int)(rounds - npass);
        GateTail tl;
        std::memset(&tl, 0, sizeof(tl));
        std::memcpy(tl.c, h_chal + 4 * npass, (size_t)rl * 32);
        const size_t lds = (2 * (size_t)kWireTabs * m + 2 * 2 * (kGateBlock / 64) * kWireEvals) * sizeof(uint4);
        if (lds > 64 * 1024 && !ctx->wiring_lds_raised) {  // once per ctx (= per device)
            ZK_HIP(ctx, hipFuncSetAttribute((const void*)k_wiring_local, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            ctx->wiring_lds_raised = true;
        }
        hipLaunchKernelGGL(k_wiring_local, dim3(1), dim3(kGateBlock), lds, ctx->stream, cur, (unsigned)m, rl, tl, gamma,
                           (void*)(res + npass * kWireEvals * fr), (void*)(res + rounds * kWireEvals * fr));
        ZK_HIP(ctx, hipGetLastError());
    }
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(h_out_evals, res, rounds * kWireEvals * fr);
    std::memcpy(h_last, res + rounds * kWireEvals * fr, kWireTabs * fr);
    return ZK_OK;
}

}  // namespace zk
