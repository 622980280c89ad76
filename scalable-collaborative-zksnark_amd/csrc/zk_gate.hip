// zk_gate.hip -- the gate identity of HyperPlonk as ONE sumcheck (the virtual circuit the reference simulates with six
// independent product sumchecks, hyperplonk/src/hyperplonk.rs:66-93, dhyperplonk.rs:218-260):
//   K9   eq table            out[x] = prod_i (x_i ? tau_i : 1 - tau_i), built by doubling,
//   K10  gate sumcheck       G(x) = eq(x) [ q1(x) (a(x) + b(x)) + q2(x) a(x) b(x) - c(x) + in(x) ], degree 4 per variable:
//                            five evaluations of the round polynomial (t = 0 .. 4) per round, seven tables folded.
//
// Conventions of zk_fr.hip: Fr in Montgomery form, 32-byte AoS elements, round i binds the TOP index bit (lo = tab[..m/2],
// hi = tab[m/2..]), inputs are never written, all sums are exact modular sums (any association order gives the same bits).
//
// The sumcheck is the preset-challenge engine of zk_fused.cuh over GateKind (zk_gate.cuh): one HBM pass per round while the tables
// are long, then every remaining round in one workgroup on tables held in LDS.  Per index pair and t four multiplications (three
// reduced ones inside the bracket, the product with eq left as an integer for the lazily reduced sum).
#include "zk_fused.cuh"

namespace zk {

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
    return run_preset<GateKind>(ctx, "zk_sumcheck_gate", "table length ", bind_gate(d_tabs), len, h_chal, h_out_evals, h_last);
}

}  // namespace zk
