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
// Conventions of zk_wiring.hip: Fr in Montgomery form, 32-byte AoS elements, round i binds the TOP index bit, inputs are never
// written, all sums are exact modular sums.  The sumcheck is the preset-challenge engine of zk_fused.cuh over Perm3Kind (zk_gate.cuh);
// the four views of v are read in place out of the tree (element i of a table is the Fr at t + 32 (i << sh): sh = 1 reads every other
// element).  Per index pair and t eight multiplications (seven reduced ones inside the bracket, the product with eq left as an
// integer), with the eleven folds 11 + 6 x 8 = 59 per index pair.  Eleven tables of 512 elements would be 176 KiB, more than the CU's
// 160 KiB of LDS: the hand-over is at most kPerm3LocalMax = 256 elements (88 KiB).
//
// Registers of the pass: eleven (value, difference) pairs are 176 VGPRs and six 17-limb sums 102 more, so it is compiled for one wave
// per SIMD (the 264 .. 512 register bracket) and launched with one workgroup per CU.
#include "zk_fused.cuh"

namespace zk {

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
    return run_preset<Perm3Kind>(ctx, "zk_sumcheck_perm3", "N = ", bind_perm3(d_eq, d_tree, d_num, d_den, N, h_gamma), N, h_chal, h_out_evals, h_last);
}

}  // namespace zk
