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
// The sumcheck is the preset-challenge engine of zk_fused.cuh over LookupKind (zk_gate.cuh).  Per index pair and t four
// multiplications (three reduced ones inside the bracket, the product with E left as an integer), with the six folds 6 + 4 x 4 = 22
// per index pair.  hf - ht, which E does not multiply, is the Kind's free term: kind_free_wide (zk_gate.cuh) says how it enters the
// lazily reduced sums of a pass; the local stage (six tables of 512 elements: 96 KiB of LDS) adds it per point as a reduced value.
#include "zk_fused.cuh"

namespace zk {

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
// host driver
// ---------------------------------------------------------------------------------------
int sumcheck_lookup(zk_ctx* ctx, const void* const* d_tabs, size_t len, const uint64_t* h_gamma, const uint64_t* h_chal, uint64_t* h_out_evals, uint64_t* h_last) {
    return run_preset<LookupKind>(ctx, "zk_sumcheck_lookup", "len = ", bind_lookup(d_tabs, h_gamma), len, h_chal, h_out_evals, h_last);
}

}  // namespace zk
