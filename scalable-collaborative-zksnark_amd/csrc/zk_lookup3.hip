// zk_lookup3.hip -- the lookup argument as a path of a Plonk circuit: the rows x with qk(x) = 1 claim that their wire triple
// (a, b, c)(x) is an entry (t0, t1, t2)(y) of a table of N triples; a row with qk(x) = 0 claims nothing.
//   K17  multiplicities      m[y] = #{x : qk(x) = 1, idx[x] = y}, checked against the wires and the table on the way
//   K18  derived tables      df = beta + a + zeta b + zeta^2 c,  dt = beta + t0 + zeta t1 + zeta^2 t2 in one pass
//   K19  lookup sumcheck     L(x) = hf(x) - ht(x) + E(x) [ hf(x) df(x) - qk(x) + gamma ( ht(x) dt(x) - m(x) ) ], degree 3 per variable:
//                            four evaluations of the round polynomial (t = 0 .. 3) per round, SEVEN tables folded
//                            (E, df, dt, m, hf, ht, qk: the order of zk_lookup.hip, the selector last).
// With hf = qk / df, ht = m / dt and E = lambda eq(tau, .), sum_x L(x) = 0 states sum_x qk(x) / df(x) = sum_y m(y) / dt(y) and the
// definitions of the two helper columns.  With qk = 1 everywhere K19 computes what K16 (zk_lookup.hip) computes, bit for bit.
//
// Conventions of zk_lookup.hip: Fr in Montgomery form, 32-byte AoS elements, round i binds the TOP index bit, inputs are never
// written, all sums are exact modular sums.  K19 is the preset-challenge engine of zk_fused.cuh over LookupSelKind (zk_gate.cuh).  Per
// index pair and t four multiplications (three reduced ones inside the bracket, the product with E left as an integer), with the seven
// folds 7 + 4 x 4 = 23 per index pair.  qk is subtracted as a reduced value INSIDE the bracket, before the wide multiplication with E:
// the only term that E does not multiply stays hf - ht, the Kind's free term as in zk_lookup.hip (kind_free_wide, zk_gate.cuh; with one
// workgroup per CU a grid has fewer lanes than the six-table pass, so its capacity argument holds).  Seven tables of 512 elements are
// 112 KiB of the CU's 160 KiB of LDS.  LookupSelKind says why the pass is compiled for one wave per SIMD.
#include "zk_fused.cuh"

namespace zk {

struct Lookup3Cols {
    const void* w[3];
    const void* t[3];
};

// ---------------------------------------------------------------------------------------
// K17.  A row with qk = 0 is skipped: its idx is never read through.  A row with qk = 1 (the Montgomery form) is good when
// idx[x] < N -- checked BEFORE anything is read through it -- and (a, b, c)(x) and (t0, t1, t2)(idx[x]) agree in all twelve 64-bit
// limbs; a good row adds one to the u32 counter of its entry.  Any other row -- a qk that is neither 0 nor 1 among them -- adds one
// to the count of bad rows (status).  Counters as in k_lookup_count: up to 2^32 - 1 rows per entry.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kGateBlock) k_lookup3_count(Lookup3Cols c, const void* __restrict__ qk, const u32* __restrict__ idx, size_t N, u32* __restrict__ cnt,
                                                             unsigned long long* __restrict__ status) {
    for (size_t x = (size_t)blockIdx.x * kGateBlock + threadIdx.x; x < N; x += (size_t)gridDim.x * kGateBlock) {
        const Fr q = fr_load(qk, x);
        if (fp_eq(q, fp_zero<FrCfg>())) continue;
        if (!fp_eq(q, fp_one<FrCfg>())) {  // neither 0 nor 1: a bad row, and nothing of it is read
            atomicAdd(status, 1ull);
            continue;
        }
        const size_t y = idx[x];
        bool ok = y < N;
        if (ok) {
#pragma unroll
            for (int j = 0; j < 3; j++) ok = ok && fp_eq(fr_load(c.w[j], x), fr_load(c.t[j], y));
        }
        if (ok)
            atomicAdd(&cnt[y], 1u);
        else
            atomicAdd(status, 1ull);
    }
}
// the counters as Montgomery Fr: integer x R^2, one multiplication per entry (k_lookup_write of zk_lookup.hip)
__global__ void __launch_bounds__(kGateBlock) k_lookup3_write(const u32* __restrict__ cnt, size_t N, void* __restrict__ m) {
    Fr r2;
#pragma unroll
    for (int i = 0; i < 8; i++) r2.l[i] = FrCfg::R2(i);
    for (size_t y = (size_t)blockIdx.x * kGateBlock + threadIdx.x; y < N; y += (size_t)gridDim.x * kGateBlock) {
        Fr c = fp_zero<FrCfg>();
        c.l[0] = cnt[y];
        fr_store(m, y, fr_mul(c, r2));
    }
}

int lookup3_multiplicities(zk_ctx* ctx, const void* const* d_w, const void* const* d_t, const void* d_qk, const uint32_t* d_idx, size_t N, void* d_m) {
    if (N < 2 || (N & (N - 1)) || N > ((size_t)1 << 32)) return fail(ctx, ZK_ERR_INVALID, "zk_lookup3_multiplicities: N = %zu is not a power of two in [2, 2^32]", N);
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    // arena 4 (the partials of the sumchecks): the status word, then the N counters
    char* s = (char*)scratch(ctx, 4, 16 + N * sizeof(u32));
    if (!s) return ZK_ERR_OOM;
    unsigned long long* h_bad = (unsigned long long*)pinned(ctx, sizeof(unsigned long long));
    if (!h_bad) return ZK_ERR_OOM;
    Lookup3Cols c;
    for (int j = 0; j < 3; j++) c.w[j] = d_w[j], c.t[j] = d_t[j];
    ZK_HIP(ctx, hipMemsetAsync(s, 0, 16 + N * sizeof(u32), ctx->stream));
    const unsigned blocks = (unsigned)std::min<size_t>((N + kGateBlock - 1) / kGateBlock, (size_t)ctx->cu_count * 8);
    hipLaunchKernelGGL(k_lookup3_count, dim3(blocks), dim3(kGateBlock), 0, ctx->stream, c, d_qk, (const u32*)d_idx, N, (u32*)(s + 16), (unsigned long long*)s);
    ZK_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_lookup3_write, dim3(blocks), dim3(kGateBlock), 0, ctx->stream, (const u32*)(s + 16), N, d_m);
    ZK_HIP(ctx, hipGetLastError());
    ZK_HIP(ctx, hipMemcpyAsync(h_bad, s, sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (*h_bad)
        return fail(ctx, ZK_ERR_INVALID,
                    "zk_lookup3_multiplicities: %llu of %zu rows are not in the table (qk neither 0 nor 1, index out of range or (a, b, c)[x] != (t0, t1, t2)[idx[x]])",
                    *h_bad, N);
    return ZK_OK;
}

// ---------------------------------------------------------------------------------------
// K18.  df and dt in one pass: per row three wires and three table columns read, two elements written; Horner in zeta, two
// multiplications per output.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kGateBlock) k_lookup3_terms(Lookup3Cols c, size_t N, GateChal zeta, GateChal beta, void* __restrict__ df, void* __restrict__ dt) {
    for (size_t x = (size_t)blockIdx.x * kGateBlock + threadIdx.x; x < N; x += (size_t)gridDim.x * kGateBlock) {
        const Fr f = fr_add(fr_load(c.w[0], x), fr_mul(zeta.r, fr_add(fr_load(c.w[1], x), fr_mul(zeta.r, fr_load(c.w[2], x)))));
        const Fr t = fr_add(fr_load(c.t[0], x), fr_mul(zeta.r, fr_add(fr_load(c.t[1], x), fr_mul(zeta.r, fr_load(c.t[2], x)))));
        fr_store(df, x, fr_add(beta.r, f));
        fr_store(dt, x, fr_add(beta.r, t));
    }
}

int lookup3_terms(zk_ctx* ctx, const void* const* d_w, const void* const* d_t, size_t N, const uint64_t* h_zeta, const uint64_t* h_beta, void* d_df, void* d_dt) {
    if (N < 2 || (N & (N - 1))) return fail(ctx, ZK_ERR_INVALID, "zk_lookup3_terms: N = %zu is not a power of two >= 2", N);
    if (N > ((size_t)1 << kGateMaxLog)) return fail(ctx, ZK_ERR_INVALID, "zk_lookup3_terms: tables longer than 2^%d elements", kGateMaxLog);
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    Lookup3Cols c;
    for (int j = 0; j < 3; j++) c.w[j] = d_w[j], c.t[j] = d_t[j];
    GateChal ze, be;
    std::memcpy(&ze.r, h_zeta, 32);
    std::memcpy(&be.r, h_beta, 32);
    const size_t blocks = std::min<size_t>((N + kGateBlock - 1) / kGateBlock, (size_t)ctx->cu_count * 8);
    hipLaunchKernelGGL(k_lookup3_terms, dim3((unsigned)blocks), dim3(kGateBlock), 0, ctx->stream, c, N, ze, be, d_df, d_dt);
    ZK_HIP(ctx, hipGetLastError());
    return ZK_OK;
}

// ---------------------------------------------------------------------------------------
// host driver
// ---------------------------------------------------------------------------------------
int sumcheck_lookup_sel(zk_ctx* ctx, const void* const* d_tabs, size_t len, const uint64_t* h_gamma, const uint64_t* h_chal, uint64_t* h_out_evals, uint64_t* h_last) {
    return run_preset<LookupSelKind>(ctx, "zk_sumcheck_lookup_sel", "len = ", bind_lookup_sel(d_tabs, h_gamma), len, h_chal, h_out_evals, h_last);
}

}  // namespace zk
