// zk_srsio.hip -- a structured parameter set (SRS) that comes from a file: validated, expanded and checked on the device, so that a
// prover never holds the trapdoor (zk_g1_decompress_check_device, zk_srs_halve, zk_fr_hash_expand, zk_srs_check).
//
//   k_srsio_decompress  48 bytes -> one 96-byte affine record (reference form) and a status byte: the rule of g1c_decompress (g1c.cuh),
//                       the text zk_g1_decompress_check runs, in a grid-stride loop over device memory
//   k_srsio_subgroup    Scott's membership test (g1c_in_subgroup) on the records of status 0; counts the bad points and takes the
//                       minimum of their indices with atomics, so neither depends on the order of the threads
//   k_srsio_result      one lane: the status of that smallest index
//   k_srsio_halve       out[j] = level[j] + level[j + m] with the complete mixed addition (equal operands double, opposite ones give
//                       infinity, which is counted); the sums are normalised by xyzz_to_affine_batch (zk_srs.hip): Montgomery's trick
//                       per lane over a strided group, one inversion per 64 points
//   k_fr_hash_expand    one SHA-256 compression per lane (sha256.cuh): the 128-bit weights of the pairing check
// Two validation kernels, not one, for the reason given in zk_g1check.hip: the square root holds 3 field elements, the ladder 12.
// No kernel waits on another workgroup; every loop has a trip count fixed by the arguments.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "g1c.cuh"
#include "host_curve.hpp"
#include "sha256.cuh"
#include "zk_ctx.hpp"

namespace zk {

namespace srsio {
constexpr int kBlk = 64;          // the validation kernels: one wave per workgroup, as zk_g1check.hip
constexpr int kBlkWide = 256;     // the cheap kernels
constexpr size_t kMaxBlocks = 2048;  // 2 waves per SIMD on 256 CUs: beyond it the validation kernels stride
constexpr unsigned char kInfinity = ZK_G1_INFINITY_REFUSED;
}  // namespace srsio

static __global__ void __launch_bounds__(srsio::kBlk) k_srsio_decompress(size_t count, const void* __restrict__ in48, void* __restrict__ out96,
                                                                        unsigned char* __restrict__ status, unsigned flags) {
#pragma unroll 1
    for (size_t i = (size_t)blockIdx.x * srsio::kBlk + threadIdx.x; i < count; i += (size_t)gridDim.x * srsio::kBlk) {
        Fq30 x = f30_zero(), y = f30_zero();
        bool inf;
        unsigned char st = g1c_decompress(in48, i, x, y, inf);
        if (st == g1c::kOk && inf && (flags & 1u)) st = srsio::kInfinity;
        const bool point = st == g1c::kOk && !inf;
        f30_store(out96, i * 96, point ? f30_to_ref(x) : f30_zero());
        f30_store(out96, i * 96 + 48, point ? f30_to_ref(y) : f30_zero());
        status[i] = st;
    }
}

// res[0]: the number of points whose status is not 0, res[1]: the smallest of their indices (all ones: none)
static __global__ void __launch_bounds__(srsio::kBlk) k_srsio_subgroup(size_t count, const void* __restrict__ out96, unsigned char* __restrict__ status,
                                                                      unsigned long long* __restrict__ res) {
#pragma unroll 1
    for (size_t i = (size_t)blockIdx.x * srsio::kBlk + threadIdx.x; i < count; i += (size_t)gridDim.x * srsio::kBlk) {
        unsigned char st = status[i];
        if (st == g1c::kOk) {
            const Fq30 xr = f30_load(out96, i * 96), yr = f30_load(out96, i * 96 + 48);
            if (!(f30_all_zero(xr) && f30_all_zero(yr))) {  // (the neutral element is a member)
                Xyzz30 P;
                P.x = f30_from_ref(xr);
                P.y = f30_from_ref(yr);
                P.zz = f30_one();
                P.zzz = f30_one();
                if (!g1c_in_subgroup(P)) status[i] = st = g1c::kNotInG1;
            }
        }
        if (st != g1c::kOk) {
            atomicAdd(&res[0], 1ULL);
            atomicMin(&res[1], (unsigned long long)i);
        }
    }
}

static __global__ void k_srsio_result(const unsigned char* __restrict__ status, unsigned long long* __restrict__ res) {
    res[2] = res[0] ? status[res[1]] : 0;
}

// xyzz[j] = level[j] + level[j + m] (internal affine form in, blocked XYZZ out), j < m
static __global__ void __launch_bounds__(srsio::kBlkWide) k_srsio_halve(const void* __restrict__ level, size_t m, void* __restrict__ xyzz,
                                                                       unsigned long long* __restrict__ res) {
    const size_t j = (size_t)blockIdx.x * srsio::kBlkWide + threadIdx.x;
    if (j >= m) return;
    Xyzz30 acc;
    xyzz30_set_inf(acc);
    xyzz30_madd(acc, aff30_load(level, j), false);
    xyzz30_madd(acc, aff30_load(level, j + m), false);  // complete: the same point doubles, its opposite cancels
    xyzz30_store(xyzz, j, acc);
    if (xyzz30_is_inf(acc)) {
        atomicAdd(&res[0], 1ULL);
        atomicMin(&res[1], (unsigned long long)j);
    }
}

struct SrsioSeed {
    u32 w[8];  // the seed's 32 bytes as big-endian words
};
// out[j] = the first 16 bytes of SHA-256(seed || u32le(domain) || u64le(j)) read as a little-endian integer, in Montgomery form.  The
// message is 44 bytes: one block.
static __global__ void __launch_bounds__(srsio::kBlkWide) k_fr_hash_expand(SrsioSeed seed, u32 domain, size_t n, void* __restrict__ out) {
    const size_t j = (size_t)blockIdx.x * srsio::kBlkWide + threadIdx.x;
    if (j >= n) return;
    u32 m[16], h[8];
#pragma unroll
    for (int i = 0; i < 8; i++) m[i] = seed.w[i];
    m[8] = sha_bswap(domain);
    m[9] = sha_bswap((u32)j);
    m[10] = sha_bswap((u32)((u64)j >> 32));
    m[11] = 0x80000000u;
    m[12] = m[13] = m[14] = 0;
    m[15] = 44 * 8;
    sha256_init(h);
    sha256_compress(h, m);
    // the Montgomery form c 2^256 mod r by 256 modular doublings (c < 2^128 < r): plain carry chains, a fraction of the hash beside them
    Fr c;
#pragma unroll
    for (int i = 0; i < 8; i++) c.l[i] = i < 4 ? sha_bswap(h[i]) : 0u;
#pragma unroll 1
    for (int i = 0; i < 256; i++) c = fp_dbl<FrCfg>(c);
    fr_store(out, j, c);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
int xyzz_to_affine_batch(zk_ctx* ctx, const void* d_xyzz, size_t n, void* d_out96);  // zk_srs.hip
void srs_finish_endo(zk_ctx* ctx, zk_srs* s);                                        // zk_msm.hip

static inline size_t srsio_up256(size_t b) { return (b + 255) & ~(size_t)255; }

// the status bytes and the three result words live in scratch arena 11, the one zk_g1check.hip and the pairing stage in: every user
// synchronises the ctx stream before it returns
int g1_decompress_check_device(zk_ctx* ctx, size_t count, const void* d_in48, void* d_out96, uint32_t flags, uint64_t* h_result) {
    h_result[0] = 0, h_result[1] = ~(uint64_t)0, h_result[2] = 0;
    if (count == 0) return ZK_OK;
    if (((uintptr_t)d_in48 | (uintptr_t)d_out96) & 15) return fail(ctx, ZK_ERR_INVALID, "zk_g1_decompress_check_device: the buffers must be 16-byte aligned");
    if (flags & ~1u) return fail(ctx, ZK_ERR_INVALID, "zk_g1_decompress_check_device: unknown flag bits %#x", flags);
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t o_res = 0, o_st = 256, total = o_st + srsio_up256(count);
    char* d = static_cast<char*>(scratch(ctx, 11, total));
    if (!d) return ZK_ERR_OOM;
    unsigned long long* d_res = reinterpret_cast<unsigned long long*>(d + o_res);
    unsigned char* d_st = reinterpret_cast<unsigned char*>(d + o_st);
    const long knob = tuning().srsio_max_blocks;
    const size_t cap = knob > 0 ? (size_t)knob : srsio::kMaxBlocks;
    const dim3 grid((unsigned)std::min((count + srsio::kBlk - 1) / srsio::kBlk, cap)), blk(srsio::kBlk);
    ZK_HIP(ctx, hipMemsetAsync(d_res, 0, 8, ctx->stream));
    ZK_HIP(ctx, hipMemsetAsync(d_res + 1, 0xff, 8, ctx->stream));
    hipLaunchKernelGGL(k_srsio_decompress, grid, blk, 0, ctx->stream, count, d_in48, d_out96, d_st, flags);
    ZK_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_srsio_subgroup, grid, blk, 0, ctx->stream, count, (const void*)d_out96, d_st, d_res);
    ZK_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_srsio_result, dim3(1), dim3(1), 0, ctx->stream, (const unsigned char*)d_st, d_res);
    ZK_HIP(ctx, hipGetLastError());
    ZK_HIP(ctx, hipMemcpyAsync(h_result, d_res, 24, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ZK_OK;
}

int srs_halve(zk_ctx* ctx, const zk_srs* level, zk_srs** out) {
    if (level->g2) return fail(ctx, ZK_ERR_INVALID, "zk_srs_halve: G1 levels only");
    if (level->n < 2 || (level->n & 1)) return fail(ctx, ZK_ERR_INVALID, "zk_srs_halve: a level of %zu points has no halves", level->n);
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t m = level->n / 2;
    unsigned long long* d_res = static_cast<unsigned long long*>(scratch(ctx, 11, 256));
    if (!d_res) return ZK_ERR_OOM;
    void* d_x = nullptr;
    zk_srs* s = new zk_srs();
    s->n = m;
    s->owned = true;
    auto drop = [&] {
        if (d_x) hipFree(d_x);
        if (s->d_bases) hipFree(s->d_bases);
        delete s;
    };
    hipError_t e = device_alloc(ctx, &d_x, ((m + 63) & ~(size_t)63) * 192);
    if (e == hipSuccess) e = device_alloc(ctx, &s->d_bases, 2 * m * 96);  // P_j, then phi(P_j)
    if (e == hipSuccess) e = hipMemsetAsync(d_res, 0, 8, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_res + 1, 0xff, 8, ctx->stream);
    if (e != hipSuccess) {
        drop();
        return hip_fail(ctx, e, "zk_srs_halve: allocation");
    }
    hipLaunchKernelGGL(k_srsio_halve, dim3((unsigned)((m + srsio::kBlkWide - 1) / srsio::kBlkWide)), dim3(srsio::kBlkWide), 0, ctx->stream,
                       (const void*)level->d_bases, m, d_x, d_res);
    e = hipGetLastError();
    int rc = e == hipSuccess ? xyzz_to_affine_batch(ctx, d_x, m, s->d_bases) : hip_fail(ctx, e, "k_srsio_halve");  // (synchronises)
    uint64_t res[2] = {0, 0};
    if (!rc && (e = hipMemcpy(res, d_res, 16, hipMemcpyDeviceToHost)) != hipSuccess) rc = hip_fail(ctx, e, "zk_srs_halve");
    if (!rc && res[0])
        rc = fail(ctx, ZK_ERR_INVALID, "zk_srs_halve: %llu of %zu sums are the point at infinity; the first is sum %llu", (unsigned long long)res[0], m,
                  (unsigned long long)res[1]);
    if (!rc) {
        srs_finish_endo(ctx, s);
        if ((e = hipGetLastError()) == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) rc = hip_fail(ctx, e, "zk_srs_halve: endomorphism images");
    }
    if (rc) {
        drop();
        return rc;
    }
    hipFree(d_x);
    *out = s;
    return ZK_OK;
}

int fr_hash_expand(zk_ctx* ctx, const uint8_t* h_seed32, uint32_t domain, size_t n, void* d_out) {
    if (n == 0) return ZK_OK;
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    SrsioSeed seed;
    for (int i = 0; i < 8; i++)
        seed.w[i] = (u32)h_seed32[4 * i] << 24 | (u32)h_seed32[4 * i + 1] << 16 | (u32)h_seed32[4 * i + 2] << 8 | (u32)h_seed32[4 * i + 3];
    hipLaunchKernelGGL(k_fr_hash_expand, dim3((unsigned)((n + srsio::kBlkWide - 1) / srsio::kBlkWide)), dim3(srsio::kBlkWide), 0, ctx->stream, seed,
                       (u32)domain, n, d_out);
    ZK_HIP(ctx, hipGetLastError());
    return ZK_OK;
}

// Relation (B) of include/zkhip.h for every level under ONE vector of weights: 2n MSMs in one batch, one pairing call of n groups.
int srs_check(zk_ctx* ctx, const zk_srs* const* levels, size_t n, const void* h_powers_g2, size_t g2_stride, const uint8_t* h_seed32, uint8_t* h_ok) {
    namespace H = zkhost;
    if (n < 1 || n > 30) return fail(ctx, ZK_ERR_INVALID, "zk_srs_check: %zu variables (1 .. 30)", n);
    if (g2_stride < 192) return fail(ctx, ZK_ERR_INVALID, "zk_srs_check: g2_stride %zu < 192", g2_stride);
    for (size_t k = 0; k <= n; k++) {
        if (!levels[k] || levels[k]->g2) return fail(ctx, ZK_ERR_INVALID, "zk_srs_check: level %zu is not a G1 level", k);
        if (levels[k]->n != (size_t)1 << k) return fail(ctx, ZK_ERR_INVALID, "zk_srs_check: level %zu holds %zu points, not 2^%zu", k, levels[k]->n, k);
    }
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t half = (size_t)1 << (n - 1);
    void* d_rho = nullptr;
    ZK_HIP(ctx, device_alloc(ctx, &d_rho, half * 32));
    int rc = fr_hash_expand(ctx, h_seed32, ZK_SRS_CHECK_DOMAIN, half, d_rho);
    // item 2k: A_k = sum_j rho_j L_{k+1}[j + 2^k]; item 2k + 1: B_k = sum_j rho_j L_k[j]
    std::vector<MsmItem> items(2 * n);
    for (size_t k = 0; k < n; k++) {
        items[2 * k] = MsmItem{levels[k + 1], (size_t)1 << k, d_rho, (size_t)1 << k};
        items[2 * k + 1] = MsmItem{levels[k], 0, d_rho, (size_t)1 << k};
    }
    std::vector<uint64_t> sums(2 * n * 18);
    if (!rc) rc = msm_g1_batch(ctx, items.data(), 2 * n, sums.data());
    hipFree(d_rho);
    if (rc) return rc;
    // group k: e(A_k, g2) e(-B_k, powers_g2[n - k]) == 1.  A sum or a key at infinity would drop its factor: such a level fails here.
    std::vector<uint64_t> g1(2 * n * 12), g2(2 * n * 24);
    std::vector<size_t> start(n + 1);
    std::vector<uint8_t> degenerate(n, 0);
    auto key = [&](size_t i, uint64_t* out) {
        const char* p = static_cast<const char*>(h_powers_g2) + i * g2_stride;
        std::memcpy(out, p, 192);
        bool zero = true;
        for (int w = 0; w < 24; w++) zero = zero && out[w] == 0;
        return !(zero || (g2_stride > 192 && p[192]));
    };
    for (size_t k = 0; k < n; k++) {
        start[k] = 2 * k;
        for (int t = 0; t < 2; t++) {
            const uint64_t* s = &sums[(2 * k + t) * 18];
            bool inf = true;
            for (int w = 12; w < 18; w++) inf = inf && s[w] == 0;
            if (inf) degenerate[k] = 1;
            std::memcpy(&g1[(2 * k + t) * 12], s, 96);
            if (t == 1) {  // -B_k
                H::Fq y;
                H::get_fe(y, s + 6);
                H::put_fe(H::neg(y), &g1[(2 * k + 1) * 12 + 6]);
            }
            if (!key(t == 0 ? 0 : n - k, &g2[(2 * k + t) * 24])) degenerate[k] = 1;
        }
    }
    start[n] = 2 * n;
    for (size_t k = 0; k < n; k++)
        if (degenerate[k])  // (keeps the pairing's own point checks away from a record that is no point)
            for (int t = 0; t < 2; t++) {
                std::memset(&g1[(2 * k + t) * 12], 0, 96);
                std::memset(&g2[(2 * k + t) * 24], 0, 192);
            }
    rc = pairing_product_check(ctx, n, start.data(), g1.data(), g2.data(), 192, h_ok);
    if (rc) return rc;
    for (size_t k = 0; k < n; k++)
        if (degenerate[k]) h_ok[k] = 0;
    return ZK_OK;
}

}  // namespace zk
