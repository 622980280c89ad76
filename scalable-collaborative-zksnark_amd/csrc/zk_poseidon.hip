// zk_poseidon.hip -- the Poseidon permutation over BLS12-381 Fr at width t = 3 (capacity 1, rate 2, S-box x^5), its 2-to-1 hash and a
// Merkle tree of that hash, on the device.
//   K28  permute   one lane per state of three Fr: the whole permutation in registers
//   K29  hash2     one lane per pair: out = permute(0, left, right)[0]
//   K30  level     ONE level of a Merkle tree with more than `poseidon_tail_nodes` nodes: one lane per node, node = hash2(left child, right child)
//   K31  tail      every level of at most `poseidon_tail_nodes` nodes: ONE workgroup of kPosBlock lanes walks them, a fence and a barrier
//                  between levels (the scheme of K23 in zk_witness.hip)
// and a tree that stays on the device (the second half of this file; leaf indices come from the host, validated there and staged here):
//   K32  paths         a gather of sibling paths, one lane per (path, level)
//   K33  roots         one lane per path: the leaf hashed up through its siblings
//   K34  write         the leaf writes of an update
//   K35  update level  ONE level of an update with more than `poseidon_tail_nodes` distinct parents: one lane per written leaf, the first lane
//                      of each parent's run of the ascending indices hashes
//   K36  update tail   every remaining level: ONE workgroup on the compacted list of distinct parents, a fence and a barrier between levels
//
// The rule (the same in include/zkhip.h, zkhip/poseidon.py, host/zkhost/poseidon.hpp and tests/poseidon_model.py).  With rf full and rp partial
// rounds, one counter k indexes all rf + rp rounds: rounds 0 .. rf/2 - 1 are full, the next rp are partial, the last rf/2 are full.
//   full round k:     s_i += rc[3k + i] for i = 0, 1, 2;  every s_i <- s_i^5;  s <- M s
//   partial round k:  s_i += rc[3k + i] for i = 0, 1, 2;  only  s_0 <- s_0^5;  s <- M s
// (M s)_i = M[i][0] s_0 + M[i][1] s_1 + M[i][2] s_2, the products added left to right.  Everything is Montgomery Fr, fully reduced after
// every operation, so the bits of a result do not depend on how the arithmetic is grouped: a sparse form of the partial rounds would give
// the same bits.  This file uses the plain matrix product: 3 multiplications per S-box, 9 per linear layer, (9 + 9) rf + (3 + 9) rp of
// them per permutation -- 828 for the instance zkhip-poseidon-v1 (rf = 8, rp = 57).
//
// The constants are DATA: a zk_poseidon_params object owns one device block [M: 9 Fr, row-major | rc: 3 (rf + rp) Fr] and every kernel
// reads it through a const pointer at wave-uniform addresses.  Nothing about an instance is compiled in but t = 3 and the exponent 5.
// The v1 constants are the project's own (SHA-256 derived round constants, a Cauchy matrix) and are not claimed to equal any other
// library's; the Poseidon paper's further checks of the matrix (invariant-subspace trails) have not been done on it.  That is the reason
// the constants are a parameter: an instance that has been through such an analysis is a different pair of arrays, not a different build.
//
// Order.  zk_poseidon_merkle copies the leaves and enqueues its launches on the ctx stream; no host read lies between them.  A node reads
// only nodes of the level below: an earlier launch, or an earlier level of the same workgroup, whose stores are complete and visible at
// workgroup scope after the fence and the barrier that close the level.  No workgroup ever waits on another; there are no atomics.
//
// Bounds.  A lane touches state i < n only; a Merkle lane of a level of cnt nodes reads tree[in + 2i], tree[in + 2i + 1] and writes
// tree[out + i] for i < cnt with in + 2 cnt = out and out + cnt <= 2n - 1: all inside the 2n - 1 elements the caller provides.
//
// Registers (hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage): DESIGN.md, section 4.
#include "poseidon.cuh"
#include "zk_ctx.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

namespace zk {

static constexpr int kPosBlock = 256;
static constexpr unsigned kPosMaxBlocks = 1u << 16;  // the grid of the lane-per-item kernels (a grid-stride loop walks longer inputs)

// pos_pow5, pos_permute, pos_hash2 and the params object: poseidon.cuh (shared with zk_jubjub.hip)

// ---------------------------------------------------------------------------------------
// K28.  in and out may be the same array: a lane reads its own state before it writes it
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kPosBlock) k_pos_permute(const void* __restrict__ consts, u32 half, u32 rp, const void* in, void* out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * kPosBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kPosBlock) {
        Fr s0 = fr_load(in, 3 * i), s1 = fr_load(in, 3 * i + 1), s2 = fr_load(in, 3 * i + 2);
        pos_permute(consts, half, rp, s0, s1, s2);
        fr_store(out, 3 * i, s0);
        fr_store(out, 3 * i + 1, s1);
        fr_store(out, 3 * i + 2, s2);
    }
}
// ---------------------------------------------------------------------------------------
// K29.  out may be left or right: a lane reads its own pair before it writes
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kPosBlock) k_pos_hash2(const void* __restrict__ consts, u32 half, u32 rp, const void* left, const void* right, void* out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * kPosBlock + threadIdx.x; i < n; i += (size_t)gridDim.x * kPosBlock)
        fr_store(out, i, pos_hash2(consts, half, rp, fr_load(left, i), fr_load(right, i)));
}
// ---------------------------------------------------------------------------------------
// K30.  one level: tree[out + i] = hash2(tree[in + 2i], tree[in + 2i + 1]), i < cnt
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kPosBlock) k_pos_level(const void* __restrict__ consts, u32 half, u32 rp, void* tree, size_t in, size_t out, size_t cnt) {
    for (size_t i = (size_t)blockIdx.x * kPosBlock + threadIdx.x; i < cnt; i += (size_t)gridDim.x * kPosBlock)
        fr_store(tree, out + i, pos_hash2(consts, half, rp, fr_load(tree, in + 2 * i), fr_load(tree, in + 2 * i + 1)));
}
// ---------------------------------------------------------------------------------------
// K31.  ONE workgroup: the levels of cnt, cnt / 2, .., 1 nodes above the `2 cnt` nodes at tree[in ..)
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kPosBlock) k_pos_tail(const void* __restrict__ consts, u32 half, u32 rp, void* tree, size_t in, size_t cnt) {
    for (; cnt >= 1; cnt >>= 1) {
        const size_t out = in + 2 * cnt;
        for (size_t i = threadIdx.x; i < cnt; i += kPosBlock)
            fr_store(tree, out + i, pos_hash2(consts, half, rp, fr_load(tree, in + 2 * i), fr_load(tree, in + 2 * i + 1)));
        __threadfence_block();
        __syncthreads();
        in = out;
    }
}

static unsigned pos_blocks(size_t n) { return (unsigned)std::min<size_t>((n + kPosBlock - 1) / kPosBlock, kPosMaxBlocks); }

// a < r, on four little-endian u64
static bool pos_canonical(const uint64_t* a) {
    static const uint64_t r[4] = {0xffffffff00000001ull, 0x53bda402fffe5bfeull, 0x3339d80809a1d805ull, 0x73eda753299d7d48ull};
    for (int i = 3; i >= 0; i--)
        if (a[i] != r[i]) return a[i] < r[i];
    return false;
}

int poseidon_params_create(zk_ctx* ctx, int rf, int rp, const uint64_t* h_rc, const uint64_t* h_mds, zk_poseidon_params** out) {
    *out = nullptr;
    if (rf <= 0 || (rf & 1) || rp < 0 || rf + rp > 256)
        return fail(ctx, ZK_ERR_INVALID, "poseidon: rf = %d full and rp = %d partial rounds (rf even and > 0, rp >= 0, rf + rp <= 256 are needed)", rf, rp);
    const size_t n_rc = 3 * (size_t)(rf + rp);
    for (size_t i = 0; i < 9; i++)
        if (!pos_canonical(h_mds + 4 * i)) return fail(ctx, ZK_ERR_INVALID, "poseidon: matrix entry %zu is not below r", i);
    for (size_t i = 0; i < n_rc; i++)
        if (!pos_canonical(h_rc + 4 * i)) return fail(ctx, ZK_ERR_INVALID, "poseidon: round constant %zu is not below r", i);
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    zk_poseidon_params* p = new zk_poseidon_params;
    p->ctx = ctx;
    p->half = (uint32_t)rf / 2;
    p->rp = (uint32_t)rp;
    hipError_t e = device_alloc(ctx, &p->d_consts, 32 * (9 + n_rc));
    if (e == hipSuccess) e = hipMemcpy(p->d_consts, h_mds, 32 * 9, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy((char*)p->d_consts + 32 * 9, h_rc, 32 * n_rc, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (p->d_consts) hipFree(p->d_consts);
        delete p;
        return hip_fail(ctx, e, "poseidon params");
    }
    *out = p;
    return ZK_OK;
}
void poseidon_params_free(zk_poseidon_params* p) {
    if (!p) return;
    if (p->d_consts) {
        hipSetDevice(p->ctx->device);
        hipStreamSynchronize(p->ctx->stream);
        hipFree(p->d_consts);
    }
    delete p;
}

int poseidon_permute(zk_ctx* ctx, const zk_poseidon_params* p, const void* d_in, void* d_out, size_t n) {
    if (p->ctx != ctx) return fail(ctx, ZK_ERR_INVALID, "poseidon: the params belong to another ctx");
    if (n == 0) return ZK_OK;
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_pos_permute, dim3(pos_blocks(n)), dim3(kPosBlock), 0, ctx->stream, p->d_consts, p->half, p->rp, d_in, d_out, n);
    ZK_HIP(ctx, hipGetLastError());
    return ZK_OK;
}
int poseidon_hash2(zk_ctx* ctx, const zk_poseidon_params* p, const void* d_left, const void* d_right, void* d_out, size_t n) {
    if (p->ctx != ctx) return fail(ctx, ZK_ERR_INVALID, "poseidon: the params belong to another ctx");
    if (n == 0) return ZK_OK;
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_pos_hash2, dim3(pos_blocks(n)), dim3(kPosBlock), 0, ctx->stream, p->d_consts, p->half, p->rp, d_left, d_right, d_out, n);
    ZK_HIP(ctx, hipGetLastError());
    return ZK_OK;
}
int poseidon_merkle(zk_ctx* ctx, const zk_poseidon_params* p, const void* d_leaves, size_t n, void* d_tree) {
    if (p->ctx != ctx) return fail(ctx, ZK_ERR_INVALID, "poseidon: the params belong to another ctx");
    if (n == 0 || (n & (n - 1)) || n > ((size_t)1 << 40)) return fail(ctx, ZK_ERR_INVALID, "poseidon: a Merkle tree of %zu leaves (a power of two is needed)", n);
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    if (d_leaves != d_tree) ZK_HIP(ctx, hipMemcpyAsync(d_tree, d_leaves, 32 * n, hipMemcpyDeviceToDevice, ctx->stream));
    const long tail = tuning().poseidon_tail_nodes;
    size_t in = 0;
    for (size_t cnt = n / 2; cnt >= 1; in += 2 * cnt, cnt >>= 1) {
        if (tail < 1 || cnt > (size_t)tail) {
            hipLaunchKernelGGL(k_pos_level, dim3(pos_blocks(cnt)), dim3(kPosBlock), 0, ctx->stream, p->d_consts, p->half, p->rp, d_tree, in, in + 2 * cnt, cnt);
        } else {
            hipLaunchKernelGGL(k_pos_tail, dim3(1), dim3(kPosBlock), 0, ctx->stream, p->d_consts, p->half, p->rp, d_tree, in, cnt);
            break;
        }
    }
    ZK_HIP(ctx, hipGetLastError());
    return ZK_OK;
}

// =======================================================================================
// The tree kept on the device: paths, roots of paths, a batch of leaf writes (include/zkhip.h)
// =======================================================================================
// level j of a tree of n leaves (two_n = 2n) starts at 2n - (2n >> j): 0, n, n + n / 2, ..
__device__ __forceinline__ size_t pos_level_lo(size_t two_n, unsigned j) { return two_n - (two_n >> j); }

// ---------------------------------------------------------------------------------------
// K32.  a gather: sib[k * d + j] = tree[lo_j + ((idx[k] >> j) ^ 1)], one lane per (path, level).  idx[k] < n (checked on the host), so
// (idx[k] >> j) ^ 1 < n >> j (even for j < d): the read stays inside level j
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kPosBlock) k_pos_paths(const void* __restrict__ tree, size_t two_n, unsigned d, const uint64_t* __restrict__ idx, size_t count, void* __restrict__ sib) {
    const size_t items = count * d;
    for (size_t t = (size_t)blockIdx.x * kPosBlock + threadIdx.x; t < items; t += (size_t)gridDim.x * kPosBlock) {
        const size_t k = t / d;
        const unsigned j = (unsigned)(t - k * d);
        fr_store(sib, t, fr_load(tree, pos_level_lo(two_n, j) + ((idx[k] >> j) ^ 1)));
    }
}
// ---------------------------------------------------------------------------------------
// K33.  one lane per path: the leaf hashed up through `depth` siblings; bit j of the index set: the running node is the RIGHT child.  The
// two operands are selected limb by limb, so the permutation is one straight piece of code whatever the bits of a wave's lanes
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kPosBlock) k_pos_roots(const void* __restrict__ consts, u32 half, u32 rp, const void* leaves, const uint64_t* __restrict__ idx,
                                                         const void* __restrict__ sib, unsigned depth, size_t count, void* roots) {
    for (size_t k = (size_t)blockIdx.x * kPosBlock + threadIdx.x; k < count; k += (size_t)gridDim.x * kPosBlock) {
        const uint64_t i = idx[k];
        Fr cur = fr_load(leaves, k);
#pragma unroll 1
        for (unsigned j = 0; j < depth; j++) {
            const Fr s = fr_load(sib, k * depth + j);
            const bool right = (i >> j) & 1;
            Fr l, r;
#pragma unroll
            for (int t = 0; t < FrCfg::N; t++) l.l[t] = right ? s.l[t] : cur.l[t], r.l[t] = right ? cur.l[t] : s.l[t];
            cur = pos_hash2(consts, half, rp, l, r);
        }
        fr_store(roots, k, cur);
    }
}
// ---------------------------------------------------------------------------------------
// K34.  the leaf writes of an update: tree[idx[k]] = values[k]; the indices are distinct (strictly ascending, checked on the host)
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kPosBlock) k_pos_write(void* __restrict__ tree, const uint64_t* __restrict__ idx, const void* __restrict__ values, size_t count) {
    for (size_t k = (size_t)blockIdx.x * kPosBlock + threadIdx.x; k < count; k += (size_t)gridDim.x * kPosBlock) fr_store(tree, idx[k], fr_load(values, k));
}
// ---------------------------------------------------------------------------------------
// K35.  ONE level of an update, one lane per written leaf.  The parent of leaf idx[k] on level j + 1 is p = idx[k] >> (j + 1); among the
// lanes of one parent (a run of the ascending indices) the FIRST hashes: lane k leads when k = 0 or idx[k - 1] >> (j + 1) differs from p.
// Both children are level j nodes, complete since the launch before.  p < n >> (j + 1): the write stays inside level j + 1
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kPosBlock) k_pos_update_level(const void* __restrict__ consts, u32 half, u32 rp, void* tree, size_t two_n, unsigned j,
                                                                const uint64_t* __restrict__ idx, size_t count) {
    const size_t in = pos_level_lo(two_n, j), out = pos_level_lo(two_n, j + 1);
    for (size_t k = (size_t)blockIdx.x * kPosBlock + threadIdx.x; k < count; k += (size_t)gridDim.x * kPosBlock) {
        const uint64_t p = idx[k] >> (j + 1);
        if (k == 0 || (idx[k - 1] >> (j + 1)) != p) fr_store(tree, out + p, pos_hash2(consts, half, rp, fr_load(tree, in + 2 * p), fr_load(tree, in + 2 * p + 1)));
    }
}
// ---------------------------------------------------------------------------------------
// K36.  ONE workgroup: levels j0 .. d - 1 of an update.  par[0 .. m): the distinct parents of level j0, ascending (node numbers on level
// j0 + 1, each < n >> (j0 + 1)); on level j0 + s entry i stands for the node par[i] >> s and leads when i = 0 or par[i - 1] >> s differs --
// the rule of K35 on the compacted list.  A level reads what the level before wrote: a fence and a barrier close each level
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kPosBlock) k_pos_update_tail(const void* __restrict__ consts, u32 half, u32 rp, void* tree, size_t two_n, unsigned j0, unsigned d,
                                                               const uint64_t* __restrict__ par, size_t m) {
    for (unsigned j = j0; j < d; j++) {
        const size_t in = pos_level_lo(two_n, j), out = pos_level_lo(two_n, j + 1);
        const unsigned s = j - j0;
        for (size_t i = threadIdx.x; i < m; i += kPosBlock) {
            const uint64_t p = par[i] >> s;
            if (i == 0 || (par[i - 1] >> s) != p) fr_store(tree, out + p, pos_hash2(consts, half, rp, fr_load(tree, in + 2 * p), fr_load(tree, in + 2 * p + 1)));
        }
        __threadfence_block();
        __syncthreads();
    }
}

static constexpr int kPosIndexSlot = 10;  // the scratch arena of host-staged tables (zk_fr.hip uses it the same way)

// h_a[0 .. na) then h_b[0 .. nb) -> one device array in scratch, through the pinned staging area.  The stream is waited for first: both areas
// may still feed earlier work.  The copy itself is enqueued
static int pos_stage_u64(zk_ctx* ctx, const uint64_t* h_a, size_t na, const uint64_t* h_b, size_t nb, const uint64_t** d_out) {
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    uint64_t* d = (uint64_t*)scratch(ctx, kPosIndexSlot, 8 * (na + nb));
    uint64_t* h = (uint64_t*)pinned(ctx, 8 * (na + nb));
    if (!d || !h) return ZK_ERR_OOM;
    std::memcpy(h, h_a, 8 * na);
    if (nb) std::memcpy(h + na, h_b, 8 * nb);
    ZK_HIP(ctx, hipMemcpyAsync(d, h, 8 * (na + nb), hipMemcpyHostToDevice, ctx->stream));
    *d_out = d;
    return ZK_OK;
}
static bool pos_tree_size(size_t n) { return n != 0 && !(n & (n - 1)) && n <= ((size_t)1 << 40); }
static unsigned pos_log2(size_t n) {
    unsigned d = 0;
    while (((size_t)1 << d) < n) d++;
    return d;
}
// "K of COUNT indices <what>; the first is position P" when an index is >= limit
static int pos_check_below(zk_ctx* ctx, const char* fn, const uint64_t* h_index, size_t count, uint64_t limit, const char* what) {
    size_t bad = 0, first = 0;
    for (size_t k = count; k-- > 0;)
        if (h_index[k] >= limit) bad++, first = k;
    if (bad) return fail(ctx, ZK_ERR_INVALID, "%s: %zu of %zu indices %s; the first is position %zu", fn, bad, count, what, first);
    return ZK_OK;
}

int poseidon_merkle_paths(zk_ctx* ctx, const void* d_tree, size_t n, const uint64_t* h_index, size_t count, void* d_siblings) {
    static const char* fn = "zk_poseidon_merkle_paths";
    if (!pos_tree_size(n)) return fail(ctx, ZK_ERR_INVALID, "%s: a Merkle tree of %zu leaves (a power of two is needed)", fn, n);
    if (count > ZK_POSEIDON_MERKLE_MAX_COUNT) return fail(ctx, ZK_ERR_INVALID, "%s: %zu paths in one call (at most %zu)", fn, count, (size_t)ZK_POSEIDON_MERKLE_MAX_COUNT);
    if (count == 0) return ZK_OK;
    char what[64];
    snprintf(what, sizeof what, "are not below n = %zu", n);
    if (int rc = pos_check_below(ctx, fn, h_index, count, n, what)) return rc;
    const unsigned d = pos_log2(n);
    if (d == 0) return ZK_OK;
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    const uint64_t* d_idx = nullptr;
    if (int rc = pos_stage_u64(ctx, h_index, count, nullptr, 0, &d_idx)) return rc;
    hipLaunchKernelGGL(k_pos_paths, dim3(pos_blocks(count * d)), dim3(kPosBlock), 0, ctx->stream, d_tree, 2 * n, d, d_idx, count, d_siblings);
    ZK_HIP(ctx, hipGetLastError());
    return ZK_OK;
}

int poseidon_merkle_roots(zk_ctx* ctx, const zk_poseidon_params* p, const void* d_leaves, const uint64_t* h_index, const void* d_siblings, size_t depth, size_t count, void* d_roots) {
    static const char* fn = "zk_poseidon_merkle_roots";
    if (p->ctx != ctx) return fail(ctx, ZK_ERR_INVALID, "poseidon: the params belong to another ctx");
    if (depth > 40) return fail(ctx, ZK_ERR_INVALID, "%s: paths of depth %zu (at most 40)", fn, depth);
    if (count > ZK_POSEIDON_MERKLE_MAX_COUNT) return fail(ctx, ZK_ERR_INVALID, "%s: %zu paths in one call (at most %zu)", fn, count, (size_t)ZK_POSEIDON_MERKLE_MAX_COUNT);
    if (count == 0) return ZK_OK;
    char what[64];
    snprintf(what, sizeof what, "have bits at or above depth %zu", depth);
    if (int rc = pos_check_below(ctx, fn, h_index, count, (uint64_t)1 << depth, what)) return rc;
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    if (depth == 0) {
        if (d_roots != d_leaves) ZK_HIP(ctx, hipMemcpyAsync(d_roots, d_leaves, 32 * count, hipMemcpyDeviceToDevice, ctx->stream));
        return ZK_OK;
    }
    const uint64_t* d_idx = nullptr;
    if (int rc = pos_stage_u64(ctx, h_index, count, nullptr, 0, &d_idx)) return rc;
    hipLaunchKernelGGL(k_pos_roots, dim3(pos_blocks(count)), dim3(kPosBlock), 0, ctx->stream, p->d_consts, p->half, p->rp, d_leaves, d_idx, d_siblings, (unsigned)depth, count, d_roots);
    ZK_HIP(ctx, hipGetLastError());
    return ZK_OK;
}

int poseidon_merkle_update(zk_ctx* ctx, const zk_poseidon_params* p, void* d_tree, size_t n, const uint64_t* h_index, const void* d_values, size_t count) {
    static const char* fn = "zk_poseidon_merkle_update";
    if (p->ctx != ctx) return fail(ctx, ZK_ERR_INVALID, "poseidon: the params belong to another ctx");
    if (!pos_tree_size(n)) return fail(ctx, ZK_ERR_INVALID, "%s: a Merkle tree of %zu leaves (a power of two is needed)", fn, n);
    if (count > ZK_POSEIDON_MERKLE_MAX_COUNT) return fail(ctx, ZK_ERR_INVALID, "%s: %zu writes in one call (at most %zu)", fn, count, (size_t)ZK_POSEIDON_MERKLE_MAX_COUNT);
    if (count == 0) return ZK_OK;
    char what[64];
    snprintf(what, sizeof what, "are not below n = %zu", n);
    if (int rc = pos_check_below(ctx, fn, h_index, count, n, what)) return rc;
    // order, and per bit b the number of neighbours whose highest differing bit is b: lane k leads on level j exactly when that bit is above j
    size_t bad = 0, first = 0, high[64] = {0};
    for (size_t k = count; k-- > 1;) {
        if (h_index[k] <= h_index[k - 1]) bad++, first = k;
        else high[63 - __builtin_clzll(h_index[k] ^ h_index[k - 1])]++;
    }
    if (bad) return fail(ctx, ZK_ERR_INVALID, "%s: %zu of %zu indices are not above the one before them (strictly ascending indices are needed); the first is position %zu", fn, bad, count, first);
    const unsigned d = pos_log2(n);
    const long tail = tuning().poseidon_tail_nodes;
    // j0: the first level whose distinct parents (1 + the neighbours that differ above bit j) fit the single workgroup; d: none
    unsigned j0 = d;
    if (tail >= 1) {
        size_t above[65] = {0};  // above[b]: neighbours whose highest differing bit is >= b
        for (int b = 63; b >= 0; b--) above[b] = above[b + 1] + high[b];
        for (unsigned j = 0; j < d && j0 == d; j++)
            if (1 + above[j + 1] <= (size_t)tail) j0 = j;
    }
    std::vector<uint64_t> par;
    if (j0 < d)
        for (size_t k = 0; k < count; k++) {
            const uint64_t q = h_index[k] >> (j0 + 1);
            if (par.empty() || par.back() != q) par.push_back(q);
        }
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    const uint64_t* d_idx = nullptr;
    if (int rc = pos_stage_u64(ctx, h_index, count, par.data(), par.size(), &d_idx)) return rc;
    hipLaunchKernelGGL(k_pos_write, dim3(pos_blocks(count)), dim3(kPosBlock), 0, ctx->stream, d_tree, d_idx, d_values, count);
    for (unsigned j = 0; j < j0; j++)
        hipLaunchKernelGGL(k_pos_update_level, dim3(pos_blocks(count)), dim3(kPosBlock), 0, ctx->stream, p->d_consts, p->half, p->rp, d_tree, 2 * n, j, d_idx, count);
    if (j0 < d) hipLaunchKernelGGL(k_pos_update_tail, dim3(1), dim3(kPosBlock), 0, ctx->stream, p->d_consts, p->half, p->rp, d_tree, 2 * n, j0, d, d_idx + count, par.size());
    ZK_HIP(ctx, hipGetLastError());
    return ZK_OK;
}

}  // namespace zk
