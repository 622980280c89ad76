// zk_batchopen.hip -- the device side of HyperPlonk's batch opening: K evaluation claims f_{j_k}(z_k) = v_k on J tables of one
// size become ONE degree-2 sumcheck of sum_j E_j f_j,  E_j = sum_{k : j_k = j} a_k eq(z_k, .),  and one opening of sum_j e_j f_j:
//   K12  eq accumulate       acc[x] += weight * eq(point, x): the doubling scheme of K9 seeded with the weight, last level added in,
//   K13  Fr linear comb.     out[x] = sum_j c_j tab_j[x], count <= 16, flat form (wide multiply-accumulates, one reduction),
//   K14  multi sumcheck      the rounds of sum_x sum_j E_j(x) f_j(x): the triple (t0, t1, t2) of zk_sumcheck_product summed over j.
//
// Conventions of zk_fr.hip / zk_gate.hip: Fr in Montgomery form, 32-byte AoS elements, round i binds the TOP index bit, inputs are
// never written, all sums are exact modular sums.
//
// Shape of K14 (the product passes of zk_fr.hip, one round per pass): a lane walks the pairs j one after the other; for each it
// folds E_j and f_j into ping-pong scratch and adds the integer products into two 544-bit sums t0 and t2 SHARED by all j -- one
// shuffle reduction and one Montgomery reduction per sum and round, not one per pair; t1 is summed in the first round only and
// derived on the host afterwards (derive_t1).  Then every remaining round in one workgroup on tables held in LDS (k_multi_local).
#include "zk_gate.cuh"

#include <algorithm>
#include <cstring>

namespace zk {

struct LincombIn {
    const void* t[kMultiMax];
    Fr c[kMultiMax];
};

// ---------------------------------------------------------------------------------------
// K12: the last level of the doubling, added into acc: lo = part[j] (the weighted table of the variables 1 .. n-1),
// acc[j + size] += lo tau_0,  acc[j] += lo - lo tau_0.  tau_0 in {0, 1} gives hi = 0 / hi = lo exactly.
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kGateBlock) k_eq_acc_last(const void* __restrict__ part, void* __restrict__ acc, size_t size, GateChal tau) {
    for (size_t j = (size_t)blockIdx.x * kGateBlock + threadIdx.x; j < size; j += (size_t)gridDim.x * kGateBlock) {
        const Fr lo = fr_load(part, j), hi = fr_mul(lo, tau.r);
        fr_store(acc, j + size, fr_add(fr_load(acc, j + size), hi));
        fr_store(acc, j, fr_add(fr_load(acc, j), fr_sub(lo, hi)));
    }
}
__global__ void k_eq_acc_one(void* __restrict__ acc, GateChal w) {
    if (threadIdx.x == 0 && blockIdx.x == 0) fr_store(acc, 0, fr_add(fr_load(acc, 0), w.r));
}

int eq_table_acc(zk_ctx* ctx, const uint64_t* h_point, size_t n, const uint64_t* h_weight, void* d_acc) {
    if (n > 40) return fail(ctx, ZK_ERR_INVALID, "zk_eq_table_acc: %zu variables", n);
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    GateChal t;
    if (n == 0) {
        std::memcpy(&t.r, h_weight, 32);
        hipLaunchKernelGGL(k_eq_acc_one, dim3(1), dim3(64), 0, ctx->stream, d_acc, t);
        ZK_HIP(ctx, hipGetLastError());
        return ZK_OK;
    }
    // one level of scratch: weight * eq((z_1 .. z_{n-1}), .), half the table
    const size_t size = (size_t)1 << (n - 1);
    void* part = scratch(ctx, 1, size * 32);
    if (!part) return ZK_ERR_OOM;
    const int rc = eq_table_seeded(ctx, h_point + 4, n - 1, h_weight, part);
    if (rc != ZK_OK) return rc;
    std::memcpy(&t.r, h_point, 32);
    const size_t blocks = std::min<size_t>((size + kGateBlock - 1) / kGateBlock, (size_t)ctx->cu_count * 16);
    hipLaunchKernelGGL(k_eq_acc_last, dim3((unsigned)blocks), dim3(kGateBlock), 0, ctx->stream, (const void*)part, d_acc, size, t);
    ZK_HIP(ctx, hipGetLastError());
    return ZK_OK;
}

// ---------------------------------------------------------------------------------------
// K13 in the flat form of k_fold_flat: the coefficients are wave-uniform kernel arguments (SGPR operands of fp_mac_wide_s), a
// lane adds the count integer products of one output into ONE 544-bit sum and reduces once.  32 (count + 1) len bytes of traffic.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void lincomb_csub(u32 (&v)[9], int s) {  // v -= r << s if v >= r << s
    u32 d[9], bw = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const u32 lo = i < 8 ? FrCfg::P(i) : 0u, below = i > 0 ? FrCfg::P(i - 1) : 0u;
        const u32 c = s == 0 ? lo : ((lo << s) | (below >> (32 - s)));
        d[i] = subb(v[i], c, bw);
    }
#pragma unroll
    for (int i = 0; i < 9; i++) v[i] = bw ? v[i] : d[i];
}
__global__ void __launch_bounds__(kGateBlock) k_fr_lincomb(LincombIn in, int count, size_t len, void* out) {  // out may be one of in.t: a lane reads element x of every table before it stores x
    for (size_t x = (size_t)blockIdx.x * kGateBlock + threadIdx.x; x < len; x += (size_t)gridDim.x * kGateBlock) {
        u32 acc[17];
#pragma unroll
        for (int i = 0; i < 17; i++) acc[i] = 0;
#pragma unroll 1
        for (int j = 0; j < count; j++) fp_mac_wide_s(acc, fr_load(in.t[j], x), in.c[j]);
        u32 v[9];
        fp_redc_wide(v, acc);  // < 16 r^2 / 2^256 + r < 8.3 r
#pragma unroll
        for (int s = 3; s >= 0; s--) lincomb_csub(v, s);
        Fr o;
#pragma unroll
        for (int i = 0; i < 8; i++) o.l[i] = v[i];
        fr_store(out, x, o);
    }
}

int fr_lincomb(zk_ctx* ctx, size_t count, const void* const* d_tabs, const uint64_t* h_coeffs, size_t len, void* d_out) {
    if (count == 0 || count > (size_t)kMultiMax) return fail(ctx, ZK_ERR_INVALID, "zk_fr_lincomb: %zu tables (1 .. %d)", count, kMultiMax);
    for (size_t j = 0; j < count; j++)
        if (!d_tabs[j]) return fail(ctx, ZK_ERR_INVALID, "zk_fr_lincomb: table %zu is null", j);
    if (len == 0) return ZK_OK;
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    LincombIn in;
    std::memset(&in, 0, sizeof(in));
    for (size_t j = 0; j < count; j++) in.t[j] = d_tabs[j], std::memcpy(&in.c[j], h_coeffs + 4 * j, 32);
    const size_t blocks = std::min<size_t>((len + kGateBlock - 1) / kGateBlock, (size_t)ctx->cu_count * 64);
    hipLaunchKernelGGL(k_fr_lincomb, dim3((unsigned)blocks), dim3(kGateBlock), 0, ctx->stream, in, (int)count, len, d_out);
    ZK_HIP(ctx, hipGetLastError());
    return ZK_OK;
}

// ---------------------------------------------------------------------------------------
// K14, one round over count pairs of tables of length 2 * half living in HBM.  partials: [t * nbw + 4 block + wave], 80-byte
// slots, t = 0, 1, 2 (slot set 1 is written by the first pass of a call only).  The products are those of round_pair_lazy
// (zk_fr.hip): t0 += e_lo f_lo, t1 += e_hi f_hi, t2 += (e_hi + de)(f_hi + df) with the factors of t2 left unreduced.
// Only the wide sums live across j: the registers do not grow with count.
// ---------------------------------------------------------------------------------------
template <bool T1>
__global__ void __launch_bounds__(kGateBlock) k_multi_pass(MultiIn in, MultiOut out, int count, size_t half, GateChal ch, void* __restrict__ partials) {
    u32 w0[17], w1[T1 ? 17 : 1], w2[17];
#pragma unroll
    for (int i = 0; i < 17; i++) w0[i] = 0, w2[i] = 0;
#pragma unroll
    for (int i = 0; i < (T1 ? 17 : 1); i++) w1[i] = 0;
#pragma unroll 1
    for (int j = 0; j < count; j++) {
        const void* __restrict__ e = in.e[j];
        const void* __restrict__ f = in.f[j];
        void* eo = reinterpret_cast<char*>(out.base) + (size_t)(2 * j) * out.stride * 32;
        void* fo = reinterpret_cast<char*>(out.base) + (size_t)(2 * j + 1) * out.stride * 32;
        for (size_t i = (size_t)blockIdx.x * kGateBlock + threadIdx.x; i < half; i += (size_t)gridDim.x * kGateBlock) {
            const Fr elo = fr_load(e, i), ehi = fr_load(e, i + half), flo = fr_load(f, i), fhi = fr_load(f, i + half);
            const Fr de = fr_sub(ehi, elo), df = fr_sub(fhi, flo);
            fp_mac_wide(w0, elo, flo);
            if constexpr (T1) fp_mac_wide(w1, ehi, fhi);
            {
                Fr a, b;  // e_hi + de, f_hi + df as integers < 2r   dsumcheck.rs:55-72
                u32 c = 0;
#pragma unroll
                for (int l = 0; l < 8; l++) a.l[l] = addc(ehi.l[l], de.l[l], c);
                c = 0;
#pragma unroll
                for (int l = 0; l < 8; l++) b.l[l] = addc(fhi.l[l], df.l[l], c);
                fp_mac_wide(w2, a, b);
            }
            fr_store(eo, i, fr_add(elo, fr_mul(ch.r, de)));  // lo + r (hi - lo)   dsumcheck.rs:14-19
            fr_store(fo, i, fr_add(flo, fr_mul(ch.r, df)));
        }
    }
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const size_t nbw = (size_t)gridDim.x * (kGateBlock / 64), slot = (size_t)blockIdx.x * (kGateBlock / 64) + wave;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        u32 o[17];
#pragma unroll
        for (int i = 0; i < 17; i++) o[i] = __shfl_down(w0[i], off, 64);
        gate_wide_add(w0, o);
#pragma unroll
        for (int i = 0; i < 17; i++) o[i] = __shfl_down(w2[i], off, 64);
        gate_wide_add(w2, o);
        if constexpr (T1) {
#pragma unroll
            for (int i = 0; i < 17; i++) o[i] = __shfl_down(w1[i], off, 64);
            gate_wide_add(w1, o);
        }
    }
    if (lane == 0) {
        gate_wide_store(partials, slot, w0);
        if constexpr (T1) gate_wide_store(partials, nbw + slot, w1);
        gate_wide_store(partials, 2 * nbw + slot, w2);
    }
}

// The sums of all passes of a call in one launch: block (t, p) = sum t of pass p (gate_reduce_block).  t1 exists for pass 0 only.
__global__ void __launch_bounds__(kGateBlock) k_multi_reduce(const void* __restrict__ partials, GateReducePlan plan, void* __restrict__ evals) {
    __shared__ uint4 lds[(kGateBlock / 64) * (kGateWideBytes / 16)];
    const unsigned t = blockIdx.x, p = blockIdx.y, nbw = plan.nbw[p];
    if (t == 1 && p != 0) return;
    gate_reduce_block(partials, (size_t)plan.off[p] + (size_t)t * nbw, nbw, lds, evals, (size_t)p * 3 + t);
}

// ---------------------------------------------------------------------------------------
// Local stage: all remaining rounds in one workgroup, the 2 count tables of E elements in LDS (table (j, which) at
// (2 j + which) E), folded in place.  The work of a round is count * h items (j, i), i < h = L / 2, spread over the lanes
// (item -> lane item mod 256, as phase B of zk_fr.hip's k_local): an item reads elements i and i + h of its two tables and writes i,
// nobody else touches either before the round's barrier.  Sums: reduced field arithmetic, wave shuffle, one LDS slot per wave
// (two sets, by round parity), three lanes finish.  All three sums are computed here (the host keeps t1 of a call's round 0).
// ---------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kGateBlock) k_multi_local(MultiIn in, int count, unsigned E, int rounds, GateTail chal, void* __restrict__ evals,
                                                           void* __restrict__ last_e, void* __restrict__ last_f) {
    extern __shared__ uint4 mlds[];
    uint4* red = mlds + 2 * (size_t)(2 * count) * E;  // [parity][wave][t] Fr
    const unsigned tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const unsigned lg = 31 - __clz(E);
    for (unsigned it = tid; it < (unsigned)count * E; it += kGateBlock) {
        const unsigned j = it >> lg, i = it & (E - 1);
        fr_store(mlds, (size_t)(2 * j) * E + i, fr_load(in.e[j], i));
        fr_store(mlds, (size_t)(2 * j + 1) * E + i, fr_load(in.f[j], i));
    }
    __syncthreads();
    unsigned L = E, lh = lg;
    for (int rd = 0; rd < rounds; rd++) {
        const unsigned h = L >> 1;
        lh--;
        const Fr r = fr_load(chal.c, rd);
        Fr acc[3];
#pragma unroll
        for (int t = 0; t < 3; t++) acc[t] = fp_zero<FrCfg>();
        for (unsigned it = tid; it < (unsigned)count * h; it += kGateBlock) {
            const unsigned j = it >> lh, i = it & (h - 1);
            const size_t eb = (size_t)(2 * j) * E + i, fb = (size_t)(2 * j + 1) * E + i;
            const Fr elo = fr_load(mlds, eb), ehi = fr_load(mlds, eb + h), flo = fr_load(mlds, fb), fhi = fr_load(mlds, fb + h);
            const Fr de = fr_sub(ehi, elo), df = fr_sub(fhi, flo);
            acc[0] = fr_add(acc[0], fr_mul(elo, flo));
            acc[1] = fr_add(acc[1], fr_mul(ehi, fhi));
            acc[2] = fr_add(acc[2], fr_mul(fr_add(ehi, de), fr_add(fhi, df)));
            fr_store(mlds, eb, fr_add(elo, fr_mul(r, de)));
            fr_store(mlds, fb, fr_add(flo, fr_mul(r, df)));
        }
        uint4* rs = red + 2 * (size_t)(rd & 1) * (kGateBlock / 64) * 3;
#pragma unroll
        for (int t = 0; t < 3; t++) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                Fr o;
#pragma unroll
                for (int i = 0; i < 8; i++) o.l[i] = __shfl_down(acc[t].l[i], off, 64);
                acc[t] = fr_add(acc[t], o);
            }
            if (lane == 0) fr_store(rs, (size_t)wave * 3 + t, acc[t]);
        }
        __syncthreads();
        if (tid < 3) {
            Fr s = fr_load(rs, tid);
            for (int g = 1; g < kGateBlock / 64; g++) s = fr_add(s, fr_load(rs, (size_t)g * 3 + tid));
            fr_store(evals, (size_t)rd * 3 + tid, s);
        }
        L = h;
    }
    if (tid < (unsigned)count) {
        fr_store(last_e, tid, fr_load(mlds, (size_t)(2 * tid) * E));
        fr_store(last_f, tid, fr_load(mlds, (size_t)(2 * tid + 1) * E));
    }
}

// ---------------------------------------------------------------------------------------
// host driver
// ---------------------------------------------------------------------------------------
int sumcheck_multi(zk_ctx* ctx, size_t count, const void* const* d_e, const void* const* d_f, size_t len, const uint64_t* h_chal,
                   uint64_t* h_out_triples, uint64_t* h_last_e, uint64_t* h_last_f) {
    if (count == 0 || count > (size_t)kMultiMax) return fail(ctx, ZK_ERR_INVALID, "zk_sumcheck_multi: %zu pairs (1 .. %d)", count, kMultiMax);
    if (len < 2 || (len & (len - 1))) return fail(ctx, ZK_ERR_INVALID, "zk_sumcheck_multi: table length %zu is not a power of two >= 2", len);
    for (size_t j = 0; j < count; j++)
        if (!d_e[j] || !d_f[j]) return fail(ctx, ZK_ERR_INVALID, "zk_sumcheck_multi: pair %zu has a null table", j);
    size_t rounds = 0;
    while (((size_t)1 << rounds) < len) rounds++;
    if (rounds > (size_t)kMultiMaxLog || count * len > ((size_t)1 << kMultiMaxLog))
        return fail(ctx, ZK_ERR_INVALID, "zk_sumcheck_multi: count * len = %zu * %zu exceeds 2^%d", count, len, kMultiMaxLog);
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    // hand-over point to the local stage: the longest power of two <= multi_local_e whose 2 count tables fit kMultiLdsBytes
    // (knob multi_local_e: 1 = HBM passes down to the last element)
    size_t emax = (size_t)tuning().multi_local_e;
    if (emax < 1 || emax > kGateLocalMax || (emax & (emax - 1))) return fail(ctx, ZK_ERR_INVALID, "multi_local_e must be a power of two in [1, %u]", kGateLocalMax);
    while (emax > 1 && 2 * count * emax * 32 > kMultiLdsBytes) emax >>= 1;
    size_t npass = 0, part_slots = 0;
    GateReducePlan rp;
    std::memset(&rp, 0, sizeof(rp));
    size_t blocks_of[kGateMaxPasses];
    const size_t per_cu = tuning().multi_pass_wg > 0 ? (size_t)tuning().multi_pass_wg : 4;
    for (size_t m = len; m > emax; m >>= 1) {
        if (npass == (size_t)kGateMaxPasses) return fail(ctx, ZK_ERR_INVALID, "zk_sumcheck_multi: table too long");
        const size_t half = m >> 1;
        const size_t blocks = std::min<size_t>((half + kGateBlock - 1) / kGateBlock, (size_t)ctx->cu_count * per_cu);
        blocks_of[npass] = blocks;
        rp.nbw[npass] = (unsigned)(blocks * (kGateBlock / 64));
        rp.off[npass] = (unsigned)part_slots;
        part_slots += 3 * (size_t)rp.nbw[npass];
        npass++;
    }
    const size_t fr = 32;
    const size_t res_bytes = (rounds * 3 + 2 * count) * fr;
    char* res = (char*)pinned(ctx, res_bytes);  // the kernels write the results straight into pinned host memory
    if (!res) return ZK_ERR_OOM;
    char* buf[2] = {nullptr, nullptr};
    char* part = nullptr;
    if (npass) {
        // the arenas of the gate sumcheck: ping-pong tables (2 count of len/2 and 2 count of len/4 elements) and the 544-bit partials
        if (!(buf[0] = (char*)scratch(ctx, 0, 2 * count * (len / 2) * fr))) return ZK_ERR_OOM;
        if (npass > 1 && !(buf[1] = (char*)scratch(ctx, 1, 2 * count * (len / 4) * fr))) return ZK_ERR_OOM;
        if (!(part = (char*)scratch(ctx, 4, part_slots * kGateWideBytes))) return ZK_ERR_OOM;
    }
    MultiIn cur;
    std::memset(&cur, 0, sizeof(cur));
    for (size_t j = 0; j < count; j++) cur.e[j] = d_e[j], cur.f[j] = d_f[j];
    size_t m = len;
    for (size_t p = 0; p < npass; p++) {
        const size_t half = m >> 1;
        const MultiOut o = {buf[p & 1], (p & 1) ? len / 4 : len / 2};
        GateChal ch;
        std::memcpy(&ch.r, h_chal + 4 * p, 32);
        void* pp = (void*)(part + (size_t)rp.off[p] * kGateWideBytes);
        if (p == 0) hipLaunchKernelGGL(k_multi_pass<true>, dim3((unsigned)blocks_of[p]), dim3(kGateBlock), 0, ctx->stream, cur, o, (int)count, half, ch, pp);
        else hipLaunchKernelGGL(k_multi_pass<false>, dim3((unsigned)blocks_of[p]), dim3(kGateBlock), 0, ctx->stream, cur, o, (int)count, half, ch, pp);
        ZK_HIP(ctx, hipGetLastError());
        for (size_t j = 0; j < count; j++) {
            cur.e[j] = (char*)o.base + (2 * j) * o.stride * fr;
            cur.f[j] = (char*)o.base + (2 * j + 1) * o.stride * fr;
        }
        m = half;
    }
    if (npass) {
        hipLaunchKernelGGL(k_multi_reduce, dim3(3, (unsigned)npass), dim3(kGateBlock), 0, ctx->stream, (const void*)part, rp, (void*)res);
        ZK_HIP(ctx, hipGetLastError());
    }
    {
        const int rl = (int)(rounds - npass);
        GateTail tl;
        std::memset(&tl, 0, sizeof(tl));
        std::memcpy(tl.c, h_chal + 4 * npass, (size_t)rl * 32);
        const size_t lds = (2 * 2 * count * m + 2 * 2 * (kGateBlock / 64) * 3) * sizeof(uint4);
        if (lds > 64 * 1024 && !ctx->multi_lds_raised) {  // once per ctx (= per device)
            ZK_HIP(ctx, hipFuncSetAttribute((const void*)k_multi_local, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            ctx->multi_lds_raised = true;
        }
        hipLaunchKernelGGL(k_multi_local, dim3(1), dim3(kGateBlock), lds, ctx->stream, cur, (int)count, (unsigned)m, rl, tl, (void*)(res + npass * 3 * fr),
                           (void*)(res + rounds * 3 * fr), (void*)(res + (rounds * 3 + count) * fr));
        ZK_HIP(ctx, hipGetLastError());
    }
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    // t1 of the passes after the first: t0 + t1 of a round is the previous round polynomial at its challenge.  The local stage's
    // own t1 are kept (round npass on), so the derivation covers rounds 1 .. npass - 1.
    if (npass > 1) derive_t1((uint64_t*)res, h_chal, npass);
    std::memcpy(h_out_triples, res, rounds * 3 * fr);
    std::memcpy(h_last_e, res + rounds * 3 * fr, count * fr);
    std::memcpy(h_last_f, res + (rounds * 3 + count) * fr, count * fr);
    return ZK_OK;
}

}  // namespace zk
