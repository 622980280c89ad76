// zk_fs.hip -- the seven fused sumchecks (zk_gate.hip, zk_wiring.hip, zk_perm3.hip, zk_gatew.hip, zk_lookup.hip, zk_lookup3.hip, zk_batchopen.hip) with their challenges drawn from a
// Fiat-Shamir transcript ON THE DEVICE (zk_transcript.hip, sha256.cuh): challenge r_p is a hash of round p's evaluations, so the
// fold by r_p cannot share a sweep with round p's sums as it does in the preset-challenge kernels (zk_fused.cuh).  The identities are
// the Kind structs of zk_gate.cuh, the ones the preset-challenge engine runs.  The shape here:
//   pass 0            evaluate only: the sums of round 0 over the caller's tables (nothing is written but the partials),
//   pass p >= 1       fold, then evaluate: a lane reads elements j, j + q, j + 2q, j + 3q of each table (q = a quarter of the
//                     table), folds the pairs (j, j + 2q) and (j + q, j + 3q) with r_{p-1} LOADED FROM DEVICE MEMORY, writes the two
//                     folded elements to ping-pong scratch and adds round p's products of them,
//   after every pass  k_fs_reduce_hash: one workgroup adds the per-wave 544-bit partials, reduces them, and lane 0 absorbs the
//                     evaluations into the transcript, draws r_p and stores it for the next kernel,
//   local stage       one workgroup: the pending fold by the last pass's challenge while loading into LDS, then per round sums,
//                     barrier, lane 0 hashes and publishes the challenge in LDS, barrier, fold.
// One enqueue and one stream synchronisation per call; no host read between the first launch and the last.  Two launches per HBM
// round (pass, reduce-and-hash) and one for the local stage.  The sums, their association into 544-bit integers and the reduction
// are those of the parents, and every value is a canonical field element: for the challenges a call derived, the parent returns
// the same bits (tests/test_gpu_fs.py).  Inputs are never written.
#include "sha256.cuh"
#include "zk_gate.cuh"

#include <algorithm>
#include <cstring>

namespace zk {

// ---------------------------------------------------------------------------------------
// One round of an identity of K::kTabs tables over HBM.  FOLD: the tables at `in` have 4 * half elements and are folded with *d_chal
// into `out` (2 * half elements each) first; otherwise they have 2 * half elements and nothing is stored.
// partials: [t * nbw + 4 block + wave], 80-byte slots, as k_sc_pass.
// ---------------------------------------------------------------------------------------
template <class K, bool FOLD>
__global__ void __launch_bounds__(kGateBlock) __attribute__((amdgpu_waves_per_eu(1, K::kWaves)))
k_fs_pass(FsIn<K::kTabs> in, FsOut<K::kTabs> out, size_t half, const void* __restrict__ d_chal, GateChal gamma, void* __restrict__ partials) {
    u32 w[K::kEvals][17];
#pragma unroll
    for (int t = 0; t < K::kEvals; t++)
#pragma unroll
        for (int i = 0; i < 17; i++) w[t][i] = 0;
    Fr r = fp_zero<FrCfg>();
    if (FOLD) r = fr_load(d_chal, 0);
    Fr g0 = fp_zero<FrCfg>(), gd = fp_zero<FrCfg>();  // kFree: the lane's sums of free(lo) and free(hi - lo)
    for (size_t j = (size_t)blockIdx.x * kGateBlock + threadIdx.x; j < half; j += (size_t)gridDim.x * kGateBlock) {
        Fr v[K::kTabs], d[K::kTabs];
#pragma unroll
        for (int k = 0; k < K::kTabs; k++) {
            const unsigned sh = in.sh[k];
            if (FOLD) {
                const Fr a0 = fr_load(in.t[k], j << sh), a1 = fr_load(in.t[k], (j + half) << sh);
                const Fr a2 = fr_load(in.t[k], (j + 2 * half) << sh), a3 = fr_load(in.t[k], (j + 3 * half) << sh);
                v[k] = fr_add(a0, fr_mul(r, fr_sub(a2, a0)));  // lo + r (hi - lo)   dsumcheck.rs:14-19
                const Fr hi = fr_add(a1, fr_mul(r, fr_sub(a3, a1)));
                fr_store(out.t[k], j, v[k]);
                fr_store(out.t[k], j + half, hi);
                d[k] = fr_sub(hi, v[k]);
            } else {
                v[k] = fr_load(in.t[k], j << sh);
                d[k] = fr_sub(fr_load(in.t[k], (j + half) << sh), v[k]);
            }
        }
        if constexpr (K::kFree) g0 = fr_add(g0, K::free(v)), gd = fr_add(gd, K::free(d));
        kind_sums_wide<K>(w, gamma.r, v, d);
    }
    if constexpr (K::kFree) kind_free_wide<K>(w, g0, gd);
    gate_wave_store_wide(w, partials);
}

// The NE sums of ONE pass, then the transcript: lane 0 writes the evaluations to the results, absorbs them, draws the round's
// challenge and stores it twice -- in device memory for the next kernel, in the results for the caller.
template <int NE>
__global__ void __launch_bounds__(kGateBlock) k_fs_reduce_hash(const void* __restrict__ partials, unsigned nbw, u32* __restrict__ state, void* __restrict__ evals,
                                                              void* __restrict__ d_chal, void* __restrict__ h_chal) {
    __shared__ uint4 lds[(kGateBlock / 64) * (kGateWideBytes / 16)];
    Fr ev[NE];
#pragma unroll 1
    for (int t = 0; t < NE; t++) {
        ev[t] = gate_reduce_value(partials, (size_t)t * nbw, nbw, lds);
        __syncthreads();  // lane 0 has read every slot before the next sum overwrites them
    }
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int t = 0; t < NE; t++) fr_store(evals, t, ev[t]);
    u32 st[8];
    fs_state_load(st, state);
    const Fr r = fs_round<NE>(st, ev);
    fs_state_store(state, st);
    fr_store(d_chal, 0, r);
    fr_store(h_chal, 0, r);
}

// ---------------------------------------------------------------------------------------
// Local stage of an identity of K::kTabs tables: tables of E <= K::kLocalMax elements in LDS.  d_pending (or null): the challenge of the last HBM
// pass -- the tables at `in` then have 2 E elements and are folded while they are loaded.  Per round: the sums (wave shuffle, one
// LDS slot per wave), barrier, lane 0 finishes them, hashes and leaves the challenge in LDS, barrier, the fold in place (a lane
// reads elements j and j + h of each table and writes j), barrier.
// ---------------------------------------------------------------------------------------
template <class K>
__global__ void __launch_bounds__(kGateBlock) k_fs_local(FsIn<K::kTabs> in, unsigned E, int rounds, const void* __restrict__ d_pending, GateChal gamma, u32* __restrict__ state,
                                                        void* __restrict__ evals, void* __restrict__ h_chal, void* __restrict__ last) {
    extern __shared__ uint4 flds[];
    uint4* red = flds + 2 * (size_t)K::kTabs * E;              // [wave][t] Fr
    uint4* cs = red + 2 * (size_t)(kGateBlock / 64) * K::kEvals;  // the round's challenge
    const unsigned tid = threadIdx.x;
    if (d_pending) {
        const Fr r = fr_load(d_pending, 0);
        for (unsigned i = tid; i < E; i += kGateBlock)
#pragma unroll
            for (int k = 0; k < K::kTabs; k++) {
                const Fr lo = fr_load(in.t[k], (size_t)i << in.sh[k]), hi = fr_load(in.t[k], (size_t)(i + E) << in.sh[k]);
                fr_store(flds, (size_t)k * E + i, fr_add(lo, fr_mul(r, fr_sub(hi, lo))));
            }
    } else {
        for (unsigned i = tid; i < E; i += kGateBlock)
#pragma unroll
            for (int k = 0; k < K::kTabs; k++) fr_store(flds, (size_t)k * E + i, fr_load(in.t[k], (size_t)i << in.sh[k]));
    }
    __syncthreads();
    u32 st[8];
    if (tid == 0) fs_state_load(st, state);
    unsigned L = E;
    for (int rd = 0; rd < rounds; rd++) {
        const unsigned h = L >> 1;
        Fr acc[K::kEvals];
#pragma unroll
        for (int t = 0; t < K::kEvals; t++) acc[t] = fp_zero<FrCfg>();
        for (unsigned j = tid; j < h; j += kGateBlock) {
            Fr v[K::kTabs], d[K::kTabs];
#pragma unroll
            for (int k = 0; k < K::kTabs; k++) {
                v[k] = fr_load(flds, (size_t)k * E + j);
                d[k] = fr_sub(fr_load(flds, (size_t)k * E + j + h), v[k]);
            }
            kind_sums_fr<K>(acc, gamma.r, v, d);
        }
        gate_wave_store_fr(acc, red);
        __syncthreads();
        if (tid == 0) {
            Fr ev[K::kEvals];
#pragma unroll
            for (int t = 0; t < K::kEvals; t++) {
                ev[t] = fr_load(red, t);
                for (int g = 1; g < kGateBlock / 64; g++) ev[t] = fr_add(ev[t], fr_load(red, (size_t)g * K::kEvals + t));
                fr_store(evals, (size_t)rd * K::kEvals + t, ev[t]);
            }
            const Fr r = fs_round<K::kEvals>(st, ev);
            fr_store(h_chal, rd, r);
            fr_store(cs, 0, r);
        }
        __syncthreads();
        const Fr r = fr_load(cs, 0);
        for (unsigned j = tid; j < h; j += kGateBlock)
#pragma unroll
            for (int k = 0; k < K::kTabs; k++) {
                const Fr lo = fr_load(flds, (size_t)k * E + j), hi = fr_load(flds, (size_t)k * E + j + h);
                fr_store(flds, (size_t)k * E + j, fr_add(lo, fr_mul(r, fr_sub(hi, lo))));
            }
        __syncthreads();
        L = h;
    }
    if (tid == 0 && rounds > 0) fs_state_store(state, st);
    if (tid < K::kTabs) fr_store(last, tid, fr_load(flds, (size_t)tid * E));
}

// ---------------------------------------------------------------------------------------
// The batch-opening sumcheck: k_multi_pass / k_multi_local of zk_batchopen.hip in the same two forms.  t1 is summed in EVERY pass:
// it has to exist on the device before the round is hashed (the parent derives t1 of its later passes on the host).
// ---------------------------------------------------------------------------------------
template <bool FOLD>
__global__ void __launch_bounds__(kGateBlock) k_multi_fs_pass(MultiIn in, MultiOut out, int count, size_t half, const void* __restrict__ d_chal,
                                                             void* __restrict__ partials) {
    u32 w[3][17];
#pragma unroll
    for (int t = 0; t < 3; t++)
#pragma unroll
        for (int i = 0; i < 17; i++) w[t][i] = 0;
    Fr r = fp_zero<FrCfg>();
    if (FOLD) r = fr_load(d_chal, 0);
#pragma unroll 1
    for (int j = 0; j < count; j++) {
        const void* __restrict__ e = in.e[j];
        const void* __restrict__ f = in.f[j];
        void* eo = reinterpret_cast<char*>(out.base) + (size_t)(2 * j) * out.stride * 32;
        void* fo = reinterpret_cast<char*>(out.base) + (size_t)(2 * j + 1) * out.stride * 32;
        for (size_t i = (size_t)blockIdx.x * kGateBlock + threadIdx.x; i < half; i += (size_t)gridDim.x * kGateBlock) {
            Fr elo, ehi, flo, fhi;
            if (FOLD) {
                const Fr e0 = fr_load(e, i), e1 = fr_load(e, i + half), e2 = fr_load(e, i + 2 * half), e3 = fr_load(e, i + 3 * half);
                const Fr f0 = fr_load(f, i), f1 = fr_load(f, i + half), f2 = fr_load(f, i + 2 * half), f3 = fr_load(f, i + 3 * half);
                elo = fr_add(e0, fr_mul(r, fr_sub(e2, e0))), ehi = fr_add(e1, fr_mul(r, fr_sub(e3, e1)));  // lo + r (hi - lo)   dsumcheck.rs:14-19
                flo = fr_add(f0, fr_mul(r, fr_sub(f2, f0))), fhi = fr_add(f1, fr_mul(r, fr_sub(f3, f1)));
                fr_store(eo, i, elo), fr_store(eo, i + half, ehi);
                fr_store(fo, i, flo), fr_store(fo, i + half, fhi);
            } else {
                elo = fr_load(e, i), ehi = fr_load(e, i + half), flo = fr_load(f, i), fhi = fr_load(f, i + half);
            }
            const Fr de = fr_sub(ehi, elo), df = fr_sub(fhi, flo);
            fp_mac_wide(w[0], elo, flo);
            fp_mac_wide(w[1], ehi, fhi);
            Fr a, b;  // e_hi + de, f_hi + df as integers < 2r   dsumcheck.rs:55-72
            u32 c = 0;
#pragma unroll
            for (int l = 0; l < 8; l++) a.l[l] = addc(ehi.l[l], de.l[l], c);
            c = 0;
#pragma unroll
            for (int l = 0; l < 8; l++) b.l[l] = addc(fhi.l[l], df.l[l], c);
            fp_mac_wide(w[2], a, b);
        }
    }
    gate_wave_store_wide(w, partials);
}

// Local stage: the 2 count tables of E elements in LDS (table (j, which) at (2 j + which) E), items (j, i) spread over the lanes as
// in k_multi_local; d_pending and the round structure as in k_fs_local.
__global__ void __launch_bounds__(kGateBlock) k_multi_fs_local(MultiIn in, int count, unsigned E, int rounds, const void* __restrict__ d_pending, u32* __restrict__ state,
                                                              void* __restrict__ evals, void* __restrict__ h_chal, void* __restrict__ last_e, void* __restrict__ last_f) {
    extern __shared__ uint4 mflds[];
    uint4* red = mflds + 2 * (size_t)(2 * count) * E;       // [wave][t] Fr
    uint4* cs = red + 2 * (size_t)(kGateBlock / 64) * 3;     // the round's challenge
    const unsigned tid = threadIdx.x;
    const unsigned lg = 31 - __clz(E);
    Fr rp = fp_zero<FrCfg>();
    if (d_pending) rp = fr_load(d_pending, 0);
    for (unsigned it = tid; it < (unsigned)count * E; it += kGateBlock) {
        const unsigned j = it >> lg, i = it & (E - 1);
        Fr ev = fr_load(in.e[j], i), fv = fr_load(in.f[j], i);
        if (d_pending) {
            ev = fr_add(ev, fr_mul(rp, fr_sub(fr_load(in.e[j], i + E), ev)));
            fv = fr_add(fv, fr_mul(rp, fr_sub(fr_load(in.f[j], i + E), fv)));
        }
        fr_store(mflds, (size_t)(2 * j) * E + i, ev);
        fr_store(mflds, (size_t)(2 * j + 1) * E + i, fv);
    }
    __syncthreads();
    u32 st[8];
    if (tid == 0) fs_state_load(st, state);
    unsigned L = E, lh = lg;
    for (int rd = 0; rd < rounds; rd++) {
        const unsigned h = L >> 1;
        lh--;
        Fr acc[3];
#pragma unroll
        for (int t = 0; t < 3; t++) acc[t] = fp_zero<FrCfg>();
        for (unsigned it = tid; it < (unsigned)count * h; it += kGateBlock) {
            const unsigned j = it >> lh, i = it & (h - 1);
            const size_t eb = (size_t)(2 * j) * E + i, fb = (size_t)(2 * j + 1) * E + i;
            const Fr elo = fr_load(mflds, eb), ehi = fr_load(mflds, eb + h), flo = fr_load(mflds, fb), fhi = fr_load(mflds, fb + h);
            const Fr de = fr_sub(ehi, elo), df = fr_sub(fhi, flo);
            acc[0] = fr_add(acc[0], fr_mul(elo, flo));
            acc[1] = fr_add(acc[1], fr_mul(ehi, fhi));
            acc[2] = fr_add(acc[2], fr_mul(fr_add(ehi, de), fr_add(fhi, df)));
        }
        gate_wave_store_fr(acc, red);
        __syncthreads();
        if (tid == 0) {
            Fr ev[3];
#pragma unroll
            for (int t = 0; t < 3; t++) {
                ev[t] = fr_load(red, t);
                for (int g = 1; g < kGateBlock / 64; g++) ev[t] = fr_add(ev[t], fr_load(red, (size_t)g * 3 + t));
                fr_store(evals, (size_t)rd * 3 + t, ev[t]);
            }
            const Fr r = fs_round<3>(st, ev);
            fr_store(h_chal, rd, r);
            fr_store(cs, 0, r);
        }
        __syncthreads();
        const Fr r = fr_load(cs, 0);
        for (unsigned it = tid; it < (unsigned)count * h; it += kGateBlock) {
            const unsigned j = it >> lh, i = it & (h - 1);
            const size_t eb = (size_t)(2 * j) * E + i, fb = (size_t)(2 * j + 1) * E + i;
            const Fr elo = fr_load(mflds, eb), ehi = fr_load(mflds, eb + h), flo = fr_load(mflds, fb), fhi = fr_load(mflds, fb + h);
            fr_store(mflds, eb, fr_add(elo, fr_mul(r, fr_sub(ehi, elo))));
            fr_store(mflds, fb, fr_add(flo, fr_mul(r, fr_sub(fhi, flo))));
        }
        __syncthreads();
        L = h;
    }
    if (tid == 0 && rounds > 0) fs_state_store(state, st);
    if (tid < (unsigned)count) {
        fr_store(last_e, tid, fr_load(mflds, (size_t)(2 * tid) * E));
        fr_store(last_f, tid, fr_load(mflds, (size_t)(2 * tid + 1) * E));
    }
}

// ---------------------------------------------------------------------------------------
// host drivers
// ---------------------------------------------------------------------------------------
// The launch plan of a call: pass p works on tables of len >> p elements, `npass` passes while they are longer than emax
struct FsPlan {
    size_t rounds = 0, npass = 0;
    size_t blocks[kGateMaxPasses];
    char* chal = nullptr;  // device: one Fr per pass
    char* part = nullptr;  // device: the partials of ONE pass (every pass is reduced before the next starts)
    char* buf[2] = {nullptr, nullptr};
};

// the part the three calls share: checks, the hand-over point, the arenas of the parents (0 and 1: ping-pong tables, 4: challenges | partials)
static int fs_plan(zk_ctx* ctx, const char* who, const zk_transcript* t, size_t len, int max_log, size_t emax, size_t per_cu, int sums, size_t tabs, FsPlan& pl) {
    if (!t) return fail(ctx, ZK_ERR_INVALID, "%s: null transcript", who);
    if (t->ctx != ctx) return fail(ctx, ZK_ERR_INVALID, "%s: the transcript belongs to another ctx", who);
    if (len < 2 || (len & (len - 1))) return fail(ctx, ZK_ERR_INVALID, "%s: table length %zu is not a power of two >= 2", who, len);
    while (((size_t)1 << pl.rounds) < len) pl.rounds++;
    if (pl.rounds > (size_t)max_log) return fail(ctx, ZK_ERR_INVALID, "%s: tables longer than 2^%d elements", who, max_log);
    for (size_t m = len; m > emax; m >>= 1) {
        if (pl.npass == (size_t)kGateMaxPasses) return fail(ctx, ZK_ERR_INVALID, "%s: table too long", who);
        pl.blocks[pl.npass++] = std::min<size_t>(((m >> 1) + kGateBlock - 1) / kGateBlock, (size_t)ctx->cu_count * per_cu);
    }
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t chal_bytes = (size_t)kGateMaxPasses * 32;
    const size_t part_bytes = pl.npass ? (size_t)sums * pl.blocks[0] * (kGateBlock / 64) * kGateWideBytes : 0;
    if (!(pl.chal = (char*)scratch(ctx, 4, chal_bytes + part_bytes))) return ZK_ERR_OOM;
    pl.part = pl.chal + chal_bytes;
    // pass p >= 1 writes tables of len >> p elements: len/2 into arena 0, len/4 into arena 1, len/8 into arena 0 ...
    if (pl.npass > 1 && !(pl.buf[0] = (char*)scratch(ctx, 0, tabs * (len / 2) * 32))) return ZK_ERR_OOM;
    if (pl.npass > 2 && !(pl.buf[1] = (char*)scratch(ctx, 1, tabs * (len / 4) * 32))) return ZK_ERR_OOM;
    return ZK_OK;
}

// b: the identity's binding of the caller's arguments (Bound, zk_gate.cuh); its *_local_e knob is checked before anything else
template <class K>
static int run_fs(zk_ctx* ctx, const char* who, const Bound<K>& b, size_t len, zk_transcript* t, uint64_t* h_out_evals, uint64_t* h_last, uint64_t* h_chal_out) {
    const GateChal& gamma = b.gamma;
    size_t emax;
    int rc = local_e(ctx, b.knob, b.knob_name, emax, K::kLocalMax);
    if (rc) return rc;
    FsPlan pl;
    rc = fs_plan(ctx, who, t, len, kGateMaxLog, emax, b.per_cu, K::kEvals, K::kTabs, pl);
    if (rc) return rc;
    const size_t fr = 32, rounds = pl.rounds, npass = pl.npass;
    char* res = (char*)pinned(ctx, (rounds * K::kEvals + K::kTabs + rounds) * fr);  // evaluations | last | challenges, written by the kernels
    if (!res) return ZK_ERR_OOM;
    char* res_last = res + rounds * K::kEvals * fr;
    char* res_chal = res_last + K::kTabs * fr;
    FsIn<K::kTabs> cur = b.first;
    for (size_t p = 0; p < npass; p++) {
        const size_t half = len >> (p + 1);
        if (p == 0) {
            hipLaunchKernelGGL((k_fs_pass<K, false>), dim3((unsigned)pl.blocks[p]), dim3(kGateBlock), 0, ctx->stream, cur, FsOut<K::kTabs>{}, half, (const void*)nullptr, gamma,
                               (void*)pl.part);
        } else {
            FsOut<K::kTabs> o;
            const size_t stride = ((p - 1) & 1) ? len / 4 : len / 2;
            for (int k = 0; k < K::kTabs; k++) o.t[k] = pl.buf[(p - 1) & 1] + (size_t)k * stride * fr;
            hipLaunchKernelGGL((k_fs_pass<K, true>), dim3((unsigned)pl.blocks[p]), dim3(kGateBlock), 0, ctx->stream, cur, o, half, (const void*)(pl.chal + (p - 1) * fr),
                               gamma, (void*)pl.part);
            for (int k = 0; k < K::kTabs; k++) cur.t[k] = o.t[k], cur.sh[k] = 0;
        }
        ZK_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL(k_fs_reduce_hash<K::kEvals>, dim3(1), dim3(kGateBlock), 0, ctx->stream, (const void*)pl.part, (unsigned)(pl.blocks[p] * (kGateBlock / 64)),
                           t->d_state, (void*)(res + p * K::kEvals * fr), (void*)(pl.chal + p * fr), (void*)(res_chal + p * fr));
        ZK_HIP(ctx, hipGetLastError());
    }
    {
        const size_t E = len >> npass;
        const size_t lds = (2 * (size_t)K::kTabs * E + 2 * (kGateBlock / 64) * K::kEvals + 2) * sizeof(uint4);
        if (lds > 64 * 1024 && !ctx->fs_lds_raised[K::kSlot]) {  // once per ctx (= per device)
            ZK_HIP(ctx, hipFuncSetAttribute((const void*)k_fs_local<K>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            ctx->fs_lds_raised[K::kSlot] = true;
        }
        hipLaunchKernelGGL(k_fs_local<K>, dim3(1), dim3(kGateBlock), lds, ctx->stream, cur, (unsigned)E, (int)(rounds - npass),
                           (const void*)(npass ? pl.chal + (npass - 1) * fr : nullptr), gamma, t->d_state, (void*)(res + npass * K::kEvals * fr),
                           (void*)(res_chal + npass * fr), (void*)res_last);
        ZK_HIP(ctx, hipGetLastError());
    }
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(h_out_evals, res, rounds * K::kEvals * fr);
    std::memcpy(h_last, res_last, K::kTabs * fr);
    std::memcpy(h_chal_out, res_chal, rounds * fr);
    return ZK_OK;
}

int sumcheck_gate_fs(zk_ctx* ctx, const void* const* d_tabs, size_t len, zk_transcript* t, uint64_t* h_out_evals, uint64_t* h_last, uint64_t* h_chal_out) {
    return run_fs<GateKind>(ctx, "zk_sumcheck_gate_fs", bind_gate(d_tabs), len, t, h_out_evals, h_last, h_chal_out);
}

int sumcheck_wiring_fs(zk_ctx* ctx, const void* d_eq, const void* d_tree, const void* d_num, const void* d_den, size_t N, const uint64_t* h_gamma, zk_transcript* t,
                       uint64_t* h_out_evals, uint64_t* h_last, uint64_t* h_chal_out) {
    return run_fs<WireKind>(ctx, "zk_sumcheck_wiring_fs", bind_wiring(d_eq, d_tree, d_num, d_den, N, h_gamma), N, t, h_out_evals, h_last, h_chal_out);
}

int sumcheck_perm3_fs(zk_ctx* ctx, const void* d_eq, const void* d_tree, const void* const* d_num, const void* const* d_den, size_t N, const uint64_t* h_gamma,
                      zk_transcript* t, uint64_t* h_out_evals, uint64_t* h_last, uint64_t* h_chal_out) {
    return run_fs<Perm3Kind>(ctx, "zk_sumcheck_perm3_fs", bind_perm3(d_eq, d_tree, d_num, d_den, N, h_gamma), N, t, h_out_evals, h_last, h_chal_out);
}

int sumcheck_gate_wide_fs(zk_ctx* ctx, const void* const* d_tabs, size_t len, zk_transcript* t, uint64_t* h_out_evals, uint64_t* h_last, uint64_t* h_chal_out) {
    return run_fs<GatewKind>(ctx, "zk_sumcheck_gate_wide_fs", bind_gate_wide(d_tabs), len, t, h_out_evals, h_last, h_chal_out);
}

int sumcheck_lookup_fs(zk_ctx* ctx, const void* const* d_tabs, size_t len, const uint64_t* h_gamma, zk_transcript* t, uint64_t* h_out_evals, uint64_t* h_last,
                       uint64_t* h_chal_out) {
    return run_fs<LookupKind>(ctx, "zk_sumcheck_lookup_fs", bind_lookup(d_tabs, h_gamma), len, t, h_out_evals, h_last, h_chal_out);
}

int sumcheck_lookup_sel_fs(zk_ctx* ctx, const void* const* d_tabs, size_t len, const uint64_t* h_gamma, zk_transcript* t, uint64_t* h_out_evals, uint64_t* h_last,
                           uint64_t* h_chal_out) {
    return run_fs<LookupSelKind>(ctx, "zk_sumcheck_lookup_sel_fs", bind_lookup_sel(d_tabs, h_gamma), len, t, h_out_evals, h_last, h_chal_out);
}

int sumcheck_multi_fs(zk_ctx* ctx, size_t count, const void* const* d_e, const void* const* d_f, size_t len, zk_transcript* t, uint64_t* h_out_triples,
                      uint64_t* h_last_e, uint64_t* h_last_f, uint64_t* h_chal_out) {
    const char* who = "zk_sumcheck_multi_fs";
    if (count == 0 || count > (size_t)kMultiMax) return fail(ctx, ZK_ERR_INVALID, "%s: %zu pairs (1 .. %d)", who, count, kMultiMax);
    for (size_t j = 0; j < count; j++)
        if (!d_e[j] || !d_f[j]) return fail(ctx, ZK_ERR_INVALID, "%s: pair %zu has a null table", who, j);
    if (len > ((size_t)1 << kMultiMaxLog) || count * len > ((size_t)1 << kMultiMaxLog))
        return fail(ctx, ZK_ERR_INVALID, "%s: count * len = %zu * %zu exceeds 2^%d", who, count, len, kMultiMaxLog);
    // hand-over point: the longest power of two <= multi_local_e whose 2 count tables fit kMultiLdsBytes, as zk_sumcheck_multi
    size_t emax;
    int rc = local_e(ctx, tuning().multi_local_e, "multi_local_e", emax);
    if (rc) return rc;
    while (emax > 1 && 2 * count * emax * 32 > kMultiLdsBytes) emax >>= 1;
    FsPlan pl;
    rc = fs_plan(ctx, who, t, len, kMultiMaxLog, emax, tuning().multi_pass_wg > 0 ? (size_t)tuning().multi_pass_wg : 4, 3, 2 * count, pl);
    if (rc) return rc;
    const size_t fr = 32, rounds = pl.rounds, npass = pl.npass;
    char* res = (char*)pinned(ctx, (rounds * 3 + 2 * count + rounds) * fr);  // triples | last_e | last_f | challenges
    if (!res) return ZK_ERR_OOM;
    char* res_last = res + rounds * 3 * fr;
    char* res_chal = res_last + 2 * count * fr;
    MultiIn cur;
    std::memset(&cur, 0, sizeof(cur));
    for (size_t j = 0; j < count; j++) cur.e[j] = d_e[j], cur.f[j] = d_f[j];
    for (size_t p = 0; p < npass; p++) {
        const size_t half = len >> (p + 1);
        if (p == 0) {
            hipLaunchKernelGGL(k_multi_fs_pass<false>, dim3((unsigned)pl.blocks[p]), dim3(kGateBlock), 0, ctx->stream, cur, MultiOut{nullptr, 0}, (int)count, half,
                               (const void*)nullptr, (void*)pl.part);
        } else {
            const MultiOut o = {pl.buf[(p - 1) & 1], ((p - 1) & 1) ? len / 4 : len / 2};
            hipLaunchKernelGGL(k_multi_fs_pass<true>, dim3((unsigned)pl.blocks[p]), dim3(kGateBlock), 0, ctx->stream, cur, o, (int)count, half,
                               (const void*)(pl.chal + (p - 1) * fr), (void*)pl.part);
            for (size_t j = 0; j < count; j++) {
                cur.e[j] = (char*)o.base + (2 * j) * o.stride * fr;
                cur.f[j] = (char*)o.base + (2 * j + 1) * o.stride * fr;
            }
        }
        ZK_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL(k_fs_reduce_hash<3>, dim3(1), dim3(kGateBlock), 0, ctx->stream, (const void*)pl.part, (unsigned)(pl.blocks[p] * (kGateBlock / 64)), t->d_state,
                           (void*)(res + p * 3 * fr), (void*)(pl.chal + p * fr), (void*)(res_chal + p * fr));
        ZK_HIP(ctx, hipGetLastError());
    }
    {
        const size_t E = len >> npass;
        const size_t lds = (2 * 2 * count * E + 2 * (kGateBlock / 64) * 3 + 2) * sizeof(uint4);
        if (lds > 64 * 1024 && !ctx->fs_lds_raised[2]) {  // once per ctx (= per device)
            ZK_HIP(ctx, hipFuncSetAttribute((const void*)k_multi_fs_local, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
            ctx->fs_lds_raised[2] = true;
        }
        hipLaunchKernelGGL(k_multi_fs_local, dim3(1), dim3(kGateBlock), lds, ctx->stream, cur, (int)count, (unsigned)E, (int)(rounds - npass),
                           (const void*)(npass ? pl.chal + (npass - 1) * fr : nullptr), t->d_state, (void*)(res + npass * 3 * fr), (void*)(res_chal + npass * fr),
                           (void*)res_last, (void*)(res_last + count * fr));
        ZK_HIP(ctx, hipGetLastError());
    }
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::memcpy(h_out_triples, res, rounds * 3 * fr);
    std::memcpy(h_last_e, res_last, count * fr);
    std::memcpy(h_last_f, res_last + count * fr, count * fr);
    std::memcpy(h_chal_out, res_chal, rounds * fr);
    return ZK_OK;
}

}  // namespace zk
