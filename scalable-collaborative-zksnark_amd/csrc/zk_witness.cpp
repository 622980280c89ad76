// zk_witness.cpp -- the witness plan of one Plonk circuit, built ONCE per circuit on the host in O(N) (include/zkhip.h states the rules):
//   1. sigma is checked to be a permutation of the 3N slots; the cycles are walked, every slot gets its SOURCE as a u32 -- the row whose
//      c slot is the smallest c slot of a computing row in the cycle, or kWitFree | the cycle's smallest slot when it has none;
//   2. the levels of the computing rows by Kahn's algorithm on the edges (source row of the a / b slot) -> row; what it cannot reach
//      depends on its own output and the plan is refused;
//   3. a counting sort by (level, row), the level offsets, and the launch schedule of zk_witness.hip: a level of more than kWitBlock rows
//      is a launch of its own, a run of consecutive smaller levels is ONE launch of ONE workgroup;
//   4. the uploads: src, the row order, the level offsets and, with an output selector, 1 / qO on the gate-computing rows (zk_fr_batch_div).
// A LOOKUP plan (d_qk, d_t given) differs in two places: before step 1 the selector qk is read and checked (0 or 1), the key table of
// (t0, t1) is built on the device (zk_witness.hip, witness_key_table) and the rows with qk = 1 that are not gate-computing become
// LOOKUP-COMPUTING; steps 1 - 3 treat both kinds alike, and the order entry of a lookup-computing row carries kWitLookup.
// An ADVICE plan (h_advice with a non-zero code) differs in three: the codes are checked (unknown ones, and rows that also compute by the
// gate or the table, are refused), a row with a code is ADVICE-COMPUTING (kind 3 in comp) for steps 1 - 3, and step 3 orders a level by
// (kind, row) with the advice rows last, so that they are contiguous; their order entries carry kWitAdvice and the plan keeps the codes
// on the device.  With all codes zero every step does what it did.
// Why on the host: it runs once per circuit and is serial on a deep circuit anyway; the per-proof work is zk_witness.hip.
#include "fp.cuh"
#include "zk_ctx.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

namespace zk {

void witness_plan_free(zk_witness_plan* plan) {
    if (!plan) return;
    if (plan->ctx) (void)hipSetDevice(plan->ctx->device);
    if (plan->d_src) (void)hipFree(plan->d_src);
    if (plan->d_order) (void)hipFree(plan->d_order);
    if (plan->d_lvoff) (void)hipFree(plan->d_lvoff);
    if (plan->d_inv) (void)hipFree(plan->d_inv);
    if (plan->d_slots) (void)hipFree(plan->d_slots);
    if (plan->d_advice) (void)hipFree(plan->d_advice);
    delete plan;
}

namespace {
struct PlanGuard {  // frees a half-built plan on every early return
    zk_witness_plan* p;
    ~PlanGuard() { witness_plan_free(p); }
};
struct DevGuard {
    void* p = nullptr;
    ~DevGuard() {
        if (p) (void)hipFree(p);
    }
};
int upload_u32(zk_ctx* ctx, const std::vector<uint32_t>& v, uint32_t** d_out) {
    ZK_HIP(ctx, device_alloc(ctx, (void**)d_out, std::max<size_t>(v.size(), 1) * sizeof(uint32_t)));
    if (!v.empty()) ZK_HIP(ctx, hipMemcpy(*d_out, v.data(), v.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    return ZK_OK;
}
// an advice code (include/zkhip.h): 0, ADV_INV0, or ADV_BITS with 1 <= width <= 64 and shift + width <= 255; bits 24 .. 31 are zero
bool advice_code_known(uint32_t code) {
    const uint32_t kind = code & 0xff, shift = (code >> 8) & 0xff, width = (code >> 16) & 0xff;
    if (code >> 24) return false;
    if (kind == 0 || kind == 1) return code == kind;
    return kind == 2 && width >= 1 && width <= 64 && shift + width <= 255;
}
}  // namespace

int witness_plan_create(zk_ctx* ctx, const char* name, const uint64_t* h_sigma, const void* d_out_sel, const void* d_qk, const void* const* d_t, const uint32_t* h_advice,
                        size_t N, zk_witness_plan** out) {
    *out = nullptr;
    if (N < 2 || (N & (N - 1)) || N > ((size_t)1 << 29)) return fail(ctx, ZK_ERR_INVALID, "%s: N = %zu is not a power of two in [2, 2^29]", name, N);
    const size_t S = 3 * N;
    ZK_HIP(ctx, hipSetDevice(ctx->device));
    // sigma: every slot number below 3N, each exactly once
    std::vector<uint8_t> mark(S, 0);
    for (size_t s = 0; s < S; s++) {
        const uint64_t t = h_sigma[s];
        if (t >= S || mark[t]) return fail(ctx, ZK_ERR_INVALID, "%s: sigma is not a permutation of the %zu wire slots (entry %zu)", name, S, s);
        mark[t] = 1;
    }
    // the advice codes: every one known.  A plan whose codes are all zero is a plan without advice
    bool advice = false;
    if (h_advice) {
        size_t bad = 0, first = N;
        for (size_t x = 0; x < N; x++) {
            if (!advice_code_known(h_advice[x]) && !bad++) first = x;
            advice |= h_advice[x] != 0;
        }
        if (bad) return fail(ctx, ZK_ERR_INVALID, "%s: %zu of %zu advice codes are unknown; the first is row %zu", name, bad, N, first);
    }
    // the gate-computing rows: all of them, or those with a non-zero output selector
    std::vector<uint8_t> comp(N, 1);
    std::vector<uint64_t> qo;
    if (d_out_sel) {
        qo.resize(4 * N);
        ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));  // the selector may have been produced on the ctx stream
        ZK_HIP(ctx, hipMemcpy(qo.data(), d_out_sel, 32 * N, hipMemcpyDeviceToHost));
        // fully reduced limbs only: r stored as it stands is zero mod r with non-zero limbs, a computing row with a zero denominator
        uint64_t r[4];
        for (int i = 0; i < 4; i++) r[i] = ((uint64_t)FrCfg::P(2 * i + 1) << 32) | FrCfg::P(2 * i);
        for (size_t x = 0; x < N; x++) {
            const uint64_t* q = &qo[4 * x];
            int i = 3;
            while (i > 0 && q[i] == r[i]) i--;
            if (q[i] >= r[i]) return fail(ctx, ZK_ERR_INVALID, "%s: the output selector of row %zu is not reduced below r", name, x);
            comp[x] = (q[0] | q[1] | q[2] | q[3]) != 0;
        }
    }
    const std::vector<uint8_t> gate_comp = comp;
    zk_witness_plan* plan = new zk_witness_plan;
    PlanGuard guard{plan};
    plan->ctx = ctx, plan->N = N;
    // a lookup plan: qk holds only 0 and the Montgomery 1; the key table; the lookup-computing rows (kind 2 in comp)
    if (d_qk) {
        std::vector<uint64_t> qk(4 * N);
        ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        ZK_HIP(ctx, hipMemcpy(qk.data(), d_qk, 32 * N, hipMemcpyDeviceToHost));
        uint64_t one[4];
        for (int i = 0; i < 4; i++) one[i] = ((uint64_t)FrCfg::ONE(2 * i + 1) << 32) | FrCfg::ONE(2 * i);
        size_t bad = 0, first = N;
        for (size_t x = 0; x < N; x++) {
            const uint64_t* q = &qk[4 * x];
            const bool is1 = !memcmp(q, one, 32);
            if (!is1 && (q[0] | q[1] | q[2] | q[3])) {
                if (!bad++) first = x;
            } else if (is1 && !comp[x]) {
                comp[x] = 2;
            }
        }
        if (bad) return fail(ctx, ZK_ERR_INVALID, "%s: %zu of %zu entries of qk are neither 0 nor 1; the first is row %zu", name, bad, N, first);
        const long force = tuning().find_force_slot;
        if (force < -1) return fail(ctx, ZK_ERR_INVALID, "find_force_slot must be -1 or a slot number");
        plan->lookup = true, plan->force = force;
        ZK_HIP(ctx, device_alloc(ctx, (void**)&plan->d_slots, 2 * N * sizeof(uint32_t)));
        const int rc = witness_key_table(ctx, name, d_t, N, force, plan->d_slots);
        if (rc != ZK_OK) return rc;
    }
    // an advice row computes by its code alone: neither by the gate nor by the table (kind 3 in comp)
    if (advice) {
        size_t bad = 0, first = N;
        for (size_t x = 0; x < N; x++) {
            if (!h_advice[x]) continue;
            if (comp[x] && !bad++) first = x;
            comp[x] = 3;
        }
        if (bad) return fail(ctx, ZK_ERR_INVALID, "%s: %zu of %zu advice rows also compute by the gate or the table; the first is row %zu", name, bad, N, first);
    }
    // 1. the cycles.  Slots are visited in ascending order, so a cycle is entered at its smallest slot
    std::vector<uint32_t> src(S);
    std::fill(mark.begin(), mark.end(), 0);
    for (size_t s = 0; s < S; s++) {
        if (mark[s]) continue;
        size_t best = S, t = s;
        do {
            if (t >= 2 * N && comp[t - 2 * N] && t < best) best = t;
            t = (size_t)h_sigma[t];
        } while (t != s);
        const uint32_t v = best < S ? (uint32_t)(best - 2 * N) : (kWitFree | (uint32_t)s);
        do {
            src[t] = v, mark[t] = 1;
            t = (size_t)h_sigma[t];
        } while (t != s);
    }
    // 2. levels.  A computing row x waits for the source rows of its a and b slots (an edge each, also when both are one row)
    std::vector<uint32_t> start(N + 1, 0), level(N, 0);
    std::vector<uint8_t> indeg(N, 0);
    size_t nc = 0;
    for (size_t x = 0; x < N; x++) {
        if (!comp[x]) continue;
        nc++;
        for (int j = 0; j < 2; j++) {
            const uint32_t v = src[j * N + x];
            if (!(v & kWitFree)) start[v + 1]++, indeg[x]++;
        }
    }
    for (size_t r = 0; r < N; r++) start[r + 1] += start[r];
    std::vector<uint32_t> adj(start[N]), fill(start.begin(), start.end() - 1);
    for (size_t x = 0; x < N; x++) {
        if (!comp[x]) continue;
        for (int j = 0; j < 2; j++) {
            const uint32_t v = src[j * N + x];
            if (!(v & kWitFree)) adj[fill[v]++] = (uint32_t)x;
        }
    }
    std::vector<uint32_t> queue;
    queue.reserve(nc);
    for (size_t x = 0; x < N; x++)
        if (comp[x] && !indeg[x]) queue.push_back((uint32_t)x);
    uint32_t top = 0;
    for (size_t head = 0; head < queue.size(); head++) {
        const uint32_t r = queue[head];
        top = std::max(top, level[r]);
        for (uint32_t e = start[r]; e < start[r + 1]; e++) {
            const uint32_t x = adj[e];
            level[x] = std::max(level[x], level[r] + 1);
            if (--indeg[x] == 0) queue.push_back(x);
        }
    }
    if (queue.size() < nc) {
        size_t first = N;
        for (size_t x = 0; x < N && first == N; x++)
            if (comp[x] && indeg[x]) first = x;
        return fail(ctx, ZK_ERR_INVALID, "%s: %zu of %zu rows depend on their own output; the first is row %zu", name, nc - queue.size(), N, first);
    }
    // 3. (level, row) order by a counting sort -- (level, advice or not, row) on an advice plan; the rows that compute nothing follow in
    // ascending order
    plan->computing = nc;
    const size_t levels = nc ? (size_t)top + 1 : 0;
    plan->levels = levels;
    std::vector<uint32_t>& lvoff = plan->lvoff;
    lvoff.assign(levels + 1, 0);
    for (size_t x = 0; x < N; x++)
        if (comp[x]) lvoff[level[x] + 1]++;
    for (size_t v = 0; v < levels; v++) {
        plan->max_level_rows = std::max<size_t>(plan->max_level_rows, lvoff[v + 1]);
        lvoff[v + 1] += lvoff[v];
    }
    std::vector<uint32_t> order(N), at(lvoff.begin(), lvoff.end() - (levels ? 1 : 0));
    std::vector<uint32_t> at_adv;  // where the advice rows of a level begin: after its other rows
    if (advice) {
        at_adv.assign(lvoff.begin() + 1, lvoff.end());
        for (size_t x = 0; x < N; x++)
            if (comp[x] == 3) at_adv[level[x]]--;
    }
    size_t rest = nc;
    for (size_t x = 0; x < N; x++) {
        if (comp[x] == 3) order[at_adv[level[x]]++] = (uint32_t)x | kWitAdvice;
        else if (comp[x]) order[at[level[x]]++] = (uint32_t)x | (comp[x] == 2 ? kWitLookup : 0);
        else order[rest++] = (uint32_t)x;
    }
    for (size_t v = 0; v < levels;) {
        size_t e = v + 1;
        const bool grid = lvoff[v + 1] - lvoff[v] > (uint32_t)kWitBlock;
        if (!grid)
            while (e < levels && lvoff[e + 1] - lvoff[e] <= (uint32_t)kWitBlock) e++;
        plan->launches.push_back({(uint32_t)v, (uint32_t)e, grid});
        v = e;
    }
    // 4. uploads
    int rc = upload_u32(ctx, src, &plan->d_src);
    if (rc == ZK_OK) rc = upload_u32(ctx, order, &plan->d_order);
    if (rc == ZK_OK) rc = upload_u32(ctx, lvoff, &plan->d_lvoff);
    if (rc != ZK_OK) return rc;
    if (advice) {
        ZK_HIP(ctx, device_alloc(ctx, (void**)&plan->d_advice, N * sizeof(uint32_t)));
        ZK_HIP(ctx, hipMemcpy(plan->d_advice, h_advice, N * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    if (d_out_sel) {
        // 1 / qO by the batch inversion: numerator 1 and denominator qO on the gate-computing rows, 0 / 1 elsewhere (no zero denominator)
        uint64_t one[4];
        for (int i = 0; i < 4; i++) one[i] = ((uint64_t)FrCfg::ONE(2 * i + 1) << 32) | FrCfg::ONE(2 * i);
        std::vector<uint64_t> num(4 * N, 0);
        for (size_t x = 0; x < N; x++) {
            if (gate_comp[x]) memcpy(&num[4 * x], one, 32);
            else memcpy(&qo[4 * x], one, 32);
        }
        DevGuard d_num, d_den;
        ZK_HIP(ctx, device_alloc(ctx, &d_num.p, 32 * N));
        ZK_HIP(ctx, device_alloc(ctx, &d_den.p, 32 * N));
        ZK_HIP(ctx, device_alloc(ctx, &plan->d_inv, 32 * N));
        ZK_HIP(ctx, hipMemcpy(d_num.p, num.data(), 32 * N, hipMemcpyHostToDevice));
        ZK_HIP(ctx, hipMemcpy(d_den.p, qo.data(), 32 * N, hipMemcpyHostToDevice));
        rc = fr_batch_div(ctx, d_num.p, d_den.p, plan->d_inv, N);  // blocking
        if (rc != ZK_OK) return rc;
    }
    guard.p = nullptr;
    *out = plan;
    return ZK_OK;
}

}  // namespace zk
