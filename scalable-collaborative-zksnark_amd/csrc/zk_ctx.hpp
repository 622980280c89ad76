// zk_ctx.hpp -- per-GPU context shared by the libzkhip translation units (host side).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/zkhip.h"
#include "../../include/zkhip_test.h"  // (the zk_dbg_* hooks are defined in this library too)

struct zk_msm_job;  // zk_msm.hip

struct zk_srs {
    void* d_bases = nullptr;  // packed 96-B affine points (x||y Montgomery, x=y=0: infinity)
    size_t n = 0;
    bool owned = true;
    bool g2 = false;  // points of G2 (192-byte affine records over Fq2, no endomorphism copies)
    // optional precomputed table: copy w of point i = 2^{bit_offset(w)} * P_i at d_table[w * table_stride + i]
    void* d_table = nullptr;
    int table_c = 0;
    size_t table_stride = 0;
    size_t table_rec = 96;  // bytes per record of d_table (G1: 96 packed, or 128 = one record per line; G2: 192)
};

struct zk_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = true;
    std::string err;
    // growable device scratch arenas (never shrunk; freed with the ctx)
    struct Arena {
        void* p = nullptr;
        size_t cap = 0;
    };
    Arena scratch[12];
    void* h_pinned = nullptr;  // pinned host staging
    size_t h_pinned_cap = 0;
    int msm_window_override = 0;
    float msm_ms[6] = {0, 0, 0, 0, 0, 0};
    float sc_ms[2] = {0, 0};  // tuning sc_ts = 3: device time of the first stage / of all launches of the last sumcheck-family call
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    static constexpr int kAux = 6;    // extra streams for independent MSM window classes of one batch
    static constexpr int kParts = 4;  // staggered parts of one MSM class (zk_msm.hip)
    // where one MSM batch runs: lane 0 = the ctx stream (blocking calls), lanes 1..2 = the asynchronous jobs
    // (zk_msm_g1_batch_async), which alternate between two sets of streams so that the latency-bound tail of one job
    // overlaps with the sort and the accumulation of the next.  Streams / events of the async lanes are created on first use.
    struct MsmLane {
        hipStream_t main = nullptr;
        hipStream_t aux[kAux] = {};
        hipEvent_t ev_fork = nullptr, ev_join[kAux] = {}, ev_part[kParts] = {};
        std::vector<hipEvent_t> ev_cls;  // completion event per MSM window class of a batch
        std::vector<hipEvent_t> ev_sort;  // end of the sort phase per class: the classes of a batch share ONE level-1 scratch region (zk_msm.hip)
        bool ready = false;
        // async lanes: growable arenas and pinned staging of their own (kept between jobs, like the ctx's scratch), and
        // whether a job currently owns the lane
        Arena mem[10];
        void* pinned = nullptr;
        size_t pinned_cap = 0;
        bool busy = false;
    };
    static constexpr int kLanes = 4;  // lane 0 + up to three asynchronous jobs in flight
    MsmLane lanes[kLanes];
    hipEvent_t ev_async_in = nullptr;  // ctx stream -> job stream: the scalars of a job are produced on the ctx stream
    void* host_pool = nullptr;       // worker threads for the per-item host chains (zk_msm.hip)
    // zk_malloc / zk_free block recycling (zk_api.cpp)
    std::unordered_map<size_t, std::vector<void*>> pool_free;
    std::unordered_map<void*, size_t> pool_size;
    size_t pool_bytes = 0;
    std::mutex pool_mu;  // a garbage collector may release buffers from another thread
    int cu_count = 256;
    bool multi_lds_raised = false;   // zk_batchopen.hip: k_multi_local's dynamic LDS limit has been raised on this ctx's device
    // the same for the local kernels of the fused identities, indexed by the Kind's kSlot (zk_gate.cuh; slot 2 of fs_lds_raised is the
    // batch opening's k_multi_fs_local): k_sc_local<K> of the preset-challenge engine (zk_fused.cuh), k_fs_local<K> of zk_fs.hip
    bool preset_lds_raised[7] = {false, false, false, false, false, false, false};
    bool fs_lds_raised[7] = {false, false, false, false, false, false, false};
    // party exchanges (zk_comm.cpp): an RCCL communicator bound to this ctx's GPU
    void* comm = nullptr;
    int comm_rank = 0, comm_world = 1;
    void* h_comm = nullptr;  // pinned staging of zk_d_msm (its own block: the MSM pass may re-allocate h_pinned)
    size_t h_comm_cap = 0;
};

// Fiat-Shamir transcript (zk_transcript.hip): the 32-byte state of the hash chain in device memory, bound to one ctx
struct zk_transcript {
    zk_ctx* ctx = nullptr;
    uint32_t* d_state = nullptr;
    // staging of host strings too long for a kernel argument: pinned block, device block, "the copy out of it is done"
    unsigned char* h_stage = nullptr;
    unsigned char* d_stage = nullptr;
    size_t stage_cap = 0;
    hipEvent_t staged = nullptr;
    bool stage_busy = false;
};

// Witness plan of one Plonk circuit (zk_witness.cpp builds it on the host, zk_witness.hip runs it): see include/zkhip.h
struct zk_witness_plan {
    zk_ctx* ctx = nullptr;
    size_t N = 0;
    uint32_t* d_src = nullptr;    // 3N: the source of every slot -- a row (its c slot holds the class's value), or kWitFree | the class's smallest slot
    uint32_t* d_order = nullptr;  // N: the computing rows by (level, row), then the other rows in ascending order
    uint32_t* d_lvoff = nullptr;  // levels + 1: level v is order[lvoff[v] .. lvoff[v + 1])
    void* d_inv = nullptr;        // N Fr: 1 / qO on the gate-computing rows, 0 elsewhere (null: built without an output selector, every row computes)
    // a lookup plan (zk_witness_plan_create_lookup): the key table of (t0, t1) -- 2N u32 slots of the protocol of zk_find.cuh, built once on
    // the device -- and the start slot its walks were built with (the knob find_force_slot at creation; every later walk must use the same).
    // The lookup-computing rows carry kWitLookup in their d_order entry.
    uint32_t* d_slots = nullptr;
    long force = -1;
    bool lookup = false;
    // an advice plan (zk_witness_plan_create_advice with a non-zero code): the plan's own copy of the N codes; the advice-computing rows
    // carry kWitAdvice in their d_order entry and stand AFTER the other rows of their level.  Null: the plan has no advice row.
    uint32_t* d_advice = nullptr;
    size_t computing = 0, levels = 0, max_level_rows = 0;
    struct Launch {
        uint32_t lv0, lv1;  // the levels [lv0, lv1): ONE level of more than kWitBlock rows (a grid of workgroups), or a run of levels of at most kWitBlock rows each (one workgroup)
        bool grid;
    };
    std::vector<Launch> launches;
    std::vector<uint32_t> lvoff;  // host copy of d_lvoff
};

namespace zk {

static constexpr uint32_t kWitFree = 0x80000000u;  // flag of zk_witness_plan::d_src (3N <= 3 * 2^29 stays below it)
static constexpr uint32_t kWitLookup = 0x80000000u;  // flag of zk_witness_plan::d_order: a lookup-computing row (N <= 2^29 stays below it)
static constexpr uint32_t kWitAdvice = 0x40000000u;  // flag of zk_witness_plan::d_order: an advice-computing row (N <= 2^29 leaves bit 30 free)
static constexpr int kWitBlock = 256;

// Experiment / diagnostics knobs of the whole library in ONE place.  Defaults are the shipped configuration; the only
// ways to change them are zk_dbg_tune(key, value) (tests, tools) and the ZKHIP_TUNE="key=value,key=value" environment
// variable, read once by zk::tuning() (zk_api.cpp) -- no other getenv in the product code.
struct Tuning {
    // sumcheck family (zk_fr.hip)
    long sc_pass_wg = 0;      // workgroups per CU of the HBM passes (0: 2 product / 4 others)
    long sc_local_g = 256;    // workgroups of a local stage
    long sc_local_threads = 1024;  // threads of a local-stage workgroup, 1024 or 256 (any other value: the call is refused; 256: fits beside two accumulation workgroups of an MSM pass -- EXPERIMENT, profiles/r06q)
    long sc_ts = 0;           // 1: in-kernel stage timestamps of the local launches on stderr, 2: host-side phases, 3: HIP events (zk_sumcheck_last_timing)
    long sc_xcd = 1;          // XCD-aware slice map of the local stages
    long sc_kf = 4;           // rounds per flat fold pass (0: round-by-round passes)
    long sc_plain_flat = 1;   // plain sumcheck passes in flat form
    long sc_kp = 2;           // rounds per product pass
    long sc_k0 = 3;           // rounds per single-table pass
    long sc_flat_wg = 64;     // workgroups per CU, flat fold
    long sc_plain_wg = 3;     // workgroups per CU, flat plain pass
    long sc_pre = 1;          // first round of a full-size local stage straight out of the table
    long sc_pinned_out = 1;   // results written straight into pinned host memory
    long sc_handover = 1;     // the pass before a multi-workgroup local stage stores that stage's slices contiguously
    long sc_t1_device = 0;    // TEST SWITCH: t1 = sum f_hi g_hi of EVERY round computed on the device (never derived)
    // gate sumcheck (zk_gate.hip)
    long gate_local_e = 512;  // longest table (elements, a power of two <= 512) the single-workgroup LDS stage takes over; 1: HBM passes down to the last element
    long gate_pass_wg = 0;    // workgroups per CU of the HBM passes (0: 2)
    // wiring sumcheck (zk_wiring.hip)
    long wiring_local_e = 512;  // longest table (elements, a power of two <= 512) the single-workgroup LDS stage takes over; 1: HBM passes down to the last element
    long wiring_pass_wg = 0;    // workgroups per CU of the HBM passes (0: 2)
    // batch-opening sumcheck (zk_batchopen.hip)
    long multi_local_e = 512;   // longest table (elements, a power of two <= 512) the single-workgroup LDS stage takes over when the 2 count tables fit; 1: HBM passes down to the last element
    long multi_pass_wg = 0;     // workgroups per CU of the HBM passes (0: 4)
    // three-column wiring sumcheck (zk_perm3.hip)
    long perm3_local_e = 256;   // longest table (elements, a power of two <= 256: eleven tables of 512 would be 176 KiB of LDS) the single-workgroup LDS stage takes over; 1: HBM passes down to the last element
    // wide gate sumcheck (zk_gatew.hip)
    long gatew_local_e = 256;   // longest table (elements, a power of two <= 256: eleven tables of 512 would be 176 KiB of LDS) the single-workgroup LDS stage takes over; 1: HBM passes down to the last element
    // lookup sumcheck (zk_lookup.hip)
    long lookup_local_e = 512;  // longest table (elements, a power of two <= 512) the single-workgroup LDS stage takes over; 1: HBM passes down to the last element
    // selector-gated lookup sumcheck (zk_lookup3.hip)
    long lookupsel_local_e = 512;  // longest table (elements, a power of two <= 512: seven tables are 112 KiB of LDS) the single-workgroup LDS stage takes over; 1: HBM passes down to the last element
    // lookup find (zk_lookup_find.hip)
    long find_force_slot = -1;  // TEST SWITCH: v >= 0 starts the walk of EVERY key at slot v mod slots (one collision chain; near the end of the array it wraps); -1: the hash
    // MSM (zk_msm.hip)
    long msm_table_dc = 0;    // window-table width delta (sweeps)
    long msm_qstep = 2;       // window-class quantisation step of batches
    long msm_tile = 0;        // sorted entries per lane of k_accum_tiles (0: auto)
    long msm_pair = 0;        // k_finish pairs the planes
    long msm_fixq = 65536;    // buckets per class up to which the fix-up runs on quads
    long msm_quad = 32768;    // additions per reduction pass up to which a quad of lanes shares one
    long msm_stage = -1;      // level-1 scatter through LDS (-1: by row length)
    long msm_split = 1;       // staggered parts of the largest class
    long msm_np = 0;          // sort partitions per row (0: auto)
    long msm_fused_min = 0;   // window-table rows of >= 2^k entries are partitioned straight from the scalars (0: k = 23; -1: never -- the round-5 path)
    long msm_share_l1 = 1;    // the classes of a batch share one level-1 sort scratch (their sort phases run in sequence; 0: a region per class)
    long msm_idx_ahead = 1;   // k_accum_tiles: the sorted index of the entry after next is fetched one iteration early (0: the round-5 loop)
    long msm_tab_spt = 0;     // fused level 1: 1 forces one scalar per thread (A/B)
    long msm_l2_tiled = 0;    // level 2 in LDS-staged tiles for partitions of >= this many entries (0: 8192, rows of >= 2^23 entries; -1: never)
    long msm_debug = 0;       // class geometry on stderr
    long msm_serial = 0;      // all classes on the ctx stream
    long msm_size_classes = 1;  // window-table items: one class per power-of-two length
    long srs_table_batched = 1;  // G1 window tables: normalise with Montgomery's trick (one inversion per 64 records; 0: one per record, the round-5 kernel)
    long srs_table_rec = 0;   // G1 window tables built from now on: bytes per record (0: by free memory, see srs_precompute | 96: packed | 128: one record per 128-B line -- faster gathers, +33 % table memory)
    long msm_size_class_min = 16;  // window-table items of up to 2^k points (and one table width) share one size class: fewer launch chains for the short items of a batch
    long msm_small_table_widths = 1;  // zk_srs_precompute's own pick: 12 bits up to 2^10 points, 14 bits for 2^11 .. 2^14 (0: log2 n + 2)
    long msm_share = 100;     // EXPERIMENT (profiles/r05g): percent of the resident workgroup slots k_accum_tiles may fill (persistent grid below 100)
    // SRS / PSS maps on points (zk_srs.hip)
    long g1_map_by_column = 1;  // zk_g1_apply_matrix: one lane per (output, column) when there are few outputs of many terms (0: always one lane per output)
    // parameter sets from a file (zk_srsio.hip)
    long srsio_max_blocks = 0;  // TEST SWITCH: v > 0 caps the grid of zk_g1_decompress_check_device at v workgroups of 64 lanes, so that a few hundred points walk the grid-stride loop (0: 2048)
    // Poseidon Merkle tree (zk_poseidon.hip)
    long poseidon_tail_nodes = 256;  // a level of more nodes than this is a launch of its own; all levels at or below it are ONE launch of one workgroup (< 1: every level its own launch)
};
Tuning& tuning();
int tune_set(const char* key, long value);  // 0, or ZK_ERR_INVALID for an unknown key

int fail(zk_ctx* ctx, int code, const char* fmt, ...);
int hip_fail(zk_ctx* ctx, hipError_t e, const char* what);
// returns device scratch of at least `bytes` (slot 0..7), or nullptr after recording the error
void* scratch(zk_ctx* ctx, int slot, size_t bytes);
void* pinned(zk_ctx* ctx, size_t bytes);
// hipMalloc that drops the ctx's parked zk_free blocks and retries once on out-of-memory
hipError_t device_alloc(zk_ctx* ctx, void** out, size_t bytes, bool pool_locked = false);
size_t pool_trim(zk_ctx* ctx);
int msm_lanes_reserve(zk_ctx* ctx, int lane, const uint64_t* caps10, uint64_t pinned_cap);  // zk_msm.hip: grow an asynchronous lane's arenas

#define ZK_HIP(ctx, call)                                            \
    do {                                                             \
        hipError_t _e = (call);                                      \
        if (_e != hipSuccess) return zk::hip_fail(ctx, _e, #call);   \
    } while (0)

// ---- zk_fr.hip ----
int fr_binary(zk_ctx* ctx, int op, const void* a, const void* b, void* out, size_t n);
int fr_axpb(zk_ctx* ctx, const void* a, const void* b, const uint64_t* alpha, const uint64_t* beta, void* out, size_t n);
int fr_apply_matrix(zk_ctx* ctx, const uint64_t* h_matrix, size_t rows, size_t cols, const void* d_in, size_t isv, size_t isc,
                    void* d_out, size_t osv, size_t osr, size_t k);
int fr_ntt_map(zk_ctx* ctx, size_t A, const uint64_t* h_winv, size_t B, const uint64_t* h_w, const uint64_t* h_scale, size_t nin, size_t take,
               size_t step, const void* d_in, size_t isv, size_t isc, void* d_out, size_t osv, size_t osr, size_t k);
int fr_deinterleave(zk_ctx* ctx, const void* t, void* even, void* odd, size_t n);
int fr_batch_div(zk_ctx* ctx, const void* num, const void* den, void* out, size_t n);
// mode 0 plain sums, 1 product sums, 2 fold only, 3 open quotients
int multilinear_run(zk_ctx* ctx, int mode, const void* d_f, const void* d_g, size_t len, const uint64_t* h_chal,
                    size_t rounds, uint64_t* h_sums, uint64_t* h_last_f, uint64_t* h_last_g, void* d_out, void* d_q);
int multilinear_batch(zk_ctx* ctx, const zk_sc_item* items, size_t count);
int product_tree(zk_ctx* ctx, const void* d_x, size_t N, void* d_tree);
// sums: rounds x (t0, t1, t2) Montgomery Fr on the host; t1 of round 0 is the device's, every later one is derived from the round before
void derive_t1(uint64_t* sums, const uint64_t* chal, size_t rounds);
int dbg_fq(zk_ctx* ctx, int op, const void* a, const void* b, void* out, size_t n);

// ---- zk_gate.hip ----
int eq_table(zk_ctx* ctx, const uint64_t* h_point, size_t n, void* d_out);
int eq_table_seeded(zk_ctx* ctx, const uint64_t* h_point, size_t n, const uint64_t* h_seed, void* d_out);  // out[x] = seed * eq(point, x)
// d_tabs: eq, q1, q2, a, b, c, in
int sumcheck_gate(zk_ctx* ctx, const void* const* d_tabs, size_t len, const uint64_t* h_chal, uint64_t* h_out_evals, uint64_t* h_last);

// ---- zk_wiring.hip ----
// d_tree: the 2N Fr of product_tree; h_last: eq, v1x, vx0, vx1, h, num, den
int sumcheck_wiring(zk_ctx* ctx, const void* d_eq, const void* d_tree, const void* d_num, const void* d_den, size_t N, const uint64_t* h_gamma,
                    const uint64_t* h_chal, uint64_t* h_out_evals, uint64_t* h_last);

// ---- zk_perm3.hip ----
// d_w, d_ssigma, d_num, d_den: three tables of N Fr each; d_P = n_0 n_1 n_2, d_Q = d_0 d_1 d_2
int perm3_terms(zk_ctx* ctx, const void* const* d_w, const void* const* d_ssigma, size_t N, const uint64_t* h_alpha, const uint64_t* h_beta, void* const* d_num,
                void* const* d_den, void* d_P, void* d_Q);
// h_out_evals: mu x 6 Fr; h_last: eq, v1x, vx0, vx1, h, n_0, n_1, n_2, d_0, d_1, d_2
int sumcheck_perm3(zk_ctx* ctx, const void* d_eq, const void* d_tree, const void* const* d_num, const void* const* d_den, size_t N, const uint64_t* h_gamma,
                   const uint64_t* h_chal, uint64_t* h_out_evals, uint64_t* h_last);

// ---- zk_gatew.hip ----
// d_tabs: eq, qL, qR, qM, qO, qC, qH, a, b, c, in; h_out_evals: rounds x 8 Fr; h_last: the eleven remaining elements in that order
int sumcheck_gate_wide(zk_ctx* ctx, const void* const* d_tabs, size_t len, const uint64_t* h_chal, uint64_t* h_out_evals, uint64_t* h_last);

// ---- zk_lookup.hip ----
int lookup_multiplicities(zk_ctx* ctx, const void* d_f, const void* d_t, const uint32_t* d_idx, size_t N, void* d_m);
int lookup_write_counts(zk_ctx* ctx, const uint32_t* d_cnt, size_t N, void* d_m);  // k_lookup_write on the ctx stream: N u32 counters -> N Montgomery Fr
// d_tabs, h_last: E, df, dt, m, hf, ht; h_out_evals: rounds x 4 Fr
int sumcheck_lookup(zk_ctx* ctx, const void* const* d_tabs, size_t len, const uint64_t* h_gamma, const uint64_t* h_chal, uint64_t* h_out_evals, uint64_t* h_last);

// ---- zk_lookup3.hip ----
// d_w: a, b, c; d_t: t0, t1, t2 (N Fr each); d_qk: the selector; m[y] = #{x : qk(x) = 1, idx[x] = y}
int lookup3_multiplicities(zk_ctx* ctx, const void* const* d_w, const void* const* d_t, const void* d_qk, const uint32_t* d_idx, size_t N, void* d_m);
int lookup3_terms(zk_ctx* ctx, const void* const* d_w, const void* const* d_t, size_t N, const uint64_t* h_zeta, const uint64_t* h_beta, void* d_df, void* d_dt);
// d_tabs, h_last: E, df, dt, m, hf, ht, qk; h_out_evals: rounds x 4 Fr
int sumcheck_lookup_sel(zk_ctx* ctx, const void* const* d_tabs, size_t len, const uint64_t* h_gamma, const uint64_t* h_chal, uint64_t* h_out_evals, uint64_t* h_last);

// ---- zk_lookup_find.hip ----
// the row-to-table indices found on the device (smallest index of an equal entry) and their multiplicities; d_idx or d_m may be null, not both
int lookup_find(zk_ctx* ctx, const void* d_f, const void* d_t, size_t N, uint32_t* d_idx, void* d_m);
int lookup3_find(zk_ctx* ctx, const void* const* d_w, const void* const* d_t, const void* d_qk, size_t N, uint32_t* d_idx, void* d_m);

// ---- zk_witness.cpp (the plan, on the host) / zk_witness.hip (the kernels) ----
// d_qk, d_t: null (a plain plan), or the lookup selector and t0, t1, t2 (a lookup plan); h_advice: null, or the N advice codes (name: the
// export the messages name)
int witness_plan_create(zk_ctx* ctx, const char* name, const uint64_t* h_sigma, const void* d_out_sel, const void* d_qk, const void* const* d_t, const uint32_t* h_advice,
                        size_t N, zk_witness_plan** out);
// zk_witness.hip: the slots of a lookup plan's key table built from (t0, t1) with the start slot `force`, then every entry's t2 compared
// with the t2 of the first entry of its pair (blocking; the function rule of include/zkhip.h)
int witness_key_table(zk_ctx* ctx, const char* name, const void* const* d_t, size_t N, long force, uint32_t* d_slots);
void witness_plan_free(zk_witness_plan* plan);
// d_qk, d_t: null on a plain plan; the selector and the tables the plan was built from on a lookup plan
int plonk_witness(zk_ctx* ctx, const zk_witness_plan* plan, int gate_kind, const void* const* d_sel, const void* d_qk, const void* const* d_t, const uint64_t* h_pi, size_t l,
                  const void* d_free, void* d_a, void* d_b, void* d_c);
// h_bad: bad gate rows, the smallest (~0: none), bad copies, the smallest (~0: none) and, on a lookup plan, bad lookups, the smallest (~0: none)
int plonk_witness_check(zk_ctx* ctx, const zk_witness_plan* plan, int gate_kind, const void* const* d_sel, const void* d_qk, const void* const* d_t, const uint64_t* h_pi,
                        size_t l, const void* d_a, const void* d_b, const void* d_c, uint64_t* h_bad);

// ---- zk_batchopen.hip ----
int eq_table_acc(zk_ctx* ctx, const uint64_t* h_point, size_t n, const uint64_t* h_weight, void* d_acc);
int fr_lincomb(zk_ctx* ctx, size_t count, const void* const* d_tabs, const uint64_t* h_coeffs, size_t len, void* d_out);
int sumcheck_multi(zk_ctx* ctx, size_t count, const void* const* d_e, const void* const* d_f, size_t len, const uint64_t* h_chal,
                   uint64_t* h_out_triples, uint64_t* h_last_e, uint64_t* h_last_f);

// ---- zk_transcript.hip ----
int transcript_create(zk_ctx* ctx, const void* h_label, size_t label_len, zk_transcript** out);
void transcript_free(zk_transcript* t);
int transcript_absorb(zk_ctx* ctx, zk_transcript* t, const void* h_bytes, size_t len);
int transcript_absorb_device(zk_ctx* ctx, zk_transcript* t, const void* d_ptr, size_t len);
int transcript_challenges(zk_ctx* ctx, zk_transcript* t, size_t count, uint64_t* h_out);
int transcript_state(zk_ctx* ctx, zk_transcript* t, uint8_t* h_state32);

// ---- zk_fs.hip: the fused sumchecks with their challenges drawn from a transcript on the device ----
// the arguments of sumcheck_gate / sumcheck_wiring / sumcheck_multi with the transcript in the place of h_chal; h_chal_out: rounds Fr
int sumcheck_gate_fs(zk_ctx* ctx, const void* const* d_tabs, size_t len, zk_transcript* t, uint64_t* h_out_evals, uint64_t* h_last, uint64_t* h_chal_out);
int sumcheck_wiring_fs(zk_ctx* ctx, const void* d_eq, const void* d_tree, const void* d_num, const void* d_den, size_t N, const uint64_t* h_gamma,
                       zk_transcript* t, uint64_t* h_out_evals, uint64_t* h_last, uint64_t* h_chal_out);
int sumcheck_multi_fs(zk_ctx* ctx, size_t count, const void* const* d_e, const void* const* d_f, size_t len, zk_transcript* t,
                      uint64_t* h_out_triples, uint64_t* h_last_e, uint64_t* h_last_f, uint64_t* h_chal_out);
int sumcheck_perm3_fs(zk_ctx* ctx, const void* d_eq, const void* d_tree, const void* const* d_num, const void* const* d_den, size_t N, const uint64_t* h_gamma,
                      zk_transcript* t, uint64_t* h_out_evals, uint64_t* h_last, uint64_t* h_chal_out);
int sumcheck_gate_wide_fs(zk_ctx* ctx, const void* const* d_tabs, size_t len, zk_transcript* t, uint64_t* h_out_evals, uint64_t* h_last, uint64_t* h_chal_out);
int sumcheck_lookup_fs(zk_ctx* ctx, const void* const* d_tabs, size_t len, const uint64_t* h_gamma, zk_transcript* t, uint64_t* h_out_evals, uint64_t* h_last,
                       uint64_t* h_chal_out);
int sumcheck_lookup_sel_fs(zk_ctx* ctx, const void* const* d_tabs, size_t len, const uint64_t* h_gamma, zk_transcript* t, uint64_t* h_out_evals, uint64_t* h_last,
                           uint64_t* h_chal_out);

// ---- zk_msm.hip ----
struct MsmItem {
    const zk_srs* srs;
    size_t offset;
    const void* d_scalars;
    size_t n;
};
int msm_g1_batch(zk_ctx* ctx, const MsmItem* items, size_t count, uint64_t* h_out);
// asynchronous form: enqueue on one of the ctx's job lanes and return; msm_job_wait runs the host chains, writes the
// results (18 u64 per item) and releases the job.  The scalars must stay valid until then.
int msm_g1_batch_async(zk_ctx* ctx, const MsmItem* items, size_t count, zk_msm_job** job);
int msm_job_wait(zk_ctx* ctx, zk_msm_job* job, uint64_t* h_out);
void msm_lanes_destroy(zk_ctx* ctx);
int msm_g2_batch(zk_ctx* ctx, const MsmItem* items, size_t count, uint64_t* h_out);  // h_out: 36 u64 per item
int srs_pack_g2(zk_ctx* ctx, const void* h_bases, size_t stride, size_t n, zk_srs** out);
int msm_g1(zk_ctx* ctx, const zk_srs* srs, size_t offset, const void* d_scalars, size_t n, uint64_t* h_out);
int srs_pack(zk_ctx* ctx, const void* h_bases, size_t stride, size_t n, zk_srs** out);
int srs_precompute(zk_ctx* ctx, zk_srs* srs, int c, int record_bytes);  // record_bytes 0: the default (tuning knob srs_table_rec)
void msm_host_pool_destroy(zk_ctx* ctx);
int srs_from_device(zk_ctx* ctx, const void* d_bases96, size_t n, zk_srs** out);
int srs_download(zk_ctx* ctx, const zk_srs* srs, void* h_out96);
int srs_generate(zk_ctx* ctx, const uint64_t* k0, const uint64_t* k1, size_t n, zk_srs** out);
// ---- zk_srs.hip ----
int srs_powers(zk_ctx* ctx, const void* h_g96, const uint64_t* h_s, size_t nvars, zk_srs** out_levels);
int srs_to_packed(zk_ctx* ctx, const zk_srs* level, const uint64_t* h_row, size_t l, zk_srs** out);
int g1_apply_matrix_ref(zk_ctx* ctx, const uint64_t* h_matrix, size_t rows, size_t cols, const void* d_in, size_t isv, size_t isc, void* d_out,
                        size_t osv, size_t osr, size_t k);
int dbg_g1_op(zk_ctx* ctx, int mode, const void* p, const void* q, void* h_out, size_t n);
int dbg_g2_op(zk_ctx* ctx, int mode, const void* p, const void* q, void* h_out, size_t n);
int dbg_xyzz_op(zk_ctx* ctx, int mode, const void* d_a, const void* d_lift_a, const void* d_b, const void* d_lift_b, const void* d_rep,
                void* d_out, size_t n);
int dbg_xyzz2_op(zk_ctx* ctx, int mode, const void* d_a, const void* d_lift_a, const void* d_b, const void* d_lift_b, const void* d_rep,
                 void* d_out, size_t n);
int msm_pick_window(size_t n);
int g1_lincomb_batch_host(zk_ctx* ctx, const uint64_t* h_points_jac, const uint64_t* h_scalars_canon, size_t n, size_t count,
                          uint64_t* h_out);
int g1_lincomb_host(zk_ctx* ctx, const uint64_t* h_points_jac, const uint64_t* h_scalars_canon, size_t n, uint64_t* h_out);
// ---- zk_pairing.hip ----
int pairing_values(zk_ctx* ctx, size_t count, const void* h_g1, const void* h_g2, size_t g2_stride, uint64_t* h_out);
int pairing_product_check(zk_ctx* ctx, size_t groups, const size_t* h_start, const void* h_g1, const void* h_g2, size_t g2_stride,
                          uint8_t* h_ok);
int pcs_vk_create(zk_ctx* ctx, const void* h_g1_96, const void* h_powers_g2, size_t g2_stride, size_t n_g2, zk_pcs_vk** out);
void pcs_vk_free(zk_pcs_vk* vk);
int pcs_verify_batch(zk_ctx* ctx, const zk_pcs_vk* vk, size_t nvars, size_t count, const uint64_t* h_comm, const uint64_t* h_values,
                     const uint64_t* h_proofs, const uint64_t* h_points, uint8_t* h_ok);
int pcs_agg_weights(size_t count, const size_t* h_nvars, const size_t* h_skip, const size_t* h_cstart, const uint64_t* h_cpoints18,
                    const uint64_t* h_cscalars, const uint64_t* h_values, const uint64_t* h_proofs18, const uint64_t* h_points, uint64_t* h_rho);
int pcs_verify_agg(zk_ctx* ctx, const zk_pcs_vk* vk, size_t count, const size_t* h_nvars, const size_t* h_skip, const size_t* h_cstart,
                   const uint64_t* h_cpoints18, const uint64_t* h_cscalars, const uint64_t* h_values, const uint64_t* h_proofs18,
                   const uint64_t* h_points, const uint64_t* h_rho, uint8_t* h_ok);
// ---- zk_g1check.hip ----
int g1_decompress_check(zk_ctx* ctx, size_t count, const void* h_in48, uint64_t* h_out18, uint8_t* h_status);
int g1_check(zk_ctx* ctx, size_t count, const uint64_t* h_points18, uint8_t* h_status);
// ---- zk_srsio.hip ----
int g1_decompress_check_device(zk_ctx* ctx, size_t count, const void* d_in48, void* d_out96, uint32_t flags, uint64_t* h_result);
int srs_halve(zk_ctx* ctx, const zk_srs* level, zk_srs** out);
int fr_hash_expand(zk_ctx* ctx, const uint8_t* h_seed32, uint32_t domain, size_t n, void* d_out);
int srs_check(zk_ctx* ctx, const zk_srs* const* levels, size_t n, const void* h_powers_g2, size_t g2_stride, const uint8_t* h_seed32, uint8_t* h_ok);
// ---- zk_g2check.hip ----
int g2_decompress_check(zk_ctx* ctx, size_t count, const void* h_in96, uint64_t* h_out24, uint8_t* h_status);
int g2_check(zk_ctx* ctx, size_t count, const void* h_g2, size_t g2_stride, uint8_t* h_status);
// ---- zk_g1seg.hip ----
// h_bad, h_why (optional): the term a ZK_ERR_INVALID names (~0 otherwise) and what is wrong with it
int g1_lincomb_seg(zk_ctx* ctx, size_t segments, const size_t* h_start, const uint64_t* h_points18, const uint64_t* h_scalars, uint64_t* h_out18,
                   size_t* h_bad = nullptr, const char** h_why = nullptr);
// ---- zk_poseidon.hip ----
int poseidon_params_create(zk_ctx* ctx, int rf, int rp, const uint64_t* h_rc, const uint64_t* h_mds, zk_poseidon_params** out);
void poseidon_params_free(zk_poseidon_params* p);
int poseidon_permute(zk_ctx* ctx, const zk_poseidon_params* p, const void* d_in, void* d_out, size_t n);
int poseidon_hash2(zk_ctx* ctx, const zk_poseidon_params* p, const void* d_left, const void* d_right, void* d_out, size_t n);
int poseidon_merkle(zk_ctx* ctx, const zk_poseidon_params* p, const void* d_leaves, size_t n, void* d_tree);
// the tree kept on the device: a gather of paths, the roots of paths, a batch of leaf writes (h_index: host, validated before anything is enqueued)
int poseidon_merkle_paths(zk_ctx* ctx, const void* d_tree, size_t n, const uint64_t* h_index, size_t count, void* d_siblings);
int poseidon_merkle_roots(zk_ctx* ctx, const zk_poseidon_params* p, const void* d_leaves, const uint64_t* h_index, const void* d_siblings, size_t depth, size_t count, void* d_roots);
int poseidon_merkle_update(zk_ctx* ctx, const zk_poseidon_params* p, void* d_tree, size_t n, const uint64_t* h_index, const void* d_values, size_t count);
// ---- zk_jubjub.hip ----
int jubjub_mul(zk_ctx* ctx, const void* d_points, const void* d_scalars, void* d_out, size_t n);
int jubjub_check(zk_ctx* ctx, const void* d_points, uint32_t* d_status, size_t n);
int schnorr_verify(zk_ctx* ctx, const zk_poseidon_params* p, const void* d_pk, const void* d_msg, const void* d_sig, uint32_t* d_status, size_t n);
// ---- zk_pairing.hip: test hooks ----
int dbg_fq30_op(zk_ctx* ctx, int mode, const void* d_x, const void* d_kx, const void* d_y, const void* d_ky, void* d_out, void* d_flags,
                size_t n);
int dbg_fq12_op(zk_ctx* ctx, int mode, const void* d_a, const void* d_b, const void* d_lift, void* d_out, void* d_flags, size_t n);

}  // namespace zk
