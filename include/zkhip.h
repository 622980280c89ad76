/*
 * zkhip.h -- C ABI of libzkhip.so: the MI355X (gfx950) drop-in for the compute loops of the
 * reference's `dist-primitive` crate (LBruyne/Scalable-Collaborative-zkSNARK).
 *
 * The reference has no FFI of its own (it is 100 % Rust on arkworks); these entry points are
 * what a `#[link(name = "zkhip")] extern "C"` block in dist-primitive would bind to replace
 *   - `G::msm(b, s)`                         dist-primitive/src/dmsm.rs:23, dpoly_comm.rs:242,274,457
 *   - the Phase-1 sumcheck loops             dsumcheck.rs:10-21,37-85,107-121,167-219,301-315,377-429
 *   - fold / fix_variable                    mle.rs:62-70,95-103
 *   - the open() quotient+fold loop          dpoly_comm.rs:309-323,337-351,418-432
 *   - the product tree                       dacc_product.rs:31-38,304-313,372-381
 *   - the element-wise Fr steps              hyperplonk/src/dhyperplonk.rs:233-238,251-256,326-339
 * INTEGRATION.md shows the Rust-side binding.
 *
 * Memory layouts are the reference's own, so a Rust caller passes its buffers unchanged:
 *   Fr  : 4 x u64 little-endian limbs, Montgomery form R = 2^256  (ark-ff Fp<MontBackend<_,4>,4>), 32 B
 *   Fq  : 6 x u64 limbs, Montgomery form R = 2^384, 48 B
 *   G1 affine: { x: Fq, y: Fq, infinity: bool }  -- stride 104 as a Rust struct; stride 96
 *              (x||y, with x = y = 0 meaning infinity) is accepted too
 *   G1 projective (results): Jacobian { x, y, z } 3 x 48 B = 144 B, as ark-ec Projective.
 *              Results are returned NORMALISED (z = R mod q, or (1,1,0) for infinity), so
 *              they are bit-comparable and are valid `Projective` values.
 *
 * Conventions: every function returns 0 on success or a negative zk_status; nothing aborts.
 * `d_` pointers are device (HBM) pointers, `h_` pointers are host pointers.  A ctx is bound
 * to one GPU; calls on distinct ctx are thread-safe, calls on one ctx are serialised by the
 * caller.  All work is enqueued on the ctx stream; functions that return host results
 * synchronise that stream before returning.
 */
#ifndef ZKHIP_H
#define ZKHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct zk_ctx zk_ctx;
typedef struct zk_srs zk_srs; /* device-resident base vector(s): one level of powers_of_g */

typedef enum {
    ZK_OK = 0,
    ZK_ERR_INVALID = -1,   /* bad argument (null, not a power of two, ...) : the reference's assert!s */
    ZK_ERR_LENGTH = -2,    /* bases/scalars length mismatch: `msm` -> Err(min_len); see zk_last_error */
    ZK_ERR_HIP = -3,       /* HIP runtime error */
    ZK_ERR_NO_DEVICE = -4, /* no gfx950 device / library built without device code */
    ZK_ERR_DIV_ZERO = -5,  /* zero denominator in zk_fr_batch_div (reference: inverse().unwrap() panic) */
    ZK_ERR_OOM = -6,
    ZK_ERR_COMM = -7,      /* RCCL error / no communicator (reference: MPCNetError) */
    ZK_ERR_INTERNAL = -8   /* an invariant of the library itself does not hold (a bug, never the caller's input) */
} zk_status;

/* ---- context ------------------------------------------------------------------------ */
int zk_ctx_create(int device_id, zk_ctx **out);
void zk_ctx_destroy(zk_ctx *ctx);
const char *zk_last_error(zk_ctx *ctx);
/* use an externally owned hipStream_t (e.g. torch's current stream); NULL = ctx-owned stream */
int zk_ctx_set_stream(zk_ctx *ctx, void *hip_stream);
int zk_ctx_sync(zk_ctx *ctx);
const char *zk_version(void);
/* number of GPUs visible to the library (a party-per-GPU caller sizes its world with it); < 0: zk_status */
int zk_device_count(void);

/* free / total bytes of the ctx's GPU (hipMemGetInfo; parked zk_free blocks count as used) */
int zk_mem_info(zk_ctx *ctx, size_t *h_free, size_t *h_total);
/* The ARENA PLAN of a ctx: the sizes its scratch arenas (MSM passes, asynchronous MSM lanes, sumcheck family, pinned staging) have
 * grown to.  The arenas are sized on demand, so the FIRST proof of a process pays their allocation (n = 24: ~110 GB, seconds).  A
 * prover issues the same passes proof after proof: export the plan after one proof of a parameter-set shape (a few hundred bytes,
 * ZK_ARENA_PLAN_WORDS u64 -- keep it beside the proving key), import it right after zk_ctx_create in later processes, and the first
 * proof allocates nothing.  Import only grows arenas; ZK_ERR_INVALID for a buffer that is not a plan, ZK_ERR_OOM when the device
 * cannot hold it (what was allocated stays).  No reference counterpart: the reference allocates per call (Vec per round). */
#define ZK_ARENA_PLAN_WORDS 48
int zk_arena_plan_export(zk_ctx *ctx, uint64_t *h_plan /* [ZK_ARENA_PLAN_WORDS] */);
int zk_arena_plan_import(zk_ctx *ctx, const uint64_t *h_plan /* [ZK_ARENA_PLAN_WORDS] */);
/* ---- device memory helpers for non-HIP callers.  zk_free parks the block in the ctx (no device
 * synchronisation) and zk_malloc of the same size reuses it; everything is released with the ctx. -- */
int zk_malloc(zk_ctx *ctx, size_t bytes, void **d_out);
int zk_free(zk_ctx *ctx, void *d_ptr);
/* release every parked block to the driver now (other allocators in the process -- torch, RCCL -- cannot
 * see parked memory); *h_freed_bytes (optional) receives the number of bytes returned.  Every internal
 * allocation of the library does this by itself, and retries once, when the device is out of memory. */
int zk_trim(zk_ctx *ctx, size_t *h_freed_bytes);
int zk_memcpy_h2d(zk_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int zk_memcpy_d2h(zk_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);
int zk_memcpy_d2d(zk_ctx *ctx, void *d_dst, const void *d_src, size_t bytes); /* asynchronous, on the ctx stream */

/* ---- element-wise Fr (hyperplonk/src/dhyperplonk.rs:233-238,251-256,326-339) -------- */
/* zk_fr_add / sub / mul / axpb: d_out may be d_a or d_b itself (the same address, not a shifted overlap): a lane reads row i of both inputs before it stores row i. */
int zk_fr_add(zk_ctx *ctx, const void *d_a, const void *d_b, void *d_out, size_t n);
int zk_fr_sub(zk_ctx *ctx, const void *d_a, const void *d_b, void *d_out, size_t n);
int zk_fr_mul(zk_ctx *ctx, const void *d_a, const void *d_b, void *d_out, size_t n);
/* out[i] = a[i] + alpha*b[i] + beta          (`s + alpha*sid + beta`, dhyperplonk.rs:326-337);
 * d_a may be NULL (taken as zero): out = alpha*b + beta */
int zk_fr_axpb(zk_ctx *ctx, const void *d_a, const void *d_b, const uint64_t h_alpha[4],
               const uint64_t h_beta[4], void *d_out, size_t n);
/* A small PUBLIC Fr matrix applied to k vectors at once -- the PSS maps on field elements
 * (pack_from_public / unpack / unpack2, secret-sharing/src/pss.rs:93-171; degree reduction
 * degree_reduce.rs:17-23) for any packing factor l:
 *   out[j*out_vec_stride + r*out_row_stride] = sum_c M[r*cols + c] * in[j*in_vec_stride + c*in_comp_stride]
 * strides in elements; h_matrix = rows*cols Fr (Montgomery) on the host. */
int zk_fr_apply_matrix(zk_ctx *ctx, const uint64_t *h_matrix, size_t rows, size_t cols, const void *d_in,
                       size_t in_vec_stride, size_t in_comp_stride, void *d_out, size_t out_vec_stride,
                       size_t out_row_stride, size_t k);
/* The same maps by transforms, as the reference computes them (ark-poly radix-2 (coset) FFTs, pss.rs:93-171),
 * for packing factors where the dense matrix is the slower form (8l >= 64): every vector is interpolated on a
 * domain of size A, cut / zero-extended to min(A, B) coefficients, and evaluated on a domain of size B:
 *   c = IDFT_A(in[0..n_in) zero-padded);  c[i] *= scale[i];  e = DFT_B(c zero-padded);  out[r] = e[r * step], r < take.
 * h_winv: A/2 powers of omega_A^-1, h_w: B/2 powers of omega_B, h_scale: min(A, B) factors A^-1 (offB/offA)^i
 * (the coset offsets of `get_coset`), all Montgomery Fr; A, B powers of two <= 512.  Strides as above.
 *   pack_from_public: A = 2l (coset g), B = 8l, n_in = l (or 2l), take = 8l
 *   unpack:  A = 8l, B = 2l (coset g), take = l          unpack2: A = 8l, B = 4l (coset g), take = l, step = 2 */
int zk_fr_ntt_map(zk_ctx *ctx, size_t A, const uint64_t *h_winv, size_t B, const uint64_t *h_w, const uint64_t *h_scale,
                  size_t n_in, size_t take, size_t step, const void *d_in, size_t in_vec_stride, size_t in_comp_stride,
                  void *d_out, size_t out_vec_stride, size_t out_row_stride, size_t k);
/* strided views of the product tree (dacc_product.rs:41-55, dhyperplonk.rs:344-359):
 * even[i] = t[2i] (v(x,0)), odd[i] = t[2i+1] (v(x,1)), i < n; v(1,x) is the contiguous upper half. */
int zk_fr_deinterleave(zk_ctx *ctx, const void *d_t, void *d_even, void *d_odd, size_t n);
/* out[i] = num[i] / den[i] (dhyperplonk.rs:339), batched inversion; ZK_ERR_DIV_ZERO if a den is 0 */
int zk_fr_batch_div(zk_ctx *ctx, const void *d_num, const void *d_den, void *d_out, size_t n);

/* ---- sumcheck family ---------------------------------------------------------------- */
/* Phase-1 loop of sumcheck / c_sumcheck / d_sumcheck (dsumcheck.rs:10-21 = :107-121 = :301-315).
 * d_tab: len = 2^n Fr (not modified). h_chal: n Fr. h_out_pairs: n pairs (sum_lo, sum_hi) = 2n Fr.
 * h_last: the single remaining table element (the caller appends (0,last), runs pss2ss, ...). */
int zk_sumcheck(zk_ctx *ctx, const void *d_tab, size_t len, const uint64_t *h_chal,
                uint64_t *h_out_pairs, uint64_t h_last[4]);
/* Phase-1 loop of sumcheck_product / c_ / d_ (dsumcheck.rs:37-85 = :167-219 = :377-429).
 * h_out_triples: n x (t0,t1,t2) = 3n Fr; h_last_f / h_last_g: remaining elements. */
int zk_sumcheck_product(zk_ctx *ctx, const void *d_f, const void *d_g, size_t len,
                        const uint64_t *h_chal, uint64_t *h_out_triples, uint64_t h_last_f[4],
                        uint64_t h_last_g[4]);
/* fix_variable (mle.rs:88-105): fold min(n, n_points) times; d_out receives len >> rounds Fr. */
int zk_fold(zk_ctx *ctx, const void *d_tab, size_t len, const uint64_t *h_points, size_t n_points,
            void *d_out);
/* eq table of a point tau of n variables: d_out[x] = prod_i (x_i ? tau_i : 1 - tau_i), x_0 the TOP index bit (the variable
 * round 0 of the sumchecks binds), len = 2^n Fr; h_point: n Fr.  Built by doubling.  sum_x out[x] = 1, and zk_fold(out, r)
 * leaves eq(tau, r) = prod_i (tau_i r_i + (1 - tau_i)(1 - r_i)).  The real form of the `eq` vector the reference samples
 * at random (hyperplonk/src/hyperplonk.rs:69-71, dhyperplonk.rs:218-222).  n = 0 gives [1].  ASYNCHRONOUS on the ctx stream like the
 * element-wise calls: h_point is copied before the call returns, d_out is complete for later calls on this ctx or after zk_ctx_sync. */
int zk_eq_table(zk_ctx *ctx, const uint64_t *h_point, size_t n, void *d_out);
/* The gate identity as ONE sumcheck -- the virtual circuit the reference simulates with six independent product sumchecks
 * (hyperplonk.rs:66-93, dhyperplonk.rs:218-260): the prover's rounds for
 *     G(x) = eq(x) [ q1(x) (a(x) + b(x)) + q2(x) a(x) b(x) - c(x) + in(x) ]
 * over seven tables of len = 2^n Fr (not modified).  Round i writes five Fr to h_out_evals: the round polynomial (degree 4)
 * at t = 0, 1, 2, 3, 4, every table extended as (1 - t) lo + t hi (dsumcheck.rs:52-66), then folds the seven tables with
 * h_chal[i].  h_out_evals: 5n Fr; h_last: the seven remaining elements (eq, q1, q2, a, b, c, in), 7 Fr.
 * Blocking: the results are on the host when it returns.  len < 2, not a power of two or > 2^35, or a null pointer: ZK_ERR_INVALID;
 * nothing is written on error. */
int zk_sumcheck_gate(zk_ctx *ctx, const void *d_eq, const void *d_q1, const void *d_q2, const void *d_a,
                     const void *d_b, const void *d_c, const void *d_in, size_t len, const uint64_t *h_chal,
                     uint64_t *h_out_evals, uint64_t *h_last);
/* The wiring identity (HyperPlonk's ProductCheck) as ONE sumcheck -- the reference simulates it with six independent product
 * sumchecks on six unrelated polynomials (hyperplonk.rs:94-141): the prover's rounds for
 *     F(x) = eq(x) [ v(1,x) - v(x,0) v(x,1) + gamma ( den(x) h(x) - num(x) ) ]
 * where v = d_tree is the 2N Fr of zk_product_tree(h), h = num / den, and with index bit 0 the TOP bit
 *     v(0,x) = h = tree[x],  v(1,x) = tree[N + x],  v(x,0) = tree[2x],  v(x,1) = tree[2x + 1].
 * d_eq, d_num, d_den: N = 2^mu Fr each; d_tree: 2N Fr; none is modified, and the four views are read in place (no
 * deinterleaved copies by the caller or the library).  Round i writes four Fr to h_out_evals: the round polynomial (degree 3) at
 * t = 0, 1, 2, 3, every table extended as (1 - t) lo + t hi, then folds the seven tables with h_chal[i].
 * h_out_evals: 4 mu Fr; h_last: the seven remaining elements in the order eq, v1x, vx0, vx1, h, num, den, 7 Fr.
 * Blocking: the results are on the host when it returns.  N < 2, not a power of two or > 2^35, or a null pointer: ZK_ERR_INVALID;
 * nothing is written on error. */
int zk_sumcheck_wiring(zk_ctx *ctx, const void *d_eq, const void *d_tree, const void *d_num, const void *d_den,
                       size_t N, const uint64_t h_gamma[4], const uint64_t *h_chal, uint64_t *h_out_evals,
                       uint64_t *h_last);
/* ---- the wiring identity over the THREE wire columns of a Plonk gate (a, b, c = columns j = 0, 1, 2 of N = 2^mu rows) ----
 * Slot j N + x is wire j of row x; sigma permutes the 3N slots and ssigma_j(x) = sigma(j N + x) as a field element.
 *     n_j(x) = w_j(x) + alpha (j N + x) + beta,   d_j(x) = w_j(x) + alpha ssigma_j(x) + beta
 * zk_perm3_terms writes the six linear tables, P = n_0 n_1 n_2 and Q = d_0 d_1 d_2 in ONE pass (N Fr each; the slot number is formed in
 * the kernel: no table of slot numbers exists).  h = zk_fr_batch_div(P, Q) (a zero denominator: ZK_ERR_DIV_ZERO there), and
 * v = zk_product_tree(h).  The inputs are not modified; an output may not alias an input.  ASYNCHRONOUS on the ctx stream like the
 * element-wise calls.  N < 2, not a power of two or > 2^35, or a null pointer: ZK_ERR_INVALID, nothing is launched. */
int zk_perm3_terms(zk_ctx *ctx, const void *const d_w[3], const void *const d_ssigma[3], size_t N,
                   const uint64_t h_alpha[4], const uint64_t h_beta[4], void *const d_num[3], void *const d_den[3],
                   void *d_P, void *d_Q);
/* The prover's rounds for
 *     F(x) = eq(x) [ v(1,x) - v(x,0) v(x,1) + gamma ( h(x) d_0(x) d_1(x) d_2(x) - n_0(x) n_1(x) n_2(x) ) ]
 * with v = d_tree the 2N Fr of zk_product_tree(h) and its four views read in place as in zk_sumcheck_wiring.  d_eq, d_num[j], d_den[j]:
 * N Fr each; none is modified.  Round i writes six Fr to h_out_evals: the round polynomial (degree 5) at t = 0 .. 5, every table
 * extended as (1 - t) lo + t hi, then folds the eleven tables with h_chal[i].  h_out_evals: 6 mu Fr; h_last: the eleven remaining
 * elements in the order eq, v1x, vx0, vx1, h, n_0, n_1, n_2, d_0, d_1, d_2, 11 Fr.  Blocking: the results are on the host when it
 * returns.  N < 2, not a power of two or > 2^35, a null pointer, or the knob perm3_local_e not a power of two in [1, 256]:
 * ZK_ERR_INVALID; nothing is launched or written on error. */
int zk_sumcheck_perm3(zk_ctx *ctx, const void *d_eq, const void *d_tree, const void *const d_num[3],
                      const void *const d_den[3], size_t N, const uint64_t h_gamma[4], const uint64_t *h_chal,
                      uint64_t *h_out_evals, uint64_t *h_last);
/* The WIDE Plonk gate as ONE sumcheck: six selectors (a constant, separate weights of the two additive wires, an output selector) and a
 * fifth-power term, so that an S-box row c = a^5 + const is one row: the prover's rounds for
 *     W(x) = eq(x) [ qL(x) a(x) + qR(x) b(x) + qM(x) a(x) b(x) + qH(x) a(x)^5 - qO(x) c(x) + qC(x) + in(x) ]
 * over the eleven tables d_tabs = eq, qL, qR, qM, qO, qC, qH, a, b, c, in of len = 2^n Fr each (not modified).  Round i writes eight Fr
 * to h_out_evals: the round polynomial (degree 7) at t = 0 .. 7, every table extended as (1 - t) lo + t hi, then folds the eleven
 * tables with h_chal[i].  h_out_evals: 8 n Fr; h_last: the eleven remaining elements in the order of d_tabs, 11 Fr.  Blocking: the
 * results are on the host when it returns.  len < 2, not a power of two or > 2^35, a null pointer, or the knob gatew_local_e not a
 * power of two in [1, 256]: ZK_ERR_INVALID; nothing is launched or written on error. */
int zk_sumcheck_gate_wide(zk_ctx *ctx, const void *const d_tabs[11], size_t len, const uint64_t *h_chal,
                          uint64_t *h_out_evals, uint64_t *h_last);
/* ---- the lookup argument (LogUp): every value of a column f lies in a table t, both of N = 2^n Fr ----
 * The multiplicities m[y] = #{x : idx[x] = y} of the caller's row-to-table indices (idx: N u32 on the device, f[x] = t[idx[x]]) as
 * N Fr in Montgomery form.  One pass checks idx[x] < N BEFORE anything is read through it, compares the four limbs of f[x] and
 * t[idx[x]] and counts on u32 counters; a second pass writes the counters as field elements.  Blocking (a status word is read back).
 * An index >= N or a row whose value is not the table's entry: ZK_ERR_INVALID, zk_last_error gives the number of such rows, d_m is
 * unspecified, nothing is read out of bounds.  N < 2, not a power of two or > 2^32, or a null pointer: ZK_ERR_INVALID, nothing is
 * launched.  The inputs are not modified. */
int zk_lookup_multiplicities(zk_ctx *ctx, const void *d_f, const void *d_t, const uint32_t *d_idx, size_t N, void *d_m);
/* The sum identity of LogUp and the definitions of its two helper columns as ONE sumcheck: with df = beta + f, dt = beta + t,
 * hf = 1 / df, ht = m / dt the prover's rounds for
 *     L(x) = hf(x) - ht(x) + E(x) [ hf(x) df(x) - 1 + gamma ( ht(x) dt(x) - m(x) ) ],        E = lambda eq(tau, .)
 * over the six tables d_tabs = E, df, dt, m, hf, ht of len = 2^n Fr each (not modified; lambda is folded into E with
 * zk_eq_table_acc, beta into df and dt).  The first two terms are NOT multiplied by E.  Round i writes four Fr to h_out_evals: the
 * round polynomial (degree 3) at t = 0, 1, 2, 3, every table extended as (1 - t) lo + t hi, then folds the six tables with h_chal[i].
 * h_out_evals: 4 n Fr; h_last: the six remaining elements in the order of d_tabs, 6 Fr.  Blocking: the results are on the host when
 * it returns.  len < 2, not a power of two or > 2^35, a null pointer, or the knob lookup_local_e not a power of two in [1, 512]:
 * ZK_ERR_INVALID; nothing is launched or written on error. */
int zk_sumcheck_lookup(zk_ctx *ctx, const void *const d_tabs[6], size_t len, const uint64_t h_gamma[4],
                       const uint64_t *h_chal, uint64_t *h_out_evals, uint64_t *h_last);
/* ---- the lookup argument as a path of a Plonk circuit: selector-gated, over the three wire columns ----
 * Row x of N = 2^n with qk(x) = 1 claims (a, b, c)(x) = (t0, t1, t2)(idx[x]); a row with qk(x) = 0 claims nothing.  qk entries are 0 or
 * the Montgomery form of 1.  zk_lookup3_multiplicities writes m[y] = #{x : qk(x) = 1, idx[x] = y} as N Fr in Montgomery form (d_w: a, b,
 * c; d_t: t0, t1, t2; d_idx: N u32).  A row with qk = 0 is skipped and its index is never read through.  A row with qk = 1 is good when
 * idx[x] < N -- checked BEFORE anything is read through it -- and all twelve limbs of the two triples agree.  Any other row, a qk that is
 * neither 0 nor 1 among them, is a bad row: ZK_ERR_INVALID, zk_last_error gives the number of such rows ("K of N rows ..."), d_m is
 * unspecified, nothing is read out of bounds.  Blocking.  N < 2, not a power of two or > 2^32, or a null pointer: ZK_ERR_INVALID,
 * nothing is launched.  The inputs are not modified. */
int zk_lookup3_multiplicities(zk_ctx *ctx, const void *const d_w[3], const void *const d_t[3], const void *d_qk,
                              const uint32_t *d_idx, size_t N, void *d_m);
/* ---- lookups without caller indices: the device finds the table rows itself ----
 * zk_lookup_find: for every row x of N = 2^n the SMALLEST y with t[y] == f[x] (all four limbs) as d_idx[x] (N u32), and the multiplicities
 * m[y] = #{x : idx[x] = y} as N Fr in Montgomery form in d_m: bit for bit what zk_lookup_multiplicities writes for that idx.  Either output
 * may be null, not both; an output that is given is written in all N entries on success.  Two phases on the ctx stream: every entry y < N is
 * inserted into an open-addressing hash table of u32 slots (a power of two >= 2N of them, scratch of the ctx; linear probing; equal entries
 * share ONE slot, which ends holding the smallest of their indices whatever the order of the threads -- a table padded by repeating an entry
 * is the normal case), then every row walks the same sequence to its entry and counts on a u32 counter.  The result does not depend on the
 * hash function.  Blocking (a status word is read back).  A row whose value is no entry of the table: ZK_ERR_INVALID, zk_last_error gives the
 * number of such rows ("K of N rows ...", the wording of zk_lookup_multiplicities) and the smallest such row; the outputs are unspecified,
 * nothing is read out of bounds.  N < 2, not a power of two or > 2^31 (the empty-slot mark stays outside the index range), f or t null, or
 * both outputs null: ZK_ERR_INVALID, nothing is launched.  Scratch that does not fit the device: ZK_ERR_OOM.  A probe walk longer than the slot
 * array (impossible at a load <= 0.5): ZK_ERR_INTERNAL.  The inputs are not modified. */
int zk_lookup_find(zk_ctx *ctx, const void *d_f, const void *d_t, size_t N, uint32_t *d_idx, void *d_m);
/* The selector-gated three-column form: a row with qk(x) = 1 gets the smallest y with (t0, t1, t2)(y) == (a, b, c)(x) in all twelve limbs; a
 * row with qk(x) = 0 gets idx[x] = 0, is not counted and nothing else of it is read; m[y] = #{x : qk(x) = 1, idx[x] = y}, bit for bit what
 * zk_lookup3_multiplicities writes for that idx.  A selected row whose triple is no entry of the table, or a qk that is neither 0 nor the
 * Montgomery form of 1, is a bad row: ZK_ERR_INVALID with "K of N rows ..." and the smallest bad row in zk_last_error.  Everything else as
 * zk_lookup_find (d_w: a, b, c; d_t: t0, t1, t2; a null column pointer: ZK_ERR_INVALID). */
int zk_lookup3_find(zk_ctx *ctx, const void *const d_w[3], const void *const d_t[3], const void *d_qk, size_t N,
                    uint32_t *d_idx, void *d_m);
/* ---- Plonk witness generation and the witness check on the device ----
 * The rules.  A circuit has N = 2^mu rows and 3N slots; slot j N + x is wire j of row x (a, b, c = 0, 1, 2).  The CLASSES are the cycles
 * of sigma; every class carries one value.
 *   Computing rows.  Row x is COMPUTING when its output coefficient is non-zero.  Basic gate (gate_kind 0; d_sel = q1, q2): every row, with
 *     c = q1 (a + b) + q2 a b + in(x).  Wide gate (gate_kind 1; d_sel = qL, qR, qM, qO, qC, qH): the rows with qO(x) != 0, with
 *     c = (qL a + qR b + qM a b + qH a^5 + qC + in(x)) / qO(x).  in holds the public inputs on rows 0 .. l - 1 and zero elsewhere: an
 *     input row is the same rule, no special case.
 *   Source of a class: the smallest c slot of a computing row in the class.  A class without one is FREE: its value is free[s] for its
 *     smallest slot s (free: 3N Fr of the caller, read only at those slots; null: zeros).  Every slot of the class that is not itself the
 *     c slot of a computing row takes the class's value.  Every computing row computes its own c: a second computing c slot in one class
 *     is an equality assertion -- checked, not assigned.
 *   Level of a computing row: 0 when the classes of both its a and b slots are free, otherwise 1 + the largest level of the source rows
 *     of those classes.  A row that depends on itself, directly or through other rows, has no level: the plan is refused.
 *   Check.  Row x is a BAD GATE ROW when the gate identity does not hold on it (after generation: only a non-computing row); slot s is a
 *     BAD COPY when its value differs from the value of its class -- the c of the source row, or what the class's smallest slot holds
 *     (after generation: only a further computing c slot).  On caller-given a, b, c every row and slot can fail.
 *   Lookups (additive: a plan built without one follows the rules above and nothing else).  A plan may be built with the lookup of the
 *     circuit: the selector qk (N Fr, every entry 0 or the Montgomery form of 1) and the table columns t0, t1, t2 (N Fr each, fully
 *     reduced, padded by repeating an entry).  THE TABLE MUST BE A FUNCTION OF ITS FIRST TWO COLUMNS: two entries with equal (t0, t1)
 *     in all eight limbs have equal t2 (repeating a whole entry is therefore allowed).
 *     Row x is LOOKUP-COMPUTING when qk(x) = 1 and it is not gate-computing (wide gate: qO(x) = 0; basic gate: never, every row is
 *     gate-computing).  Its c is t2[y] for the smallest y with (t0, t1)[y] == (a, b)(x); with no such y its c is 0 and the check
 *     reports the row.  A row with qk = 1 that is gate-computing stays gate-computing: the table only checks it.  Wherever the rules
 *     above say "computing row" they mean gate-computing or lookup-computing: the source of a class, the levels (edges from the source
 *     rows of the a and b slots), the refusal of rows that depend on their own output; a second computing c slot in a class is still an
 *     equality assertion.
 *     Check: row x is a BAD LOOKUP when qk(x) = 1 and (a, b, c)(x) is no table entry, whether the row is lookup- or gate-computing.
 *     Because the table is a function this is exact with the pairs alone: the row is good iff (a, b) is the pair of some entry y and
 *     c == t2[y].
 *     On generated wires the index zk_lookup3_find gives for a lookup-computing row is the y the generator used (a smaller index with an
 *     equal triple would have an equal pair), so the proof's multiplicities need nothing from the generator.
 *   Advice (additive: a plan built without a non-zero code follows the rules above and nothing else).  A circuit may carry ADVICE: N u32
 *     codes, one per row, 0 meaning none.  Advice is prover-side only: not preprocessed, not committed, in no vk, proof or digest of them.
 *       ZK_ADV_INV0 = 1                              c = 1 / a mod r, and c = 0 when a = 0.  b is gathered and stored as usual, not used.
 *       ZK_ADV_BITS(shift, width) = 2 | shift << 8 | width << 16
 *                                                    c = (A >> shift) mod 2^width for the canonical integer A in [0, r) of a;
 *                                                    0 <= shift, 1 <= width <= 64, shift + width <= 255.
 *     Bits 24 .. 31 of a code are 0; anything else is an UNKNOWN code.
 *     A row with a non-zero code is ADVICE-COMPUTING: a computing row like the other two kinds for the source of a class, the levels and
 *     the refusal of rows that depend on their own output.  It must not also be gate-computing (wide gate: qO(x) = 0; the basic gate
 *     computes on every row and so has no advice row: any non-zero code is refused) nor lookup-computing (qk(x) = 0).  It constrains
 *     nothing by itself: soundness comes from ordinary gate rows next to it.  The CHECK does not test advice values -- h_bad keeps its
 *     four (lookup plans: six) numbers -- so a witness may hold other advice where the constraints allow it (any c for INV0 of 0).
 *     The outputs are fully reduced Montgomery forms, as every wire zk_plonk_witness writes; a free value or public input at or above r
 *     is reduced before the advice acts on it.
 *
 * zk_witness_plan_create: the plan of one circuit, built once, on the host, in O(N): the cycles, the source of every slot, the levels
 * (Kahn's algorithm), the rows ordered by (level, row), the launch schedule; uploads 3N + N u32, the level offsets and, with d_out_sel,
 * N Fr of 1 / qO (zk_fr_batch_div; the only kernel of the call).  h_sigma: 3N slot numbers; d_out_sel: the output selector qO as N Fr on
 * the device (fully reduced Montgomery forms), or NULL: every row computes (the basic gate).  N < 2, not a power of two or > 2^29, a
 * sigma that is not a permutation, a qO that is not reduced below r ("the output selector of row X ..."; the test for zero is on the
 * limbs): ZK_ERR_INVALID.  Rows without a level: ZK_ERR_INVALID, zk_last_error gives "K of N rows depend on their own output" and the smallest
 * such row.  The plan belongs to ctx and must be freed before it. */
typedef struct zk_witness_plan zk_witness_plan;
int zk_witness_plan_create(zk_ctx *ctx, const uint64_t *h_sigma, const void *d_out_sel, size_t N, zk_witness_plan **out);
/* The plan of a circuit WITH its lookup: zk_witness_plan_create, and the plan owns a KEY TABLE -- 2N u32 slots of the open-addressing
 * protocol of zk_lookup_find over the pair (t0, t1), built once, here, on the device; the probes of every later call are plain loads.
 * d_qk: N Fr; d_t: t0, t1, t2, N Fr each.  A qk entry that is neither 0 nor 1: ZK_ERR_INVALID, "K of N entries of qk are neither 0 nor 1"
 * and the smallest such row.  A table that is no function of (t0, t1): ZK_ERR_INVALID, "K of N table entries repeat the pair (t0, t1) of
 * an earlier entry with another t2; the first is entry Y" -- K counts the entries whose t2 differs from the t2 of the FIRST entry of their
 * pair, Y is the smallest of them; neither depends on the order of the threads.  The knob find_force_slot applies to this table as to
 * those of zk_lookup_find: it is read here, kept in the plan and used by every walk of the plan; no result depends on it.  Everything
 * else as zk_witness_plan_create (the messages name this call).  Blocking.  zk_witness_plan_info and zk_witness_plan_free serve both. */
int zk_witness_plan_create_lookup(zk_ctx *ctx, const uint64_t *h_sigma, const void *d_out_sel, const void *d_qk, const void *const d_t[3],
                                  size_t N, zk_witness_plan **out);
/* The plan of a circuit WITH its advice codes (h_advice: N u32 on the host; the plan keeps a device copy), and with its lookup when d_qk
 * and d_t are given (both NULL: no lookup).  With all codes zero the plan is the one zk_witness_plan_create / _create_lookup builds.
 * Refusals beyond theirs (ZK_ERR_INVALID, nothing stays allocated; K and X are properties of the inputs): "K of N advice codes are
 * unknown; the first is row X"; "K of N advice rows also compute by the gate or the table; the first is row X" (every advice row when
 * d_out_sel is NULL); the rows that depend on their own output include the advice rows.  zk_plonk_witness (no lookup) and
 * zk_plonk_witness_lookup run such a plan: an advice row takes its c in the level where its a becomes known; inside a level the advice
 * rows stand together.  zk_witness_plan_info counts them as computing rows.  The check calls take such plans as they are. */
#define ZK_ADV_INV0 1u
#define ZK_ADV_BITS(shift, width) (2u | (uint32_t)(shift) << 8 | (uint32_t)(width) << 16)
int zk_witness_plan_create_advice(zk_ctx *ctx, const uint64_t *h_sigma, const void *d_out_sel, const void *d_qk, const void *const d_t[3],
                                  const uint32_t *h_advice, size_t N, zk_witness_plan **out);
void zk_witness_plan_free(zk_witness_plan *plan);
/* levels: how many levels the computing rows have (the largest level + 1); max_level_rows: the rows of the largest level; launches: the
 * level launches of one zk_plonk_witness -- a level of more than 256 rows is one launch of many workgroups, a run of consecutive
 * levels of at most 256 rows each is ONE launch of ONE 256-thread workgroup that walks them with a barrier in between (the fill pass
 * and the check are not counted).  Any output may be NULL. */
int zk_witness_plan_info(const zk_witness_plan *plan, size_t *levels, size_t *max_level_rows, size_t *launches);
/* zk_plonk_witness: a, b, c (N Fr each, fully reduced Montgomery forms; three distinct buffers) from the selectors, the l public inputs
 * (host, l x 4 u64 Montgomery) and free.  The level launches follow one another on the ctx stream with no host read in between, no
 * kernel waits on another workgroup; a last pass fills the rows that compute nothing; then the check below runs on the result
 * (blocking: ONE status read).  A bad gate row or a bad copy: ZK_ERR_INVALID, zk_last_error gives "K of N rows do not satisfy the gate"
 * / "K of 3N slots differ from the value of their class" and the smallest index; a, b, c then hold what was generated.  gate_kind other
 * than 0 / 1, a wide gate on a plan built without d_out_sel (or the basic gate on one built with it), l > N, a null selector:
 * ZK_ERR_INVALID, nothing is launched.  The division uses the plan's 1 / qO: d_sel[3] must be the selector the plan was built from.
 * Nothing is read out of bounds whatever free and the selectors hold; the inputs are not modified. */
int zk_plonk_witness(zk_ctx *ctx, const zk_witness_plan *plan, int gate_kind, const void *const *d_sel, const uint64_t *h_public_inputs,
                     size_t l, const void *d_free, void *d_a, void *d_b, void *d_c);
/* The check alone, on any a, b, c: h_bad = { bad gate rows, the smallest (2^64 - 1: none), bad copies, the smallest slot (2^64 - 1:
 * none) }.  a, b, c must be fully reduced Montgomery forms, as zk_plonk_witness writes them: copies are compared limb for limb, so a
 * wire at or above r is reported as a bad copy of its reduced twin (nothing is read out of bounds; the public inputs are reduced when
 * read).  Returns ZK_OK whatever it counts (the report is the result); blocking, the inputs are not modified. */
int zk_plonk_witness_check(zk_ctx *ctx, const zk_witness_plan *plan, int gate_kind, const void *const *d_sel,
                           const uint64_t *h_public_inputs, size_t l, const void *d_a, const void *d_b, const void *d_c, uint64_t h_bad[4]);
/* The two calls on a plan built by zk_witness_plan_create_lookup.  d_qk and d_t are passed per call, as the selectors are, and MUST be the
 * ones the plan was built from (the plan keeps indices into the tables, not the tables; other tables of N entries give other wires and
 * reports, never a read out of bounds).  zk_plonk_witness_lookup: zk_plonk_witness, and the lookup-computing rows of the wide gate take
 * their c from the table in the level they belong to (the basic gate has none); the check then also counts the bad lookups, and a
 * witness with any is refused: "K of N rows with qk = 1 hold a triple that is no table entry; the first is row R", joined to the two
 * other reports with "; " when several fail (gate, copies, lookups in that order).  zk_plonk_witness_check_lookup: h_bad gains
 * { bad lookups, the smallest such row (2^64 - 1: none) }.  A walk that passes every slot of the key table (impossible at a load <= 0.5):
 * ZK_ERR_INTERNAL.  A _lookup call on a plan built without a lookup, or zk_plonk_witness / zk_plonk_witness_check on a plan built with
 * one: ZK_ERR_INVALID with a message, nothing is launched. */
int zk_plonk_witness_lookup(zk_ctx *ctx, const zk_witness_plan *plan, int gate_kind, const void *const *d_sel, const void *d_qk,
                            const void *const d_t[3], const uint64_t *h_public_inputs, size_t l, const void *d_free, void *d_a, void *d_b,
                            void *d_c);
int zk_plonk_witness_check_lookup(zk_ctx *ctx, const zk_witness_plan *plan, int gate_kind, const void *const *d_sel, const void *d_qk,
                                  const void *const d_t[3], const uint64_t *h_public_inputs, size_t l, const void *d_a, const void *d_b,
                                  const void *d_c, uint64_t h_bad[6]);
/* df = beta + a + zeta b + zeta^2 c and dt = beta + t0 + zeta t1 + zeta^2 t2 in ONE pass (N Fr each).  The inputs are not modified; an
 * output may not alias an input.  ASYNCHRONOUS on the ctx stream like zk_perm3_terms.  N < 2, not a power of two or > 2^35, or a null
 * pointer: ZK_ERR_INVALID, nothing is launched. */
int zk_lookup3_terms(zk_ctx *ctx, const void *const d_w[3], const void *const d_t[3], size_t N, const uint64_t h_zeta[4],
                     const uint64_t h_beta[4], void *d_df, void *d_dt);
/* zk_sumcheck_lookup with a selector: with hf = qk / df and ht = m / dt the prover's rounds for
 *     L(x) = hf(x) - ht(x) + E(x) [ hf(x) df(x) - qk(x) + gamma ( ht(x) dt(x) - m(x) ) ],        E = lambda eq(tau, .)
 * over the SEVEN tables d_tabs = E, df, dt, m, hf, ht, qk of len = 2^n Fr each (not modified).  Round i writes four Fr to h_out_evals: the
 * round polynomial (degree 3) at t = 0, 1, 2, 3, then folds the seven tables with h_chal[i].  h_out_evals: 4 n Fr; h_last: the seven
 * remaining elements in the order of d_tabs, 7 Fr.  With qk = 1 everywhere the rounds and the first six last values are those of
 * zk_sumcheck_lookup, bit for bit.  Blocking.  len < 2, not a power of two or > 2^35, a null pointer, or the knob lookupsel_local_e not
 * a power of two in [1, 512]: ZK_ERR_INVALID; nothing is launched or written on error. */
int zk_sumcheck_lookup_sel(zk_ctx *ctx, const void *const d_tabs[7], size_t len, const uint64_t h_gamma[4],
                           const uint64_t *h_chal, uint64_t *h_out_evals, uint64_t *h_last);
/* ---- batch opening: K claims f_{j_k}(z_k) = v_k on J tables of one size -> one degree-2 sumcheck and one opening ---- */
/* d_acc[x] += weight * eq(point, x) over the cube of n variables (x_0 the TOP index bit), d_acc: 2^n Fr, read and written.  The
 * doubling scheme of zk_eq_table seeded with the weight; the last level is added into d_acc instead of stored, so a claim costs
 * one level of scratch (2^(n-1) Fr), not a table.  Coordinates 0 and 1 come out exact: the point (1,..,1,0) adds the weight to one
 * entry and zero to the others.  n = 0 adds the weight to d_acc[0].  ASYNCHRONOUS on the ctx stream like zk_eq_table. */
int zk_eq_table_acc(zk_ctx *ctx, const uint64_t *h_point, size_t n, const uint64_t h_weight[4], void *d_acc);
/* d_out[x] = sum_j c_j * d_tabs[j][x], x < len, 1 <= count <= 16; h_coeffs: count Fr (Montgomery).  d_out may be one of the inputs.
 * Wide multiply-accumulates and ONE Montgomery reduction per output: 32 (count + 1) len bytes of traffic.  ASYNCHRONOUS on the ctx
 * stream (the pointer array and the coefficients are copied before the call returns).  count 0 or > 16, or a null pointer:
 * ZK_ERR_INVALID. */
int zk_fr_lincomb(zk_ctx *ctx, size_t count, const void *const *d_tabs, const uint64_t *h_coeffs, size_t len, void *d_out);
/* The prover's rounds of  sum_x sum_j E_j(x) f_j(x)  over count <= 16 pairs of tables of len = 2^n Fr (not modified): round i writes
 * (t0, t1, t2), the round polynomial at t = 0, 1, 2 -- the triple of zk_sumcheck_product (dsumcheck.rs:38-72) summed over j -- and
 * folds all 2 count tables with h_chal[i].  h_out_triples: 3n Fr; h_last_e / h_last_f: count Fr each, E_j(chal) and f_j(chal).
 * count = 1 is zk_sumcheck_product bit for bit.  Blocking: the results are on the host when it returns.
 * Capacity: the sums of a round are 544-bit integers of count * len / 2 products < 2^512, so count * len <= 2^33.
 * count 0 or > 16, len < 2 or not a power of two, count * len > 2^33, or a null pointer: ZK_ERR_INVALID; nothing is written on error. */
int zk_sumcheck_multi(zk_ctx *ctx, size_t count, const void *const *d_e, const void *const *d_f, size_t len,
                      const uint64_t *h_chal, uint64_t *h_out_triples, uint64_t *h_last_e, uint64_t *h_last_f);
/* ---- Fiat-Shamir on the device: a transcript whose state lives in device memory, and the three fused sumchecks driven by it ----
 * The transcript is a SHA-256 hash chain on a 32-byte state (normative: the device, both hosts and the test model agree byte for byte):
 *   init(label):   state = SHA256("zkhip-fs-v1" || label)
 *   absorb(data):  state = SHA256(state || 0x00 || data); field elements and points go in as they sit in proof records (little-endian
 *                  u64 limbs, Montgomery form), integers such as n as one little-endian u64
 *   challenge():   d = SHA256(state || 0x01), state = d; the challenge is d read as a little-endian 256-bit integer with its top two
 *                  bits cleared: < 2^254 < r, so there is no rejection loop.
 * A transcript belongs to the ctx it was created on (any other: ZK_ERR_INVALID) and is freed BEFORE that ctx.  create, absorb and
 * absorb_device are ASYNCHRONOUS on the ctx stream (host bytes are copied before the call returns); challenges and state wait for it.
 * ONE lane hashes an absorb, byte by byte: it is meant for statements, commitments and values.  An absorb of more than 2^20 bytes
 * is refused with ZK_ERR_INVALID (commit to a table and absorb the commitment instead). */
typedef struct zk_transcript zk_transcript;
int zk_transcript_create(zk_ctx *ctx, const void *h_label, size_t label_len, zk_transcript **out); /* label_len <= 2048 */
void zk_transcript_free(zk_transcript *t);
int zk_transcript_absorb(zk_ctx *ctx, zk_transcript *t, const void *h_bytes, size_t len);
int zk_transcript_absorb_device(zk_ctx *ctx, zk_transcript *t, const void *d_ptr, size_t len);
/* count successive challenges; h_out: count Fr in Montgomery form */
int zk_transcript_challenges(zk_ctx *ctx, zk_transcript *t, size_t count, uint64_t *h_out);
int zk_transcript_state(zk_ctx *ctx, zk_transcript *t, uint8_t h_state32[32]);
/* zk_sumcheck_gate / zk_sumcheck_wiring / zk_sumcheck_perm3 / zk_sumcheck_gate_wide / zk_sumcheck_multi with every challenge DERIVED: round i's evaluations are
 * absorbed as they appear in the output (5, 4, 6, 8 or 3 Fr) and one challenge is drawn, on the device, between the kernels of ONE enqueue -- no host read and
 * one stream synchronisation per call.  h_chal_out: the n challenges that were used (Montgomery Fr); every other argument, the
 * outputs, the limits and the error cases are those of the parent, and for the challenges in h_chal_out the parent returns the same
 * bits.  The transcript has absorbed all n rounds when the call returns.  A null transcript or one of another ctx: ZK_ERR_INVALID. */
int zk_sumcheck_gate_fs(zk_ctx *ctx, const void *d_eq, const void *d_q1, const void *d_q2, const void *d_a,
                        const void *d_b, const void *d_c, const void *d_in, size_t len, zk_transcript *t,
                        uint64_t *h_out_evals, uint64_t *h_last, uint64_t *h_chal_out);
int zk_sumcheck_wiring_fs(zk_ctx *ctx, const void *d_eq, const void *d_tree, const void *d_num, const void *d_den,
                          size_t N, const uint64_t h_gamma[4], zk_transcript *t, uint64_t *h_out_evals,
                          uint64_t *h_last, uint64_t *h_chal_out);
int zk_sumcheck_perm3_fs(zk_ctx *ctx, const void *d_eq, const void *d_tree, const void *const d_num[3],
                         const void *const d_den[3], size_t N, const uint64_t h_gamma[4], zk_transcript *t,
                         uint64_t *h_out_evals, uint64_t *h_last, uint64_t *h_chal_out);
int zk_sumcheck_gate_wide_fs(zk_ctx *ctx, const void *const d_tabs[11], size_t len, zk_transcript *t,
                             uint64_t *h_out_evals, uint64_t *h_last, uint64_t *h_chal_out);
/* zk_sumcheck_lookup in the same form (4 Fr absorbed per round) */
int zk_sumcheck_lookup_fs(zk_ctx *ctx, const void *const d_tabs[6], size_t len, const uint64_t h_gamma[4],
                          zk_transcript *t, uint64_t *h_out_evals, uint64_t *h_last, uint64_t *h_chal_out);
/* zk_sumcheck_lookup_sel in the same form (4 Fr absorbed per round) */
int zk_sumcheck_lookup_sel_fs(zk_ctx *ctx, const void *const d_tabs[7], size_t len, const uint64_t h_gamma[4],
                              zk_transcript *t, uint64_t *h_out_evals, uint64_t *h_last, uint64_t *h_chal_out);
int zk_sumcheck_multi_fs(zk_ctx *ctx, size_t count, const void *const *d_e, const void *const *d_f, size_t len,
                         zk_transcript *t, uint64_t *h_out_triples, uint64_t *h_last_e, uint64_t *h_last_f,
                         uint64_t *h_chal_out);
/* Phase 1 of open / d_local_open / c_open (dpoly_comm.rs:309-323 = :337-351 = :418-432):
 * for every round q_i = hi - lo then fold with point[i].  d_q_out receives len-1 Fr: q_0 (len/2)
 * followed by q_1 (len/4) ... q_{n-1} (1) -- exactly the scalar vectors of the n commitments.
 * h_value: the final evaluation. */
int zk_open_rounds(zk_ctx *ctx, const void *d_tab, size_t len, const uint64_t *h_point,
                   void *d_q_out, uint64_t h_value[4]);
/* product tree of acc_product / d_acc_product / c_acc_product (dacc_product.rs:31-38):
 * d_tree receives 2N Fr: tree[0..N) = x, tree[N+j] = tree[2j]*tree[2j+1], tree[2N-1] = 0. */
int zk_product_tree(zk_ctx *ctx, const void *d_x, size_t N, void *d_tree);

/* Several INDEPENDENT calls of the four functions above in one go.  A proof issues them in groups that do not depend on each
 * other -- three product sumchecks and three opens per layer of the wiring identity (hyperplonk/src/dhyperplonk.rs:417-478),
 * the six gate sumchecks (:223-260), the opens of :383-407 -- and most of them are chains of one to three latency-bound
 * launches.  The batch gives every item its own scratch, spreads the items over several streams and waits ONCE; every
 * output is bit-identical to the one-call-at-a-time form (same kernels, same launch plan per item).
 *   mode 0: zk_sumcheck          h_sums 2 log2(len) Fr, h_last_f = the remaining element
 *   mode 1: zk_sumcheck_product  h_sums 3 log2(len) Fr, h_last_f / h_last_g
 *   mode 2: zk_fold              n_points points, d_out receives len >> min(log2 len, n_points) Fr
 *   mode 3: zk_open_rounds       d_out receives the len - 1 quotient elements, h_last_f = the value */
typedef struct {
    int mode;
    const void *d_f;
    const void *d_g;
    size_t len;
    const uint64_t *h_chal;
    size_t n_points;
    uint64_t *h_sums;
    uint64_t *h_last_f;
    uint64_t *h_last_g;
    void *d_out;
} zk_sc_item;
int zk_sumcheck_batch(zk_ctx *ctx, size_t count, const zk_sc_item *items);

/* ---- G1 MSM -------------------------------------------------------------------------- */
/* Upload a base vector once (the reference clones powers_of_g[level] per call, dpoly_comm.rs:258).
 * h_bases: n affine points at `stride` bytes (96 or 104).  The device copy is the library's own:
 * packed at 96 B in its internal Montgomery form, followed by the endomorphism images (beta*x, y) of
 * every point (2 * n * 96 bytes).  Bases must lie in the prime-order subgroup, as arkworks' G1Affine
 * guarantees: the MSM splits scalars as k1 + k2*lambda and phi = [lambda] holds only there. */
int zk_srs_register(zk_ctx *ctx, const void *h_bases, size_t stride, size_t n, zk_srs **out);
/* Same from a device buffer in the packed 96-B reference layout.  The library keeps its own copy in
 * its internal Montgomery form (one conversion pass); the caller's buffer is not referenced afterwards. */
int zk_srs_wrap_device(zk_ctx *ctx, const void *d_bases96, size_t n, zk_srs **out);
/* Synthetic SRS on device: P_i = (k0 + i*k1)*G, the generator G1; mirrors the random-point SRS of
 * PolynomialCommitmentCub::new_single/new_random (dpoly_comm.rs:197-233). k0,k1 canonical 4xu64. */
int zk_srs_generate(zk_ctx *ctx, const uint64_t h_k0[4], const uint64_t h_k1[4], size_t n, zk_srs **out);
/* Structured SRS, PolynomialCommitmentCub::new (dpoly_comm.rs:37-67): out_levels[k], k = 0..nvars, receives
 * powers_of_g[k] = g^{E_k[j]}, E_0 = [1], E_{k+1} = E_k (1 - s_{nvars-k-1}) ++ E_k s_{nvars-k-1}  (2^k points).
 * h_g96: the base in the reference affine layout (NULL: the G1 generator); h_s: nvars Fr (Montgomery).
 * The exponents are expanded in Fr on the device and every point is one fixed-base multiplication. */
int zk_srs_powers(zk_ctx *ctx, const void *h_g96, const uint64_t *h_s, size_t nvars, zk_srs **out_levels);
/* One party's packed level, PolynomialCommitmentCub::to_packed (dpoly_comm.rs:164-194): out[k] = sum_{j<l}
 * row[j] * level[k l + j] with row = this party's row of the pack_from_public matrix (l CANONICAL 4 x u64
 * scalars); a level shorter than l is zero-extended to one chunk. */
int zk_srs_to_packed(zk_ctx *ctx, const zk_srs *level, const uint64_t *h_row, size_t l, zk_srs **out);
/* zk_fr_apply_matrix on G1 points -- the PSS maps are generic over DomainCoeff (pss.rs:93-171; the leader's
 * unpack2 / pack_from_public on commitments, dmsm.rs:30-39): device buffers of affine points in the reference
 * layout (96 B, x = y = 0: infinity), h_matrix = rows*cols CANONICAL 4 x u64 scalars,
 *   out[j*out_vec_stride + r*out_row_stride] = sum_c M[r*cols + c] * in[j*in_vec_stride + c*in_comp_stride]. */
int zk_g1_apply_matrix(zk_ctx *ctx, const uint64_t *h_matrix, size_t rows, size_t cols, const void *d_in96,
                       size_t in_vec_stride, size_t in_comp_stride, void *d_out96, size_t out_vec_stride,
                       size_t out_row_stride, size_t k);
/* Optional, once per SRS level (setup, like uploading it): build the table 2^{o_w} * P_i for every
 * window offset o_w of a `window_bits`-wide signed-digit decomposition (0 = pick for the level's
 * length).  MSMs on this SRS then use ONE bucket set for all windows: 1/W of the bucket-reduction
 * and fix-up work and no cross-window doubling chain.  Costs W x the level's memory (W ~ 13-22 copies).  A G1 table's
 * records are padded from 96 to 128 bytes -- one per cache line: the accumulation's gathers then move one line each, 2^20 MSM
 * +4-7 %, 4/3 of the table memory -- when that leaves at least 60 % of the device free at the moment of the call, and packed
 * (96 bytes) otherwise; zk_srs_precompute_layout forces one form.  window_bits <= 22. */
int zk_srs_precompute(zk_ctx *ctx, zk_srs *srs, int window_bits);
/* The same with the record layout of a G1 table chosen by the caller: record_bytes = 96 (packed), 128 (one record per 128-byte
 * cache line) or 0 (zk_srs_precompute's own choice, by free memory).  Same MSM results.  G2 levels ignore it (192-byte
 * records).  ZK_ERR_INVALID for any other value. */
int zk_srs_precompute_layout(zk_ctx *ctx, zk_srs *srs, int window_bits, int record_bytes);
/* bytes per record of the level's table (0: none built) */
int zk_srs_table_record(const zk_srs *srs);
/* window bits of the level's table (0: none built) -- the MSMs on it insert ceil(256 / bits) digits per scalar */
int zk_srs_table_window(const zk_srs *srs);
int zk_srs_free(zk_ctx *ctx, zk_srs *srs);
size_t zk_srs_len(const zk_srs *srs);
/* the library's device copy (INTERNAL Montgomery form, radix 2^390): for diagnostics only */
const void *zk_srs_device_ptr(const zk_srs *srs);
/* read the bases back in the reference layout (96 B per point, Montgomery radix 2^384) */
int zk_srs_download(zk_ctx *ctx, const zk_srs *srs, void *h_out96);

/* sum_i scalars[i] * bases[offset + i], i < n.  d_scalars: n Fr (Montgomery, as the reference
 * passes them; converted on device like `into_bigint`).  h_out: 18 u64 normalised Jacobian. */
int zk_msm_g1(zk_ctx *ctx, const zk_srs *srs, size_t offset, const void *d_scalars, size_t n,
              uint64_t h_out[18]);
/* A batch of independent MSMs in one pipeline pass -- the shape of d_msm's input
 * (`bases: &Vec<Vec<Affine>>, scalars: &Vec<Vec<Fr>>`, dmsm.rs:9-24; c_open hands it n+2 MSMs of
 * halving size, dpoly_comm.rs:435-436).  Items are grouped by window width and share the launch
 * sequence; all host combines run after ONE synchronisation, in parallel host threads.
 * offsets may be NULL (all zero).  h_out: count x 18 u64. */
int zk_msm_g1_batch(zk_ctx *ctx, size_t count, const zk_srs *const *srs, const size_t *offsets,
                    const void *const *d_scalars, const size_t *n, uint64_t *h_out);
/* Asynchronous form of zk_msm_g1_batch.  Nothing on the reference's path consumes an MSM result on the device (challenges are
 * pre-sampled, hyperplonk/src/dhyperplonk.rs:159-571), so a caller can start the commitments of a protocol step, run the
 * step's sumchecks on the same ctx while they are in flight, and collect the points afterwards.  The job is enqueued on
 * streams of its own (ordered after the work already enqueued on the ctx stream, which produced its scalars) with buffers of
 * its own; consecutive jobs alternate between two sets of streams, so the latency-bound end of one job overlaps with the
 * sort and the accumulation of the next.  The scalar buffers must stay valid and unmodified until zk_msm_wait, which runs the
 * host part, writes count x 18 u64 to h_out and releases the job (also on error). */
typedef struct zk_msm_job zk_msm_job;
int zk_msm_g1_batch_async(zk_ctx *ctx, size_t count, const zk_srs *const *srs, const size_t *offsets,
                          const void *const *d_scalars, const size_t *n, zk_msm_job **job);
int zk_msm_wait(zk_ctx *ctx, zk_msm_job *job, uint64_t *h_out);
/* ---- G2: `d_msm` / `G::msm` are generic over CurveGroup (dmsm.rs:9,23); the reference's parameters carry G2 points
 * in powers_of_g2 (dpoly_comm.rs:27,59-62).  Same pipeline, coordinates in Fq2 = Fq[u]/(u^2 + 1).
 * Layouts (ark-bls12-381): G2Affine = { x: Fq2{c0, c1}, y: Fq2, infinity } -> 192-byte records x.c0|x.c1|y.c0|y.c1,
 * stride 192 or the Rust struct's stride (flag byte at offset 192); results G2Projective = 3 x Fq2 = 36 u64, normalised.
 * zk_srs_download on a G2 vector writes 192-byte records; zk_srs_len / zk_srs_free apply unchanged. */
int zk_srs_register_g2(zk_ctx *ctx, const void *h_bases, size_t stride, size_t n, zk_srs **out);
int zk_msm_g2(zk_ctx *ctx, const zk_srs *srs, size_t offset, const void *d_scalars, size_t n, uint64_t h_out[36]);
int zk_msm_g2_batch(zk_ctx *ctx, size_t count, const zk_srs *const *srs, const size_t *offsets,
                    const void *const *d_scalars, const size_t *n, uint64_t *h_out);
/* Drop-in for `G::msm(&[Affine], &[Fr]) -> Result<G, usize>` on host slices (dmsm.rs:23):
 * returns ZK_ERR_LENGTH when n_bases != n_scalars and stores min(n_bases, n_scalars) in *h_err_len. */
int zk_msm_g1_host(zk_ctx *ctx, const void *h_bases, size_t stride, size_t n_bases,
                   const uint64_t *h_scalars, size_t n_scalars, uint64_t h_out[18], size_t *h_err_len);
/* K9 -- the leader's small public linear maps on points (d_msm closure dmsm.rs:30-39: unpack2 ->
 * sum -> pack_from_public; d_commit/d_open sums dpoly_comm.rs:289-292,372-391): sum_i k_i * P_i
 * for a handful of points.  h_points: n Jacobian points (18 u64 each, any representative),
 * h_scalars: n CANONICAL (non-Montgomery) 4xu64 scalars; h_out normalised Jacobian.  Runs on
 * the host: n is N_p = 8l and the work is one ~255-step dependency chain. */
int zk_g1_lincomb(zk_ctx *ctx, const uint64_t *h_points, const uint64_t *h_scalars, size_t n,
                  uint64_t h_out[18]);
/* `count` combinations with one shared scalar vector: out[r] = sum_i k_i * P[r*n + i]
 * (the per-proof-element sums of d_open, dpoly_comm.rs:372-376); inversions are batched. */
int zk_g1_lincomb_batch(zk_ctx *ctx, const uint64_t *h_points, const uint64_t *h_scalars, size_t n,
                        size_t count, uint64_t *h_out);
/* window size (bits) the device Pippenger picks for n points (2n entries of 128-bit half scalars per
 * window, ceil(129 / bits) windows); 0 < override <= 20 forces it */
int zk_msm_window(size_t n);
int zk_msm_set_window(zk_ctx *ctx, int c_override);
/* per-phase time of the last zk_msm_g1 (first window class of a batch) on this ctx, in ms, HIP
 * events on the ctx stream: [0] digits+sort, [1] k_accum_tiles (bucket accumulation kernel alone),
 * [2] fix-up, [3] bucket reduction + conversion + D2H, [4] host combine (wall), [5] total */
int zk_msm_last_timing(zk_ctx *ctx, float h_ms[6]);

/* device time of the last zk_sumcheck / zk_sumcheck_product / zk_open_rounds call on this ctx, HIP events on the ctx stream,
 * recorded only while the knob "sc_ts" is 3 (ZKHIP_TUNE=sc_ts=3, or zk_dbg_tune of include/zkhip_test.h): [0] the first stage (the first HBM pass of a large table:
 * k_pass<2,1> for the product sumcheck), [1] all launches of the call */
int zk_sumcheck_last_timing(zk_ctx *ctx, float h_ms[2]);

/* ---- party exchanges on one node: an RCCL communicator inside the ctx -------------------------
 * Replaces the typed adapter over mpc-net's TCP star, dist-primitive/src/utils/serializing_net.rs:11-141.
 * The party axis is the GPU axis (party p = rank p); payloads are raw Montgomery limbs in HBM, moved over
 * xGMI with no serialisation or compression; every call is enqueued on the ctx stream (zk_ctx_sync, or any
 * function returning host results, completes it).  RCCL is loaded at run time (librccl.so.1).
 *   serializing_net.rs pattern                               here
 *   worker_send_or_leader_receive_element          :11-39    zk_gather(root = 0)
 *   dynamic_worker_send_or_leader_receive_element  :41-72    zk_gather(root = receiver)
 *   worker_receive_or_leader_send_element          :74-96    zk_scatter(root = 0)
 *   dynamic_worker_receive_or_worker_send_element  :98-122   zk_scatter(root = sender)
 *   leader_compute_element                         :128-141  zk_allgather + the public map on every party
 *   loops of dynamic scatters over every root (dacc_product.rs:94-104,155-203)   zk_alltoall            */
#define ZK_COMM_ID_BYTES 128
/* rank 0 creates the id and hands it to the other parties out of band (once, over any channel) */
int zk_comm_unique_id(uint8_t h_id[ZK_COMM_ID_BYTES]);
/* one process per GPU: collective over all `world` parties */
int zk_comm_init(zk_ctx *ctx, int rank, int world, const uint8_t h_id[ZK_COMM_ID_BYTES]);
/* one process holding a ctx per GPU (the reference's model: one task per party, mpc-net/src/multi.rs:330-352):
 * ctxs[p] becomes party p.  The collectives below block until every party has entered them, so each party's calls
 * must come from ITS OWN host thread (as the reference's parties are separate tasks): driving two parties of one
 * communicator from a single thread deadlocks in the first exchange that returns host results (e.g. zk_d_msm). */
int zk_comm_init_all(zk_ctx *const *ctxs, int world);
int zk_comm_destroy(zk_ctx *ctx); /* also done by zk_ctx_destroy */
/* A party that cannot go on for a reason of its own (an out-of-memory arena, a failed kernel: anything outside the exchanges, which carry
 * their own status words) aborts its communicator (ncclCommAbort) so that its peers' pending and later collectives end with
 * ZK_ERR_COMM instead of waiting for it -- the library's form of the reference's `unwrap()` panic taking the job down
 * (mpc-net/src/multi.rs:330-352).  The ctx is left without a communicator. */
int zk_comm_abort(zk_ctx *ctx);
int zk_comm_rank(const zk_ctx *ctx);
int zk_comm_size(const zk_ctx *ctx);
/* d_recv[p * bytes ..] = party p's d_send, for every p, on every party */
int zk_allgather(zk_ctx *ctx, const void *d_send, size_t bytes, void *d_recv);
/* d_recv[p * bytes ..] = what party p put at d_send[me * bytes ..] */
int zk_alltoall(zk_ctx *ctx, const void *d_send, size_t bytes_per_peer, void *d_recv);
/* root receives world x bytes ordered by party (d_recv is ignored elsewhere) */
int zk_gather(zk_ctx *ctx, const void *d_send, size_t bytes, int root, void *d_recv);
/* party p receives d_send[p * bytes ..] of the root (d_send is ignored elsewhere) */
int zk_scatter(zk_ctx *ctx, const void *d_send, size_t bytes, int root, void *d_recv);
/* d_msm end to end (dmsm.rs:9-43): the batch of local MSMs (:19-24), the gather of the 144-byte results
 * (:29) as ONE all-gather, and the leader closure unpack2 -> sum -> pack_from_public (:30-39) as the public
 * linear map  h_out[k] = sum_i coeffs[i] * C_{i,k}  computed by every party for its own slot.
 * h_coeffs: world x 4 u64 CANONICAL scalars (for party p: coeffs[i] = c_p * lambda_i).  h_lambda (optional,
 * Montgomery): this party's scalars are multiplied by it on the device before its MSM; callers that pass
 * lambda_p = sum_j unpack2[j][p] pass coeffs[i] = c_p for all i (7 additions + one scalar multiplication).
 * h_out: count x 18 u64 normalised Jacobian -- this party's share of every result.
 * Error behaviour: a party whose local MSMs fail (ZK_ERR_LENGTH, ZK_ERR_OOM, ...) still takes part in the exchange and
 * returns its own error; every other party returns ZK_ERR_COMM naming the failed party.  The staging memory of the
 * exchange is taken before the local MSMs, so an out-of-memory party can still publish its status.  A party does NOT
 * join (its peers wait until its communicator is destroyed) only when: it has no communicator / an empty batch; the
 * few-KiB staging allocation itself fails; the HIP runtime or RCCL fails while enqueueing the exchange.
 * The 144-byte results travel pinned host -> device -> all-gather -> pinned host (the last steps of an MSM run on the
 * host, so the points exist there first): two PCIe hops of count x 144 x world bytes per call, see INTEGRATION.md. */
int zk_d_msm(zk_ctx *ctx, size_t count, const zk_srs *const *srs, const size_t *offsets, const void *const *d_scalars,
             const size_t *n, const uint64_t *h_lambda, const uint64_t *h_coeffs, uint64_t *h_out);

/* ---- the BLS12-381 pairing and PolynomialCommitment::verify (dist-primitive/src/dpoly_comm.rs:466-484) ----------------------
 * Inputs: G1 affine 96-byte records (x||y, x = y = 0: infinity), G2 affine 192-byte records at g2_stride (192, or the Rust
 * struct's stride: a nonzero flag byte at offset 192 marks infinity), G1 Jacobian 18 u64 (any representative; the library's
 * results are normalised), Fr 4 u64 Montgomery.  Before anything is launched every point is checked to be canonical and on
 * its curve (ZK_ERR_INVALID otherwise).  Membership in the prime-order subgroups is NOT checked -- as for zk_srs_register it is
 * the caller's responsibility (arkworks' G1Affine / G2Affine guarantee it; zk_g1_check and zk_g2_check below are that check
 * for points from elsewhere); off-subgroup points give meaningless values or verdicts, never a fault or a hang.  A pair with a point at infinity contributes a factor 1.  Every call ends in one
 * synchronisation of the ctx stream.
 *
 * Values: e(P, Q) is the optimal ate Miller value f_{|x|,Q}(P) (|x| = 0xd201000000010000, not conjugated) after the final
 * exponentiation, raised to ZK_PAIRING_EXP_MULTIPLE: f^(3 (q^12 - 1) / r).  3 is coprime to r, so a product of pairings is 1
 * exactly when it is 1 under any other normalisation of the pairing.
 * Output Fq12: ark's Fq12{c0: Fq6{c0, c1, c2: Fq2}, c1: Fq6} -- 72 u64, each Fq 6 u64 in Montgomery form (radix 2^384). */
#define ZK_PAIRING_EXP_MULTIPLE 3
/* e(P_i, Q_i) for count pairs; h_out: count x 72 u64 */
int zk_pairing(zk_ctx *ctx, size_t count, const void *h_g1_96, const void *h_g2, size_t g2_stride, uint64_t *h_out);
/* h_ok[g] = (prod_{h_start[g] <= i < h_start[g+1]} e(P_i, Q_i) == 1), one final exponentiation per group; h_start: groups + 1
 * non-decreasing offsets from 0 (an empty group is 1).  The Miller loops of all pairs run in parallel; the product of a group
 * is taken serially by one lane (one Fq12 multiplication per pair, ~0.1 ms each), so a group of thousands of pairs costs
 * tenths of a second on its own: split very large products into groups of tens of pairs and compare their values instead. */
int zk_pairing_product_check(zk_ctx *ctx, size_t groups, const size_t *h_start, const void *h_g1_96, const void *h_g2,
                             size_t g2_stride, uint8_t *h_ok);
/* the verifying key of PolynomialCommitment: g1 = powers_of_g[0][0] (NULL: the generator), powers_of_g2 = [g2, s_0 g2, ...]
 * (n_g2 >= 1; host copies are kept) */
typedef struct zk_pcs_vk zk_pcs_vk;
int zk_pcs_vk_create(zk_ctx *ctx, const void *h_g1_96, const void *h_powers_g2, size_t g2_stride, size_t n_g2, zk_pcs_vk **out);
int zk_pcs_vk_free(zk_ctx *ctx, zk_pcs_vk *vk);
/* PolynomialCommitment::verify for count openings of nvars-variate polynomials (nvars + 1 <= n_g2, else ZK_ERR_INVALID):
 * commitments count x 18 u64, values count x 4, proofs count x nvars x 18, points count x nvars x 4; h_ok[k] = 1 when
 *   e(C_k - v_k g1, g2) == prod_i e(pi_ki, s_i g2 - u_ki g2),
 * computed as e(A_k, g2) * prod_i e(-pi_ki, s_i g2) == 1 with A_k = C_k - v_k g1 + sum_i u_ki pi_ki. */
int zk_pcs_verify_batch(zk_ctx *ctx, const zk_pcs_vk *vk, size_t nvars, size_t count, const uint64_t *h_commitments,
                        const uint64_t *h_values, const uint64_t *h_proofs, const uint64_t *h_points, uint8_t *h_ok);

/* ---- G1 points from outside: decompression and subgroup membership (csrc/zk_g1check.hip) ----------------------------------------
 * This is the check zk_pairing / zk_pcs_verify_batch leave to their caller.  One device lane per point; a bad point is a STATUS,
 * not an error: both functions return ZK_OK whenever they ran (count = 0 included), ZK_ERR_INVALID only for null pointers with
 * count > 0.  Each call makes one synchronisation of the ctx stream.
 *   status 0  ok: on the curve and in the prime-order subgroup (the point at infinity is a member)
 *          1  bad encoding (zk_g1_check: a coordinate that is not canonical, >= q)
 *          2  x is not the abscissa of a curve point (zk_g1_check: the point is not on the curve)
 *          3  on the curve, not in G1
 * Membership is phi(P) == -[x^2]P with phi(x, y) = (beta x, y), |x| = 0xd201000000010000 (Scott, "A note on group membership
 * tests for G1, G2 and GT on BLS pairing-friendly curves"): two 64-bit scalar multiplications, complete for every input (equal
 * and opposite operands, infinity on the way), constant trip counts. */
#define ZK_G1_OK 0
#define ZK_G1_BAD_ENCODING 1
#define ZK_G1_NOT_ON_CURVE 2
#define ZK_G1_NOT_IN_SUBGROUP 3
/* h_in48: count x 48 bytes, the zcash / arkworks compressed encoding: big-endian x, top three bits of byte 0 = (compressed,
 * infinity, y is the larger root: y > (q - 1) / 2).  Refused with status 1: the compressed bit clear; x >= q; the infinity bit
 * together with any other bit or byte, the sign bit included.  h_out18: count x 18 u64 normalised Jacobian, Montgomery form,
 * (x, y, 1) or (1, 1, 0) for infinity -- what zk_msm_g1 returns; written for status 0 and 3, all zero for status 1 and 2. */
int zk_g1_decompress_check(zk_ctx *ctx, size_t count, const void *h_in48, uint64_t *h_out18, uint8_t *h_status);
/* h_points18: count x 18 u64 Jacobian (X, Y, Z), Montgomery form, any representative; Z = 0 is infinity whatever X and Y are (as
 * in zk_pcs_verify_batch).  The curve equation is checked as Y^2 == X^3 + 4 Z^6: no inversion. */
int zk_g1_check(zk_ctx *ctx, size_t count, const uint64_t *h_points18, uint8_t *h_status);

/* ---- G2 points from outside: decompression and subgroup membership (csrc/zk_g2check.hip) ----------------------------------------
 * The same two calls for the twist E'(Fq2): y^2 = x^3 + 4 (1 + u), whose cofactor has about 507 bits: the keys of a verifying key
 * that comes from a file or another host.  One status byte per point, the values of the G1 calls; ZK_OK whenever the call ran,
 * count = 0 included.  Each call makes one synchronisation of the ctx stream.
 * Membership is psi(P) == [x]P with psi(x, y) = (c_x conj(x), c_y conj(y)), c_x = (1 + u)^(-(q-1)/3), c_y = (1 + u)^(-(q-1)/2), and
 * x = -0xd201000000010000 (Scott, as above): one 64-bit scalar multiplication over Fq2, complete for every input, constant trip
 * counts.  Infinity is a member. */
#define ZK_G2_OK 0
#define ZK_G2_BAD_ENCODING 1
#define ZK_G2_NOT_ON_CURVE 2
#define ZK_G2_NOT_IN_SUBGROUP 3
/* h_in96: count x 96 bytes, the zcash / arkworks compressed encoding: big-endian, x.c1 in bytes 0..47 and x.c0 in bytes 48..95, top
 * three bits of byte 0 = (compressed, infinity, y is the larger of (y, -y): y.c1 > (q - 1) / 2, or y.c1 = 0 and y.c0 > (q - 1) / 2).
 * Refused with status 1: the compressed bit clear; x.c0 >= q or x.c1 >= q; the infinity bit together with any other bit or byte.
 * h_out24: count x 24 u64 affine records x.c0 | x.c1 | y.c0 | y.c1, Montgomery form -- what zk_pairing and zk_pcs_vk_create take;
 * written for status 0 and 3, all zero for status 1 and 2 and for infinity. */
int zk_g2_decompress_check(zk_ctx *ctx, size_t count, const void *h_in96, uint64_t *h_out24, uint8_t *h_status);
/* h_g2: count affine records at g2_stride bytes as zk_pairing takes them (192, or the Rust struct's stride: a nonzero flag byte at
 * offset 192 marks infinity; all zero is infinity).  Status 1: a coordinate >= q; 2: y^2 != x^3 + 4 (1 + u).  g2_stride < 192:
 * ZK_ERR_INVALID. */
int zk_g2_check(zk_ctx *ctx, size_t count, const void *h_g2, size_t g2_stride, uint8_t *h_status);

/* ---- aggregated PCS verification: many openings, one pairing check (csrc/zk_g1seg.hip, csrc/zk_pairing.hip) ----------------------
 * The G2 arguments of PolynomialCommitment::verify are the fixed keys g2, s_0 g2, ..., so any number of openings of mixed variable
 * counts folds into one product of n_g2 pairings with one final exponentiation.  With weights rho_k:
 *     L   = sum_k rho_k ( sum_j e_kj C_kj  -  v_k g1  +  sum_i u_ki pi_ki )
 *     M_j = sum_{k uses key j} rho_k pi_{k, j-1-skip_k}                           j = 1 .. n_g2 - 1
 *     accept  <=>  e(L, g2) prod_j e(-M_j, powers_g2[j]) == 1.
 * The aggregate accepts when every opening holds; when one fails it rejects except with probability about count / 2^128. */
/* out[s] = sum over t in [h_start[s], h_start[s+1]) of k_t * P_t, entirely on the device (h_start: segments + 1 non-decreasing
 * offsets from 0).  h_points18: Jacobian, Montgomery, any representative, Z = 0 is infinity (as zk_g1_check); h_scalars: CANONICAL
 * 4 x u64 (as zk_g1_lincomb); h_out18: normalised Jacobian, (1,1,0) for infinity and for an empty segment (what zk_msm_g1 returns).
 * A term that is not canonical or not on the curve: ZK_ERR_INVALID naming the smallest such term; nothing else is returned.
 * One lane per term (a double-and-add over the bit length of the call's largest scalar, complete additions), a tree in LDS per
 * workgroup of 256 terms, a second launch for segments longer than that; one synchronisation of the ctx stream. */
int zk_g1_lincomb_seg(zk_ctx *ctx, size_t segments, const size_t *h_start, const uint64_t *h_points18, const uint64_t *h_scalars,
                      uint64_t *h_out18);
/* h_ok[0] = 1 iff the aggregate equation above holds.  Opening k: nvars_k variables, proof point i pairs with
 * powers_g2[1 + skip_k + i] (1 + skip_k + nvars_k <= n_g2, else ZK_ERR_INVALID); its commitment is sum_j e_kj C_kj over terms
 * [h_cstart[k], h_cstart[k+1]) (one term with e = 1 is a plain commitment).  Values, points, e: Fr Montgomery as in
 * zk_pcs_verify_batch; proofs / points are the openings' rows one after another.  h_rho: count x 2 u64 (128-bit weights), or NULL:
 * derived by zk_pcs_agg_weights.  count = 0: h_ok[0] = 1, nothing launched.  Points are checked as in zk_pcs_verify_batch (canonical,
 * on the curve; not the subgroup).  One zk_g1_lincomb_seg call and one pairing call: two synchronisations of the ctx stream. */
int zk_pcs_verify_agg(zk_ctx *ctx, const zk_pcs_vk *vk, size_t count, const size_t *h_nvars, const size_t *h_skip,
                      const size_t *h_cstart, const uint64_t *h_cpoints18, const uint64_t *h_cscalars, const uint64_t *h_values,
                      const uint64_t *h_proofs18, const uint64_t *h_points, const uint64_t *h_rho, uint8_t *h_ok);
/* host only, no ctx: the derived weights (Fiat-Shamir over the batch, deterministic).
 *   seed  = SHA-256("zkhip-pcs-agg-v1" || u64le(count) || for each k: u64le(nvars_k) || u64le(skip_k) || u64le(J_k) || its commitment
 *           points || its commitment scalars || value || proof points || point),  every array as the little-endian words given;
 *   rho_k = the first 16 bytes of SHA-256(seed || u64le(k)) as two little-endian u64.
 * ZK_ERR_INVALID: a null array that is read, or commitment offsets that do not start at 0 or decrease. */
int zk_pcs_agg_weights(size_t count, const size_t *h_nvars, const size_t *h_skip, const size_t *h_cstart,
                       const uint64_t *h_cpoints18, const uint64_t *h_cscalars, const uint64_t *h_values, const uint64_t *h_proofs18,
                       const uint64_t *h_points, uint64_t *h_rho);

/* ---- a structured parameter set from a file: validation, expansion and the consistency check on the device (csrc/zk_srsio.hip) -----
 * zk_srs_powers builds powers_of_g from the trapdoor s; a prover that must never see s loads the TOP level L_n (2^n compressed points)
 * and the keys [g2, s_0 g2, .., s_{n-1} g2] from a file instead.  With L_k = powers_of_g[k], for every k < n and j < 2^k
 *     (A)  L_k[j] = L_{k+1}[j] + L_{k+1}[j + 2^k]
 *     (B)  e(L_{k+1}[j + 2^k], g2) = e(L_k[j], s_{n-k-1} g2)
 * so the lower levels are DERIVED by (A) (zk_srs_halve) and (B) is checked per level under random weights (zk_srs_check).  By induction
 * from L_0 = [g], (A) and (B) for all k give L_n[x] = eq(s, x) g for the s the keys define.  This proves that the G1 points are
 * consistent with the G2 keys; it does not prove that nobody knows s. */
/* zk_g1_decompress_check on DEVICE memory, for counts of millions: d_in48: count x 48 bytes, the encoding and the rule of
 * zk_g1_decompress_check (the same device functions); d_out96: count affine records x || y in the reference Montgomery form, as
 * zk_srs_wrap_device takes them, written for status 0 and 3, all zero (the layout's infinity) for every other status and for infinity.
 * Both buffers 16-byte aligned.  flags bit 0: a point at infinity is refused with status 4 (a well-formed SRS holds none); other bits:
 * ZK_ERR_INVALID.  h_result = { the number of points whose status is not 0, the smallest such index (2^64 - 1: none), its status (0:
 * none) }; the index is an atomic minimum and the status is read at that index afterwards, so the report does not depend on the order
 * of the threads.  The kernels walk the points in a grid-stride loop (at most 2048 workgroups of 64 lanes).  ZK_OK whenever the call
 * ran, count = 0 included; one synchronisation of the ctx stream. */
#define ZK_G1_INFINITY_REFUSED 4
int zk_g1_decompress_check_device(zk_ctx *ctx, size_t count, const void *d_in48, void *d_out96, uint32_t flags, uint64_t h_result[3]);
/* (A): out[j] = level[j] + level[j + m], j < m, for a G1 level of 2m points, as a new level (free it with zk_srs_free).  The addition
 * is complete: equal operands are a doubling, and the two halves need not be distinct points.  The sums are normalised with
 * Montgomery's trick, one inversion per lane over a strided group of 64.  A sum at infinity: ZK_ERR_INVALID, zk_last_error gives "K of
 * M sums are the point at infinity; the first is sum J" (no level of a well-formed SRS has one).  A level of 0 points or of an odd
 * number, or a G2 level: ZK_ERR_INVALID.  Blocking. */
int zk_srs_halve(zk_ctx *ctx, const zk_srs *level, zk_srs **out);
/* d_out[j], j < n: the Montgomery form of the low 128 bits of SHA-256(seed (32 bytes) || domain (4 bytes, little-endian) || j (8 bytes,
 * little-endian)).  Byte order: the digest is read as a little-endian 256-bit integer, as the transcript's challenges are, so the low 128
 * bits are its FIRST 16 bytes, byte 0 the least significant.  One lane per element, one compression each.  ASYNCHRONOUS on the ctx
 * stream (the seed is copied before the call returns). */
int zk_fr_hash_expand(zk_ctx *ctx, const uint8_t h_seed32[32], uint32_t domain, size_t n, void *d_out);
/* (B) for every level: levels[k], k = 0 .. n, holds 2^k points (anything else: ZK_ERR_INVALID; 1 <= n <= 30); h_powers_g2: the n + 1
 * keys as zk_pairing takes them.  rho = zk_fr_hash_expand(seed, ZK_SRS_CHECK_DOMAIN, 2^(n-1)); level k uses its first 2^k values (one
 * vector serves every level by the union bound: an error escapes with probability about n / 2^128).  With
 *     A_k = sum_j rho_j levels[k+1][j + 2^k],     B_k = sum_j rho_j levels[k][j]
 * h_ok[k] = ( e(A_k, g2) e(-B_k, powers_g2[n - k]) == 1 ), k < n: the 2n sums are ONE zk_msm_g1_batch (the upper halves through its
 * offsets), the n products ONE zk_pairing_product_check of n groups of two pairs.  A level whose A_k, B_k or key is the point at
 * infinity fails.  The seed must not be known before the points are fixed: the hosts take the SHA-256 of the file.
 * NOT checked here: that the points and the keys lie in the prime-order subgroups -- zk_g1_decompress_check_device and
 * zk_g2_decompress_check do that on the way in from a file; off-subgroup inputs give meaningless verdicts, never a fault. */
#define ZK_SRS_CHECK_DOMAIN 1u
int zk_srs_check(zk_ctx *ctx, const zk_srs *const *levels, size_t n, const void *h_powers_g2, size_t g2_stride,
                 const uint8_t h_seed32[32], uint8_t *h_ok);

/* ---- Poseidon over BLS12-381 Fr: permutation, 2-to-1 hash, Merkle tree (csrc/zk_poseidon.hip) --------------------------------------
 * Width t = 3 (capacity 1, rate 2), S-box x^5, rf full rounds (rf / 2 first, rf / 2 last) around rp partial rounds.  The state is three
 * Fr (s_0, s_1, s_2); one counter k indexes all rf + rp rounds; rc holds 3 (rf + rp) round constants, M is 3 x 3, row-major:
 *     full round k      (k < rf / 2 or k >= rf / 2 + rp):  s_i += rc[3k + i] for i = 0, 1, 2;  every s_i <- s_i^5;  s <- M s
 *     partial round k   (the rp rounds between):            s_i += rc[3k + i] for i = 0, 1, 2;  only  s_0 <- s_0^5;  s <- M s
 *     hash2(l, r) = permute(0, l, r)[0];    a Merkle node = hash2(left child, right child).
 * All values are Montgomery Fr, fully reduced, 32 bytes each; a state is 96 bytes.  Results are exact field elements, so they do not
 * depend on how an implementation groups the arithmetic.
 *
 * The constants are DATA, handed over as a parameter object; t = 3 and the exponent 5 are all that is compiled in.  The project's own
 * instance "zkhip-poseidon-v1" has rf = 8, rp = 57 (the Poseidon paper's round counts for a prime of about 255 bits, t = 3, alpha = 5 and
 * 128-bit security) and
 *     rc[k] = int_le( SHA-256(tag || u32le(k) || 0x00) || SHA-256(tag || u32le(k) || 0x01) ) mod r,  k < 195,  tag = "zkhip-poseidon-v1"
 *     M[i][j] = 1 / (i + j + 3):  a Cauchy matrix on x = 0, 1, 2 and y = 3, 4, 5, hence MDS (every square submatrix is invertible).
 * The hosts build these arrays (zkhip/poseidon.py params(), host/zkhost/poseidon.hpp).  The instance is SELF-DEFINED: it is not claimed
 * to equal the constants of any other library, and the paper's further checks of the matrix (invariant-subspace trails) have NOT been
 * done on it.  That is why the kernels take the constants as a parameter and do not bake them in. */
typedef struct zk_poseidon_params zk_poseidon_params;
/* Device copies of the constants, owned by the object: h_rc 3 (rf + rp) Fr, h_mds 9 Fr, both Montgomery and below r (else
 * ZK_ERR_INVALID).  An odd rf, rf <= 0, rp < 0 or rf + rp > 256: ZK_ERR_INVALID.  Blocking.  The object belongs to ctx and must be
 * freed before it. */
int zk_poseidon_params_create(zk_ctx *ctx, int rf, int rp, const uint64_t *h_rc, const uint64_t *h_mds, zk_poseidon_params **out);
void zk_poseidon_params_free(zk_poseidon_params *params);
/* d_out[i] = permute(d_in[i]), i < n, on states of three Fr (96 bytes, 16-byte aligned).  d_out == d_in is allowed (no other overlap).
 * One lane per state.  ASYNCHRONOUS on the ctx stream; n = 0 is ZK_OK and launches nothing. */
int zk_poseidon_permute(zk_ctx *ctx, const zk_poseidon_params *params, const void *d_in, void *d_out, size_t n);
/* d_out[i] = hash2(d_left[i], d_right[i]), i < n Fr each.  d_out may be d_left or d_right.  ASYNCHRONOUS on the ctx stream. */
int zk_poseidon_hash2(zk_ctx *ctx, const zk_poseidon_params *params, const void *d_left, const void *d_right, void *d_out, size_t n);
/* The Merkle tree of n = 2^k leaves, k >= 0 (anything else: ZK_ERR_INVALID).  d_tree: 2n - 1 Fr in the order of zk_product_tree's
 * levels -- the n leaves, then n / 2 nodes, .., the root at index 2n - 2; node j of a level = hash2(nodes 2j, 2j + 1 of the level
 * below).  d_leaves may be d_tree itself (the leaves already in place).  A level of more nodes than the tuning knob
 * poseidon_tail_nodes (256) is one launch, one lane per node; all levels at or below it are ONE launch of one 256-lane workgroup with a
 * barrier between levels.  No workgroup waits on another, no atomics.  ASYNCHRONOUS on the ctx stream: one copy and the launches are
 * enqueued, the host reads nothing. */
int zk_poseidon_merkle(zk_ctx *ctx, const zk_poseidon_params *params, const void *d_leaves, size_t n, void *d_tree);

/* ---- A Poseidon Merkle tree kept on the device: open, check and update (csrc/zk_poseidon.hip, K32-K36) -----------------------------
 * d_tree is the tree of zk_poseidon_merkle: n = 2^d leaves, 2n - 1 Fr, level j (j = 0: the leaves) at lo_j = 2n - (2n >> j), the root
 * at 2n - 2.  Leaf indices are HOST arrays of uint64_t; the library validates them on the host before anything is enqueued and stages
 * them itself, so no call reads a status back from the device.  A refusal is ZK_ERR_INVALID with a message of the form
 * "K of COUNT indices ..; the first is position P" (P: the smallest offending position in h_index) and enqueues nothing.  The three
 * calls are ordered on the ctx stream like every other call (they wait for the stream once, before their index staging area is
 * reused; the kernels themselves are enqueued and not waited for).  The largest count of every call is ZK_POSEIDON_MERKLE_MAX_COUNT.
 * count = 0 is ZK_OK and enqueues nothing. */
#define ZK_POSEIDON_MERKLE_MAX_COUNT ((size_t)1 << 26)
/* A gather of `count` paths: d_siblings is [count][d] Fr, path k contiguous from the leaf level up,
 *     d_siblings[k * d + j] = d_tree[lo_j + ((h_index[k] >> j) ^ 1)],  j < d.
 * The bits of a path are the bits of its index (bit j set: the running node of level j is the RIGHT child); they are not written.
 * Indices may repeat and come in any order; an index >= n is refused.  n = 1: empty paths, nothing is written.  n as for
 * zk_poseidon_merkle. */
int zk_poseidon_merkle_paths(zk_ctx *ctx, const void *d_tree, size_t n, const uint64_t *h_index, size_t count, void *d_siblings);
/* d_roots[k] = the root of path k: cur = d_leaves[k]; for j < depth: cur = hash2(sib, cur) if bit j of h_index[k] is set, else
 * hash2(cur, sib), sib = d_siblings[k * depth + j].  One lane per path.  depth <= 40; an index with a bit at or above `depth` is
 * refused; depth = 0 copies the leaves.  The caller compares the roots.  d_roots may be d_leaves. */
int zk_poseidon_merkle_roots(zk_ctx *ctx, const zk_poseidon_params *params, const void *d_leaves, const uint64_t *h_index, const void *d_siblings,
                             size_t depth, size_t count, void *d_roots);
/* d_tree[h_index[k]] = d_values[k] for k < count, then exactly the nodes with a written leaf below them are recomputed; every other
 * element of d_tree keeps its bits.  h_index must be STRICTLY ASCENDING (a repeat or a descent is refused with the first offending
 * position, an index >= n likewise): "last write wins" is the business of the caller.  The result is a function of the inputs alone:
 * among the lanes that share a parent the one that hashes is taken from the sorted order (lane k leads at level j when k = 0 or
 * h_index[k - 1] >> (j + 1) differs from its own), never from a race; no atomics, no workgroup waits on another.  Launches: one for
 * the leaf writes; one per level while the level has more than poseidon_tail_nodes distinct parents; then ONE launch of one 256-lane
 * workgroup for all remaining levels, a fence and a barrier between levels.  count = n equals zk_poseidon_merkle of the new leaves.
 * d_values: fully reduced Montgomery Fr, no overlap with d_tree. */
int zk_poseidon_merkle_update(zk_ctx *ctx, const zk_poseidon_params *params, void *d_tree, size_t n, const uint64_t *h_index, const void *d_values,
                              size_t count);

/* ---- Jubjub over BLS12-381 Fr and the Schnorr signature "zkhip-schnorr-v1" (csrc/zk_jubjub.hip, K37-K40) ---------------------------
 * The twisted Edwards curve -x^2 + y^2 = 1 + d x^2 y^2 over Fr with d = -10240 / 10241 (a non-square: the addition law
 *     (x1, y1) + (x2, y2) = ((x1 y2 + y1 x2) / (1 + d x1 x2 y1 y2), (y1 y2 + x1 x2) / (1 - d x1 x2 y1 y2))
 * is complete), identity (0, 1), -(x, y) = (-x, y), cofactor 8, prime subgroup order
 *     l = 0x0e7db4ea6533afa906673b0101343b00a6682093ccc81082d0970e5ed6f72cb7.
 * The generator G is derived by rule: the smallest integer y >= 2 for which x^2 = (y^2 - 1) / (1 + d y^2) is a square (y = 3), the
 * smaller root x, the point times 8.  A point is [2] Fr (x, y), affine, Montgomery, fully reduced, 64 bytes, 16-byte aligned; a
 * coordinate that is not below r makes the point "not on the curve".  A scalar is 4 little-endian uint64_t, a PLAIN integer; every
 * 256-bit value is allowed.  One lane per item, 256-lane workgroups, a grid-stride loop; every loop length is fixed by the call, table
 * entries are selected without branches.  All launches go on the ctx stream; no workgroup waits on another; no atomics but the count
 * and minimum of the refusal below. */
/* d_out[i] = [d_scalars[i]] d_points[i], i < n; d_points = NULL: the fixed base G.  256 double-and-add steps in extended
 * coordinates, one inversion at the end.  Every input point is checked first: if any is not on the curve nothing is written and the
 * call fails with ZK_ERR_INVALID, zk_last_error gives "K of N points are not on the curve; the first is I" (I: the smallest such
 * index, an atomic minimum).  With points the call waits for that check (one synchronisation of the ctx stream) and then enqueues the
 * multiplication; with NULL it is ASYNCHRONOUS.  d_out may be d_points. */
int zk_jubjub_mul(zk_ctx *ctx, const void *d_points, const void *d_scalars, void *d_out, size_t n);
/* d_status[i] (uint32_t), i < n: 0 the point is in the prime-order subgroup (the identity is), 2 it is not on the curve, 3 it is on
 * the curve but [l] P is not the identity -- the numbers of zk_g1_check.  ASYNCHRONOUS on the ctx stream. */
int zk_jubjub_check(zk_ctx *ctx, const void *d_points, uint32_t *d_status, size_t n);
/* Signatures.  Secret key sk in [1, l), public key PK = [sk] G; a signature on a message m (one Fr) is (R, s) with
 *     e = hash2(hash2(hash2(R.x, R.y), hash2(PK.x, PK.y)), m)    (hash2 of `params`; the scalar is e's canonical integer below r,
 *                                                                  not reduced by hand: the group reduces it)
 *     [s] G = R + [e] PK.
 * d_pk: [n][2] Fr, d_msg: [n] Fr, d_sig: [n][3] 32-byte words -- R.x, R.y (Montgomery) and s (a plain 256-bit integer).  d_status[i]
 * (uint32_t) is the FIRST of these that applies: 1 s >= l; 2 PK or R not on the curve; 3 PK outside the subgroup, or PK the identity;
 * 4 the equation fails (a message that is not below r also gives 4); 0 valid.  There is no cofactor multiplication: an R with a
 * torsion part fails the equality.  One lane per signature: four permutations, the subgroup test [l] PK and ONE joint double-and-add
 * of 255 steps over the bits of s and e with the table {O, G, -PK, G - PK}, compared with R projectively (no inversion).  Signing is
 * host code (zkhip/jubjub.py).  ASYNCHRONOUS on the ctx stream. */
int zk_schnorr_verify(zk_ctx *ctx, const zk_poseidon_params *params, const void *d_pk, const void *d_msg, const void *d_sig, uint32_t *d_status,
                      size_t n);

/* (the zk_dbg_* test hooks of the library are declared in include/zkhip_test.h: they are not part of this surface) */

#ifdef __cplusplus
}
#endif
#endif /* ZKHIP_H */
