/* zkhip_test.h -- TEST HOOKS of libzkhip.so, NOT ABI.
 *
 * The zk_dbg_* entry points exist for tests/ and tools/ only.  They are not part of the drop-in surface of include/zkhip.h: a
 * reference-side binding must not bind them (rust/zkhip_sys.rs is generated from zkhip.h alone and does not carry them), the
 * Python host resolves them only when a test or a tool asks (zkhip._lib.test_hooks()), and they may change or disappear
 * between versions. */
#ifndef ZKHIP_TEST_H
#define ZKHIP_TEST_H
#include "zkhip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Process-wide experiment / diagnostics knobs (csrc/zk_ctx.hpp `struct Tuning` lists them; the same keys are read once
 * from ZKHIP_TUNE="key=value,..."): e.g. "sc_t1_device" = 1 makes the product sumcheck compute t1 = sum f_hi g_hi of
 * EVERY round on the device instead of deriving it from the previous round polynomial (the cross-check of
 * tests/test_gpu_bigsizes.py).  Returns ZK_ERR_INVALID for an unknown key. */
int zk_dbg_tune(const char *key, long value);
/* the current value of a knob (so that a test can put back what it found); ZK_ERR_INVALID for an unknown key or a null pointer */
int zk_dbg_tune_get(const char *key, long *value);
int zk_dbg_fq_mul(zk_ctx *ctx, const void *d_a, const void *d_b, void *d_out, size_t n);
int zk_dbg_fq_add(zk_ctx *ctx, const void *d_a, const void *d_b, void *d_out, size_t n);
int zk_dbg_fq_sub(zk_ctx *ctx, const void *d_a, const void *d_b, void *d_out, size_t n);
/* a*b + b*b through the fused two-product multiplication (one Montgomery reduction) */
int zk_dbg_fq_mul2add(zk_ctx *ctx, const void *d_a, const void *d_b, void *d_out, size_t n);
/* device XYZZ formulas on pairs of packed affine points; h_out[i] = 18 u64 normalised Jacobian.
 * mode 0: p+q (mixed add)  1: (p+q)+p (full add)  2: (p+q)+(p+q) (doubling path)  3: p-q */
int zk_dbg_g1_op(zk_ctx *ctx, int mode, const void *d_p96, const void *d_q96, void *h_out, size_t n);

/* the G2 formulas on pairs of affine points (192 B, reference form); h_out[i] = 36 u64 normalised Jacobian.
 * mode 0: p+q  1: (p+q)+p  2: (p+q)+(p+q) (full-addition doubling path)  3: p-q  4: 2(p+q) (doubling)  5: (p+q)-(p+q) */
int zk_dbg_g2_op(zk_ctx *ctx, int mode, const void *d_p192, const void *d_q192, void *h_out, size_t n);

/* The XYZZ group formulas of the MSM (csrc/curve30.cuh for G1, csrc/curve30_g2.cuh for G2: zk_dbg_xyzz2_op) one operation at a time, at
 * chosen representatives.  d_a, d_b: n operands of four coordinates X, Y, ZZ, ZZZ, each an integer below q in 48 bytes little-endian,
 * re-limbed as they are (no Montgomery conversion); for G2 eight integers per operand, c0 then c1 of every coordinate.  d_lift_a,
 * d_lift_b: n u32, one nibble per coordinate from bit 0 up (per component for G2): the coordinate becomes value + k q by additions of q,
 * k clamped to what the invariant X < 8q, Y < 4q, ZZ < 2q, ZZZ < 2q allows (7, 3, 1, 1).  ZZ = 0 with lift 0 is infinity.  d_out: the raw
 * result, 13 u32 limbs per coordinate (per component) at a 64-byte stride, 256 B (G2: 512 B) per element; nothing is reduced or normalised.
 * d_rep: n u32 (mode 6 only, may be null otherwise).  All pointers are device memory.
 * mode 0: madd(acc = a, p = (b.X, b.Y))   1: the same with neg   (b with lift 0: the affine operand)
 *      2: add(a, b)   3: dbl(a)   4: dbl_affine(a.X, a.Y)   (3, 4 do not read d_b, d_lift_b: may be null)
 *      5: add_quad, four lanes per element: a_i is stored at index i and b_i at index N + i (N = n rounded up to 64) of a scratch array in
 *         the blocked 64-point chunk layout, the sums are read back with xyzz30_load / xyzz2_load
 *      6: acc_quad, four lanes per element: acc = a_i, then d_rep[i] (at most 3) times acc += b_i from the same scratch array
 * ZK_ERR_INVALID for an unknown mode or a null pointer, before any launch. */
int zk_dbg_xyzz_op(zk_ctx *ctx, int mode, const void *d_a, const void *d_lift_a, const void *d_b, const void *d_lift_b, const void *d_rep,
                   void *d_out, size_t n);
int zk_dbg_xyzz2_op(zk_ctx *ctx, int mode, const void *d_a, const void *d_lift_a, const void *d_b, const void *d_lift_b, const void *d_rep,
                    void *d_out, size_t n);

/* The Fq layer of the pairing (csrc/fq30.cuh: 13 limbs of 30 bits, lazily reduced) at chosen representatives.  d_x, d_y: n integers
 * below q, 48 bytes little-endian, re-limbed as they are (no Montgomery conversion); d_kx, d_ky: n u32 <= 15.  Lane i works on
 * a = x + kx q and b = y + ky q (built by additions of q, so every representative below 16q).  d_out: 13 u32 limbs of the raw result
 * per element at a 64-byte stride; d_flags: n u32, bit 0 = limbs 0..11 of the result are below 2^30.  All pointers are device memory.
 * mode 0..7: csub_q, csub_2q, csub_4q, csub_8q, red4, red8, red16, canon8 (a only: d_y, d_ky may be null)
 *      8..12: sub2, sub4, sub6, sub8, sub12 (a + K q - b)   13: add   14: add2x (a + 2b)
 *      15: mul   16: sqr (a only)   17: mul2add (a b + b a)   18: inv (a only; 0 -> 0) */
int zk_dbg_fq30_op(zk_ctx *ctx, int mode, const void *d_x, const void *d_kx, const void *d_y, const void *d_ky, void *d_out, void *d_flags,
                   size_t n);

/* The Fq2 / Fq6 / Fq12 tower of the pairing (csrc/fq12.cuh, csrc/zk_pairing.hip) one operation at a time.  d_a, d_b: n x 576 bytes in
 * ark's layout (what zk_pairing returns); d_lift: n u32, bits 0..11 add q to those components of a after the conversion to the
 * internal form, bits 12..23 to those of b (the residue stays, the representative becomes < 2q: the largest the tower's bound rule
 * allows).  d_out: n x 576 bytes, ark's layout.  d_flags: n u32 taken on the value the function returned, before it is converted
 * back: bit 0 = limbs 0..11 of every component below 2^30, bit 1 = every component below 2q.  All pointers are device memory.
 * mode 0: mul  1: sqr  2: cyc_sqr  3: inv  4: conj  5..7: frob1..3  8: mul_by_014 (the line's c0, c1, c4 = b's c0.c0, c0.c1, c1.c1)
 *      9: exp_by_x  10: final_exp  11: f6_mul  12: f6_inv (on the c0 halves; the result's c1 is zero)
 *      13: f2_mul  14: f2_sqr  15: f2_inv (on c0.c0; the other components of the result are zero)
 * Unary modes do not read d_b (may be null). */
int zk_dbg_fq12_op(zk_ctx *ctx, int mode, const void *d_a, const void *d_b, const void *d_lift, void *d_out, void *d_flags, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* ZKHIP_TEST_H */
