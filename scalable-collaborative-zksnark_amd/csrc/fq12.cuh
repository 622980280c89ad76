// fq12.cuh -- BLS12-381 Fq6 = Fq2[v] / (v^3 - xi), xi = 1 + u, and Fq12 = Fq6[w] / (w^2 - v) on the unsaturated field of fq30.cuh
// and the Fq2 of curve30_g2.cuh: arkworks' tower, the target group of the device pairing (zk_pairing.hip).
//
// The same tower as zkhip/pairing.py's Fq[w] / (w^12 - 2 w^6 + 2) with v = w^2 and u = w^6 - 1: sum a_ij w^i v^j <-> w^(i + 2 j).
//
// Bound rule.  Every Fq2 / Fq6 / Fq12 value handed from one function to another has normalised components < 2q.  Inside a
// function sums grow (< 4q, < 6q, ...) and are brought back below 2q by conditional subtractions (f30_red4 / red8 / red16: 40
// instructions per step against ~600 of one multiplication).  Multiplications are curve30_g2.cuh's f2_mul<8> / f2_sqr<8>:
// operands < 8q, bound 8 * (8 + 8) = 128 <= 256, result < 2q.
//
// Register pressure.  An Fq12 is 156 VGPRs; the multiplies are __noinline__ so that a kernel holds at most a few of them live and
// the code of the ~15 k Fq products of a pairing is emitted a handful of times, not per call site.
#pragma once
#include "curve30.cuh"  // (f30_neg_canon, used by curve30_g2.cuh)
#include "curve30_g2.cuh"
#include "pairing_consts.cuh"

namespace zk {

struct Fq6x {
    Fq2x c0, c1, c2;
};
struct Fq12x {
    Fq6x c0, c1;
};

// ---- Fq: conditional reductions --------------------------------------------------------------------------------------------------
__device__ __forceinline__ Fq30 f30_csub_8q(const Fq30& v) {  // v - 8q if v >= 8q
    Fq30 d, r;
    u32 bw = 0;
#pragma unroll
    for (int i = 0; i < 13; i++) {
        u32 x = v.l[i] - pc::Q8[i] - bw;
        bw = x >> 31;
        d.l[i] = (i < 12) ? (x & Q30::MASK) : x;
    }
#pragma unroll
    for (int i = 0; i < 13; i++) r.l[i] = bw ? v.l[i] : d.l[i];
    return r;
}
__device__ __forceinline__ Fq30 f30_red4(const Fq30& v) { return f30_csub_2q(v); }                 // < 4q  -> < 2q
__device__ __forceinline__ Fq30 f30_red8(const Fq30& v) { return f30_csub_2q(f30_csub_4q(v)); }    // < 8q  -> < 2q
__device__ __forceinline__ Fq30 f30_red16(const Fq30& v) { return f30_red8(f30_csub_8q(v)); }      // < 16q -> < 2q
__device__ __forceinline__ Fq30 f30_c(const u32 (&t)[13]) {
    Fq30 r;
#pragma unroll
    for (int i = 0; i < 13; i++) r.l[i] = t[i];
    return r;
}

// ---- Fq2 (inputs < 2q, outputs < 2q unless noted) ----------------------------------------------------------------------------------
__device__ __forceinline__ Fq2x f2_r4(const Fq2x& a) { return Fq2x{f30_red4(a.c0), f30_red4(a.c1)}; }
__device__ __forceinline__ Fq2x f2_r8(const Fq2x& a) { return Fq2x{f30_red8(a.c0), f30_red8(a.c1)}; }
__device__ __forceinline__ Fq2x f2_r16(const Fq2x& a) { return Fq2x{f30_red16(a.c0), f30_red16(a.c1)}; }
__device__ __forceinline__ Fq2x f2_addr(const Fq2x& a, const Fq2x& b) { return f2_r4(f2_add(a, b)); }
__device__ __forceinline__ Fq2x f2_subr(const Fq2x& a, const Fq2x& b) { return f2_r4(f2_sub2(a, b)); }  // a + 2q - b < 4q
__device__ __forceinline__ Fq2x f2_negr(const Fq2x& a) { return f2_r4(f2_sub2(f2_zero(), a)); }
__device__ __forceinline__ Fq2x f2_dblr(const Fq2x& a) { return f2_addr(a, a); }
// t - x - y for t, x, y < 2q: t + 4q - (x + y) < 6q
__device__ __forceinline__ Fq2x f2_sub_pair(const Fq2x& t, const Fq2x& x, const Fq2x& y) { return f2_r8(f2_sub4(t, f2_add(x, y))); }
// a * xi = (a0 - a1) + (a0 + a1) u
__device__ __forceinline__ Fq2x f2_xir(const Fq2x& a) { return Fq2x{f30_red4(f30_sub2(a.c0, a.c1)), f30_red4(f30_add(a.c0, a.c1))}; }
__device__ __forceinline__ Fq2x f2_conj(const Fq2x& a) { return Fq2x{a.c0, f30_red4(f30_sub2(f30_zero(), a.c1))}; }
// operands < 8q
__device__ __forceinline__ Fq2x f2_mulr(const Fq2x& a, const Fq2x& b) { return f2_mul<8>(a, b); }
__device__ __forceinline__ Fq2x f2_sqrr(const Fq2x& a) { return f2_sqr<8>(a); }
// a (< 8q) times s in Fq (< 2q): 8 * 2 <= 256
__device__ __forceinline__ Fq2x f2_mul_fq(const Fq2x& a, const Fq30& s) { return Fq2x{f30_mul(a.c0, s), f30_mul(a.c1, s)}; }
__device__ __forceinline__ Fq2x f2_c(const u32 (&c0)[13], const u32 (&c1)[13]) { return Fq2x{f30_c(c0), f30_c(c1)}; }
// 1 / a = conj(a) / (a0^2 + a1^2); 0 -> 0
__device__ __forceinline__ Fq2x f2_inv(const Fq2x& a) {
    const Fq30 n = f30_inv(f30_mul2add(a.c0, a.c0, a.c1, a.c1));  // 2 * 2 + 2 * 2; < 2q
    return Fq2x{f30_mul(a.c0, n), f30_red4(f30_sub2(f30_zero(), f30_mul(a.c1, n)))};
}

// ---- Fq6 ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ Fq6x f6_zero() { return Fq6x{f2_zero(), f2_zero(), f2_zero()}; }
__device__ __forceinline__ Fq6x f6_one() { return Fq6x{f2_one(), f2_zero(), f2_zero()}; }
__device__ __forceinline__ Fq6x f6_addr(const Fq6x& a, const Fq6x& b) { return Fq6x{f2_addr(a.c0, b.c0), f2_addr(a.c1, b.c1), f2_addr(a.c2, b.c2)}; }
__device__ __forceinline__ Fq6x f6_subr(const Fq6x& a, const Fq6x& b) { return Fq6x{f2_subr(a.c0, b.c0), f2_subr(a.c1, b.c1), f2_subr(a.c2, b.c2)}; }
__device__ __forceinline__ Fq6x f6_negr(const Fq6x& a) { return Fq6x{f2_negr(a.c0), f2_negr(a.c1), f2_negr(a.c2)}; }
__device__ __forceinline__ Fq6x f6_sub_pair(const Fq6x& t, const Fq6x& x, const Fq6x& y) {
    return Fq6x{f2_sub_pair(t.c0, x.c0, y.c0), f2_sub_pair(t.c1, x.c1, y.c1), f2_sub_pair(t.c2, x.c2, y.c2)};
}
__device__ __forceinline__ Fq6x f6_mul_v(const Fq6x& a) { return Fq6x{f2_xir(a.c2), a.c0, a.c1}; }  // a v
// Karatsuba over Fq2: 6 Fq2 multiplications (operand sums < 4q)
__device__ __noinline__ Fq6x f6_mul(Fq6x a, Fq6x b) {
    const Fq2x v0 = f2_mulr(a.c0, b.c0), v1 = f2_mulr(a.c1, b.c1), v2 = f2_mulr(a.c2, b.c2);
    Fq6x r;
    r.c0 = f2_addr(v0, f2_xir(f2_sub_pair(f2_mulr(f2_add(a.c1, a.c2), f2_add(b.c1, b.c2)), v1, v2)));
    r.c1 = f2_addr(f2_sub_pair(f2_mulr(f2_add(a.c0, a.c1), f2_add(b.c0, b.c1)), v0, v1), f2_xir(v2));
    r.c2 = f2_addr(f2_sub_pair(f2_mulr(f2_add(a.c0, a.c2), f2_add(b.c0, b.c2)), v0, v2), v1);
    return r;
}
__device__ __forceinline__ Fq6x f6_inv(const Fq6x& a) {
    const Fq2x t0 = f2_subr(f2_sqrr(a.c0), f2_xir(f2_mulr(a.c1, a.c2)));
    const Fq2x t1 = f2_subr(f2_xir(f2_sqrr(a.c2)), f2_mulr(a.c0, a.c1));
    const Fq2x t2 = f2_subr(f2_sqrr(a.c1), f2_mulr(a.c0, a.c2));
    const Fq2x n = f2_addr(f2_mulr(a.c0, t0), f2_xir(f2_addr(f2_mulr(a.c2, t1), f2_mulr(a.c1, t2))));
    const Fq2x ni = f2_inv(n);
    return Fq6x{f2_mulr(t0, ni), f2_mulr(t1, ni), f2_mulr(t2, ni)};
}

// ---- Fq12 --------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ Fq12x f12_one() { return Fq12x{f6_one(), f6_zero()}; }
__device__ __forceinline__ Fq12x f12_conj(const Fq12x& a) { return Fq12x{a.c0, f6_negr(a.c1)}; }  // a^(q^6); the inverse on the cyclotomic subgroup
// Karatsuba over Fq6: 3 Fq6 multiplications
__device__ __noinline__ Fq12x f12_mul(Fq12x a, Fq12x b) {
    const Fq6x v0 = f6_mul(a.c0, b.c0), v1 = f6_mul(a.c1, b.c1);
    const Fq6x t = f6_mul(f6_addr(a.c0, a.c1), f6_addr(b.c0, b.c1));
    return Fq12x{f6_addr(v0, f6_mul_v(v1)), f6_sub_pair(t, v0, v1)};
}
// (a0 + a1 w)^2 = (a0 + a1)(a0 + v a1) - a0 a1 - v a0 a1 + 2 a0 a1 w: 2 Fq6 multiplications
__device__ __noinline__ Fq12x f12_sqr(Fq12x a) {
    const Fq6x ab = f6_mul(a.c0, a.c1);
    const Fq6x t = f6_mul(f6_addr(a.c0, a.c1), f6_addr(a.c0, f6_mul_v(a.c1)));
    return Fq12x{f6_sub_pair(t, ab, f6_mul_v(ab)), f6_addr(ab, ab)};
}
// f * (c0 + c1 v + c4 v w): the line of the M-twist Miller loop (nonzero slots c0.c0, c0.c1, c1.c1).  15 Fq2 multiplications.
__device__ __noinline__ Fq12x f12_mul_by_014(Fq12x f, Fq2x c0, Fq2x c1, Fq2x c4) {
    const Fq6x& a = f.c0;
    const Fq6x& b = f.c1;
    Fq6x aa, bb, t;
    aa.c0 = f2_addr(f2_mulr(a.c0, c0), f2_xir(f2_mulr(a.c2, c1)));  // a (c0 + c1 v)
    aa.c1 = f2_addr(f2_mulr(a.c0, c1), f2_mulr(a.c1, c0));
    aa.c2 = f2_addr(f2_mulr(a.c1, c1), f2_mulr(a.c2, c0));
    bb.c0 = f2_xir(f2_mulr(b.c2, c4));  // b (c4 v)
    bb.c1 = f2_mulr(b.c0, c4);
    bb.c2 = f2_mulr(b.c1, c4);
    const Fq6x s = f6_addr(a, b);
    const Fq2x o = f2_addr(c1, c4);
    t.c0 = f2_addr(f2_mulr(s.c0, c0), f2_xir(f2_mulr(s.c2, o)));  // (a + b)(c0 + (c1 + c4) v)
    t.c1 = f2_addr(f2_mulr(s.c0, o), f2_mulr(s.c1, c0));
    t.c2 = f2_addr(f2_mulr(s.c1, o), f2_mulr(s.c2, c0));
    return Fq12x{f6_addr(aa, f6_mul_v(bb)), f6_sub_pair(t, aa, bb)};
}
// a^(q^K): coefficient of w^e (e = i + 2 j) -> conj^K(b_e) * gamma_{K,e}
template <int K>
__device__ __noinline__ Fq12x f12_frob(Fq12x a) {
    auto one = [](const Fq2x& b, int e) {
        const Fq2x c = (K & 1) ? f2_conj(b) : b;
        return e == 0 ? c : f2_mulr(c, f2_c(pc::FROB[K - 1][e - 1][0], pc::FROB[K - 1][e - 1][1]));
    };
    Fq12x r;
    r.c0.c0 = one(a.c0.c0, 0);
    r.c0.c1 = one(a.c0.c1, 2);
    r.c0.c2 = one(a.c0.c2, 4);
    r.c1.c0 = one(a.c1.c0, 1);
    r.c1.c1 = one(a.c1.c1, 3);
    r.c1.c2 = one(a.c1.c2, 5);
    return r;
}
// 1 / (a0 + a1 w) = (a0 - a1 w) / (a0^2 - v a1^2); 0 -> 0
__device__ __noinline__ Fq12x f12_inv(Fq12x a) {
    const Fq6x t = f6_inv(f6_subr(f6_mul(a.c0, a.c0), f6_mul_v(f6_mul(a.c1, a.c1))));
    return Fq12x{f6_mul(a.c0, t), f6_negr(f6_mul(a.c1, t))};
}
// squaring in the cyclotomic subgroup (Granger-Scott, "Faster squaring in the cyclotomic subgroup of sixth degree extensions",
// PKC 2010): Fq12 = Fq4[w] over Fq4 = Fq2[w^3], three Fq4 squarings = 6 Fq2 multiplications (f12_sqr: 12).
// Valid only for a^(q^6 + 1)(q^2 - 1)... = elements of norm 1, i.e. after the easy part of the final exponentiation.
__device__ __forceinline__ void f4_sqr(const Fq2x& a, const Fq2x& b, Fq2x& t0, Fq2x& t1) {  // (a + b y)^2, y^2 = xi
    const Fq2x t = f2_mulr(a, b);
    t0 = f2_sub_pair(f2_mulr(f2_add(a, b), f2_add(f2_xir(b), a)), t, f2_xir(t));  // a^2 + xi b^2
    t1 = f2_dblr(t);
}
__device__ __forceinline__ Fq2x f2_3t_m2z(const Fq2x& t, const Fq2x& z) {  // 3t - 2z: 3t + 4q - 2z < 10q
    return f2_r16(f2_sub4(f2_add(f2_add(t, t), t), f2_add(z, z)));
}
__device__ __forceinline__ Fq2x f2_3t_p2z(const Fq2x& t, const Fq2x& z) {  // 3t + 2z < 10q
    return f2_r16(f2_add(f2_add(f2_add(t, t), t), f2_add(z, z)));
}
__device__ __noinline__ Fq12x f12_cyc_sqr(Fq12x f) {
    const Fq2x &r0 = f.c0.c0, &r4 = f.c0.c1, &r3 = f.c0.c2, &r2 = f.c1.c0, &r1 = f.c1.c1, &r5 = f.c1.c2;
    Fq2x t0, t1, t2, t3, t4, t5;
    f4_sqr(r0, r1, t0, t1);
    f4_sqr(r2, r3, t2, t3);
    f4_sqr(r4, r5, t4, t5);
    Fq12x z;
    z.c0.c0 = f2_3t_m2z(t0, r0);
    z.c1.c1 = f2_3t_p2z(t1, r1);
    z.c1.c0 = f2_3t_p2z(f2_xir(t5), r2);
    z.c0.c2 = f2_3t_m2z(t4, r3);
    z.c0.c1 = f2_3t_m2z(t2, r4);
    z.c1.c2 = f2_3t_p2z(t3, r5);
    return z;
}

// ---- loads / stores: an Fq12 is 12 Fq in ark's order (c0.c0.c0, c0.c0.c1, c0.c1.c0, ..., c1.c2.c1), 48 bytes each -----------------
__device__ __forceinline__ Fq30& f12_at(Fq12x& a, int k) {
    Fq6x& h = (k < 6) ? a.c0 : a.c1;
    Fq2x& c = ((k % 6) < 2) ? h.c0 : ((k % 6) < 4) ? h.c1 : h.c2;
    return (k & 1) ? c.c1 : c.c0;
}
__device__ __forceinline__ Fq12x f12_load(const void* base, size_t idx) {
    Fq12x a;
#pragma unroll
    for (int k = 0; k < 12; k++) f12_at(a, k) = f30_load(base, idx * 576 + 48 * k);
    return a;
}
__device__ __forceinline__ void f12_store(void* base, size_t idx, Fq12x a) {
#pragma unroll
    for (int k = 0; k < 12; k++) f30_store(base, idx * 576 + 48 * k, f12_at(a, k));
}

}  // namespace zk
