// g1c.cuh -- what the one-lane-per-point kernels share (zk_g1check.hip, zk_g2check.hip: validation; zk_g1seg.hip: segmented linear
// combination; zk_srsio.hip: parameter sets from a file): the Fq constants, the canonical-coordinate and sign tests, the complete G1 XYZZ
// doubling / addition with the doubling inlined, and the two rules of G1 validation -- decompression of a 48-byte record and Scott's
// membership test -- as lane functions, so that every kernel that validates points runs the same text.
#pragma once
#include "curve30.cuh"

namespace zk {

namespace g1c {
__host__ __device__ constexpr u32 FOUR(int i) {  // 4 (the curve's b), internal form
    constexpr u32 t[13] = {0x0347fcb8u, 0x27600000u, 0x12002b11u, 0x3803379bu, 0x090c7212u, 0x1a7e0e88u, 0x373e0376u, 0x26d0b683u, 0x17bb09b0u, 0x17663c4au, 0x12ca7c51u, 0x167f3e80u, 0x000577a6u};
    return t[i];
}
__host__ __device__ constexpr u32 R2(int i) {  // 2^780 mod q: canonical integer -> internal form (x 2^390)
    constexpr u32 t[13] = {0x0510070fu, 0x3b19070du, 0x0132243au, 0x299bb0e8u, 0x3507af6eu, 0x3b81ec77u, 0x21b145efu, 0x0a487bb4u, 0x370a4144u, 0x05dcb4cbu, 0x18c97900u, 0x3812b364u, 0x000f696eu};
    return t[i];
}
__host__ __device__ constexpr u32 HALF(int i) {  // (q - 1) / 2, a plain integer
    constexpr u32 t[13] = {0x3fffd555u, 0x33fdffffu, 0x0a9ffffdu, 0x157fffd6u, 0x187b120fu, 0x21a541edu, 0x2895fb39u, 0x29709e70u, 0x166bb23bu, 0x0f6c8697u, 0x34d258ddu, 0x3d472ffcu, 0x000d0088u};
    return t[i];
}
// beta = 0x5f19672fdf76ce51ba69c6076a0f77eaddb3a93be6f89688de17d813620a00022e01fffffffefffe, internal form: the cube root of unity whose
// endomorphism is multiplication by -x^2 on G1 (the other one belongs to x^2 - 1)
__host__ __device__ constexpr u32 BETA(int i) {
    constexpr u32 t[13] = {0x229d39fcu, 0x11661b79u, 0x3a68a8f8u, 0x09dabbd8u, 0x12744b7eu, 0x22bc97d4u, 0x3c5ccd3eu, 0x1cf87540u, 0x0197e4f4u, 0x3433d1ecu, 0x0d20861fu, 0x33953662u, 0x000edc53u};
    return t[i];
}
// (q + 1) / 4 in 32-bit words, 379 bits
static __device__ const u32 kSqrtExp[12] = {0xffffeaabu, 0xee7fbfffu, 0xac54ffffu, 0x07aaffffu, 0x3dac3d89u, 0xd9cc34a8u, 0x3ce144afu, 0xd91dd2e1u, 0x90d2eb35u, 0x92c6e9edu, 0x8e5ff9a6u, 0x0680447au};
constexpr int kSqrtBits = 379;
constexpr unsigned long long kXAbs = 0xd201000000010000ULL;
enum : unsigned char { kOk = 0, kBadEncoding = 1, kNotOnCurve = 2, kNotInG1 = 3 };
}  // namespace g1c

#define ZK_G1C_CONST(name, T)                                    \
    __device__ __forceinline__ Fq30 name() {                     \
        Fq30 r;                                                  \
        _Pragma("unroll") for (int i = 0; i < 13; i++) r.l[i] = T(i); \
        return r;                                                \
    }
ZK_G1C_CONST(g1c_four, g1c::FOUR)
ZK_G1C_CONST(g1c_r2, g1c::R2)
ZK_G1C_CONST(g1c_one_ref, Q30::C384)  // 2^384 mod q: the reference form of 1
ZK_G1C_CONST(g1c_beta, g1c::BETA)

// v < q for a normalised v < 2^384
__device__ __forceinline__ bool g1c_lt_q(const Fq30& v) {
    u32 bw = 0;
#pragma unroll
    for (int i = 0; i < 13; i++) bw = (v.l[i] - Q30::Q(i) - bw) >> 31;
    return bw != 0;
}
__device__ __forceinline__ bool g1c_same(const Fq30& a, const Fq30& b) {  // canonical operands
    u32 o = 0;
#pragma unroll
    for (int i = 0; i < 13; i++) o |= a.l[i] ^ b.l[i];
    return o == 0;
}

// 2p (dbl-2008-s-1, a = 0) and a + b below: the formulas of xyzz30_dbl / xyzz30_add of curve30.cuh, inlined.  There the doubling is a rare
// path behind a call (__noinline__); here it IS the hot path.  k_g1_subgroup built on the curve30.cuh pair takes 255 VGPRs + 105 AGPRs
// and 640 bytes of scratch per lane (the call's stack frame); with these two it takes 256 + 21 and none.  A change of either
// formula must be made in both files; tests/test_gpu_g1check.py (this copy) and tests/test_gpu_xyzz.py (that one) check each against a model.
__device__ __forceinline__ Xyzz30 g1c_dbl(const Xyzz30& p) {
    if (xyzz30_is_inf(p)) return p;
    Xyzz30 r;
    const Fq30 U = f30_add(p.y, p.y);               // < 8q
    const Fq30 V = f30_sqr(U);
    const Fq30 W = f30_mul(U, V);
    const Fq30 S = f30_mul(p.x, V);                 // 8q * 2q
    const Fq30 xx = f30_sqr(p.x);                   // 64 q^2
    const Fq30 M = f30_add(f30_add(xx, xx), xx);    // < 6q
    const Fq30 X3 = f30_sub4(f30_sqr(M), f30_add(S, S));  // < 6q
    r.y = f30_sub2(f30_mul(M, f30_sub8(S, X3)), f30_mul(W, p.y));  // < 4q
    r.x = X3;
    r.zz = f30_mul(V, p.zz);
    r.zzz = f30_mul(W, p.zzz);
    return r;
}
// a + b (add-2008-s), complete: xyzz30_add of curve30.cuh with the doubling inlined
__device__ __forceinline__ Xyzz30 g1c_add(const Xyzz30& a, const Xyzz30& b) {
    if (xyzz30_is_inf(a)) return b;
    if (xyzz30_is_inf(b)) return a;
    const Fq30 U1 = f30_mul(a.x, b.zz);       // 8q * 2q
    const Fq30 U2 = f30_mul(b.x, a.zz);
    const Fq30 S1 = f30_mul(a.y, b.zzz);      // 4q * 2q
    const Fq30 S2 = f30_mul(b.y, a.zzz);
    const Fq30 P = f30_sub2(U2, U1);          // < 4q
    const Fq30 R = f30_sub2(S2, S1);          // < 4q
    const Fq30 PP = f30_sqr(P);
    const Fq30 PPP = f30_mul(P, PP);
    const Fq30 Q = f30_mul(U1, PP);
    const Fq30 ZZ3 = f30_mul(f30_mul(a.zz, b.zz), PP);
    Xyzz30 r;
    if (f30_is_zero_2q(ZZ3)) {  // same x: the same point or its opposite
        if (f30_all_zero(f30_canon8(R))) r = g1c_dbl(a);
        else xyzz30_set_inf(r);
        return r;
    }
    r.x = f30_sub6(f30_sqr(R), f30_add2x(PPP, Q));                          // < 8q
    r.y = f30_mul2add(R, f30_sub8(Q, r.x), f30_sub2(f30_zero(), S1), PPP);  // 4q*10q + 2q*2q -> < 2q
    r.zz = ZZ3;
    r.zzz = f30_mul(f30_mul(a.zzz, b.zzz), PPP);
    return r;
}

// v > (q - 1) / 2 for a canonical plain integer v
__device__ __forceinline__ bool g1c_is_larger(const Fq30& v) {
    u32 bw = 0;
#pragma unroll
    for (int i = 0; i < 13; i++) bw = (g1c::HALF(i) - v.l[i] - bw) >> 31;
    return bw != 0;
}

// One 48-byte compressed record (the zcash / arkworks encoding: big-endian x, top three bits of byte 0 = compressed, infinity, y is the
// larger root): flags, x < q, y = (x^3 + 4)^((q+1)/4), y^2 == x^3 + 4, the root the sign bit names.  Returns the status; for g1c::kOk
// `inf` says whether the record is the point at infinity, and otherwise (x, y) are the canonical coordinates in the internal form.  The
// loop has a constant trip count.  Membership in G1 is NOT part of it: g1c_in_subgroup.
__device__ __forceinline__ unsigned char g1c_decompress(const void* in48, size_t i, Fq30& x, Fq30& y, bool& inf) {
    // big-endian bytes -> little-endian words: word k of the integer is the byte-swapped word 11 - k of the record
    u32 w[12];
    const uint4* p = reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(in48) + i * 48);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const uint4 v = p[k];
        w[11 - 4 * k] = __builtin_bswap32(v.x);
        w[10 - 4 * k] = __builtin_bswap32(v.y);
        w[9 - 4 * k] = __builtin_bswap32(v.z);
        w[8 - 4 * k] = __builtin_bswap32(v.w);
    }
    const bool compressed = (w[11] >> 31) & 1u, sign = (w[11] >> 29) & 1u;
    inf = (w[11] >> 30) & 1u;
    w[11] &= 0x1fffffffu;
    u32 any = 0;
#pragma unroll
    for (int k = 0; k < 12; k++) any |= w[k];
    const Fq30 xc = f30_from_words(w);
    if (!compressed || (inf ? (sign || any != 0) : !g1c_lt_q(xc))) return g1c::kBadEncoding;
    if (inf) return g1c::kOk;
    x = f30_canon8(f30_mul(xc, g1c_r2()));                            // internal form, canonical
    const Fq30 rhs = f30_add(f30_mul(f30_sqr(x), x), g1c_four());     // x^3 + 4 < 3q
    y = rhs;                                                          // rhs^((q+1)/4): the top bit, then 378 squarings
#pragma unroll 1
    for (int b = g1c::kSqrtBits - 2; b >= 0; b--) {
        y = f30_sqr(y);
        if ((g1c::kSqrtExp[b >> 5] >> (b & 31)) & 1u) y = f30_mul(y, rhs);  // (the same branch in every lane)
    }
    if (!g1c_same(f30_canon8(f30_sqr(y)), f30_canon8(rhs))) return g1c::kNotOnCurve;
    Fq30 unit = f30_zero();
    unit.l[0] = 1;
    const Fq30 y_plain = f30_canon8(f30_mul(y, unit));  // out of Montgomery form: "larger" is a property of the integer
    y = f30_canon8(y);
    if (g1c_is_larger(y_plain) != sign) y = f30_neg_canon(y);
    return g1c::kOk;
}

// phi(P) == -[x^2]P for a point of the curve that is not infinity (Scott's membership test, see zk_g1check.hip): [x^2]P is two passes of
// 63 doublings and 5 additions (|x| = 0xd201000000010000), the comparison is by cross-multiplication: no inversion.
__device__ __forceinline__ bool g1c_in_subgroup(const Xyzz30& P) {
    Xyzz30 base = P, acc = P;
#pragma unroll 1
    for (int pass = 0; pass < 2; pass++) {  // acc = [|x|] base, twice: the top bit, then 63 doublings and 5 additions
        acc = base;
#pragma unroll 1
        for (int b = 62; b >= 0; b--) {
            acc = g1c_dbl(acc);
            if ((g1c::kXAbs >> b) & 1ULL) acc = g1c_add(acc, base);
        }
        base = acc;
    }
    // (beta Px / Pzz, Py / Pzzz) == (Ax / Azz, -Ay / Azzz), cross-multiplied; infinity is no such point
    bool ok = !xyzz30_is_inf(acc);
    if (ok) {
        const Fq30 l = f30_mul(f30_mul(g1c_beta(), P.x), acc.zz);  // q * 8q, then 2q * 2q
        const Fq30 r = f30_mul(acc.x, P.zz);                       // 8q * 2q
        const Fq30 s = f30_mul2add(P.y, acc.zzz, acc.y, P.zzz);    // 4q*2q + 4q*2q -> < 2q
        ok = g1c_same(f30_canon8(l), f30_canon8(r)) && f30_is_zero_2q(s);
    }
    return ok;
}

// One 18-word Jacobian record (X, Y, Z), reference Montgomery form, any representative, as XYZZ: canonical coordinates and
// Y^2 == X^3 + 4 Z^6 (no inversion).  Z = 0 is infinity whatever X and Y are.  Returns the status; p is set for g1c::kOk only.
__device__ __forceinline__ unsigned char g1c_load_jac(const void* in18, size_t i, Xyzz30& p) {
    const Fq30 xr = f30_load(in18, i * 144), yr = f30_load(in18, i * 144 + 48), zr = f30_load(in18, i * 144 + 96);
    if (!g1c_lt_q(xr) || !g1c_lt_q(yr) || !g1c_lt_q(zr)) return g1c::kBadEncoding;
    if (f30_all_zero(zr)) {
        xyzz30_set_inf(p);
        return g1c::kOk;
    }
    const Fq30 X = f30_from_ref(xr), Y = f30_from_ref(yr), Z = f30_from_ref(zr);  // canonical
    const Fq30 ZZ = f30_sqr(Z), ZZZ = f30_mul(ZZ, Z);                            // < 2q
    const Fq30 rhs = f30_mul2add(f30_sqr(X), X, f30_sqr(ZZZ), g1c_four());
    if (!g1c_same(f30_canon8(f30_sqr(Y)), f30_canon8(rhs))) return g1c::kNotOnCurve;
    p.x = X;  // (X, Y, Z^2, Z^3) is the XYZZ form of the same point
    p.y = Y;
    p.zz = ZZ;
    p.zzz = ZZZ;
    return g1c::kOk;
}

}  // namespace zk
