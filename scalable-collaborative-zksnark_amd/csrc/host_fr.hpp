// host_fr.hpp -- the few Fr operations on 4 x u64 that the host side of the aggregated verifier needs (zk_g1seg.hip, zk_pairing.hip):
// the modulus, the canonical test, a Montgomery product and a canonical sum.  Plain integers, no device code.
#pragma once
#include <cstdint>
#include <cstring>

namespace zkhost {
namespace fr {

typedef unsigned __int128 u128;
static const uint64_t R[4] = {0xffffffff00000001ULL, 0x53bda402fffe5bfeULL, 0x3339d80809a1d805ULL, 0x73eda753299d7d48ULL};
static const uint64_t RINV = 0xfffffffeffffffffULL;  // -r^-1 mod 2^64

// k < r
static inline bool canonical(const uint64_t* k) {
    for (int w = 3; w >= 0; w--)
        if (k[w] != R[w]) return k[w] < R[w];
    return false;
}
// t (with a fifth word `hi`) below 2r -> t mod r
static inline void csub_r(uint64_t* t, uint64_t hi) {
    if (!hi && canonical(t)) return;
    uint64_t bw = 0;
    for (int k = 0; k < 4; k++) {
        u128 d = (u128)t[k] - R[k] - bw;
        t[k] = (uint64_t)d;
        bw = (uint64_t)(d >> 64) & 1;
    }
}
// a b / 2^256 mod r, below r for a < r or b < r: with b = x 2^256 (Montgomery) and a canonical this is a x, canonical
static inline void mont_mul(const uint64_t* a, const uint64_t* b, uint64_t* out) {
    uint64_t t[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 4; i++) {
        u128 c = 0;
        for (int k = 0; k < 4; k++) {
            c += (u128)a[k] * b[i] + t[k];
            t[k] = (uint64_t)c;
            c >>= 64;
        }
        c += t[4];
        t[4] = (uint64_t)c;
        t[5] = (uint64_t)(c >> 64);
        const uint64_t m = t[0] * RINV;
        c = ((u128)m * R[0] + t[0]) >> 64;
        for (int k = 1; k < 4; k++) {
            c += (u128)m * R[k] + t[k];
            t[k - 1] = (uint64_t)c;
            c >>= 64;
        }
        c += t[4];
        t[3] = (uint64_t)c;
        t[4] = t[5] + (uint64_t)(c >> 64);
    }
    csub_r(t, t[4]);
    std::memcpy(out, t, 32);
}
// a + b mod r for a, b < r (r < 2^255: no carry out of four words)
static inline void add_canon(const uint64_t* a, const uint64_t* b, uint64_t* out) {
    uint64_t t[4];
    u128 c = 0;
    for (int k = 0; k < 4; k++) {
        c += (u128)a[k] + b[k];
        t[k] = (uint64_t)c;
        c >>= 64;
    }
    csub_r(t, 0);
    std::memcpy(out, t, 32);
}

}  // namespace fr
}  // namespace zkhost
