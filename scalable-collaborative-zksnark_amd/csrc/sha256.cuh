// sha256.cuh -- SHA-256 (FIPS 180-4) and the Fiat-Shamir transcript of include/zkhip.h on ONE lane, in plain C++.
//
// The transcript is a hash chain on a 32-byte state:
//   init(label):  state = SHA256("zkhip-fs-v1" || label)
//   absorb(data): state = SHA256(state || 0x00 || data)
//   challenge():  d = SHA256(state || 0x01), state = d; the challenge is d read as a little-endian 256-bit integer with its top two
//                 bits cleared (< 2^254 < r: no rejection loop), taken to Montgomery form by one multiplication with R^2.
// In registers the state is the eight big-endian words of the digest; in memory it is the digest's 32 bytes (fs_state_load / _store).
//
// Two front ends over one compression function: Sha256Bytes feeds single bytes (labels, byte strings of any length: the
// transcript kernels of zk_transcript.hip), fs_absorb_words<NW> hashes state || 0x00 || NW little-endian 32-bit words with
// every index known at compile time, so the message schedule stays in registers (the per-round hash of the sumcheck kernels,
// zk_fs.hip: four compressions for the 193 bytes state || 0x00 || five evaluations of a gate round, one more for the challenge).
#pragma once
#include "fp.cuh"

namespace zk {

__device__ __forceinline__ u32 sha_rotr(u32 x, int n) { return (x >> n) | (x << (32 - n)); }
__device__ __forceinline__ u32 sha_bswap(u32 x) { return (x >> 24) | ((x >> 8) & 0xff00u) | ((x << 8) & 0xff0000u) | (x << 24); }

__device__ __forceinline__ constexpr u32 sha_k(int i) {
    constexpr u32 k[64] = {
        0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, 0x243185beu,
        0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau,
        0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u, 0x27b70a85u,
        0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u,
        0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu,
        0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
    return k[i];
}

__device__ __forceinline__ void sha256_init(u32 (&h)[8]) {
    h[0] = 0x6a09e667u, h[1] = 0xbb67ae85u, h[2] = 0x3c6ef372u, h[3] = 0xa54ff53au;
    h[4] = 0x510e527fu, h[5] = 0x9b05688cu, h[6] = 0x1f83d9abu, h[7] = 0x5be0cd19u;
}

// one block: m = sixteen big-endian message words.  The schedule is a rolling window of sixteen words, every index a constant.
__device__ __forceinline__ void sha256_compress(u32 (&h)[8], const u32 (&m)[16]) {
    u32 w[16];
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = m[i];
    u32 a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
#pragma unroll
    for (int i = 0; i < 64; i++) {
        if (i >= 16) {
            const u32 w15 = w[(i + 1) & 15], w2 = w[(i + 14) & 15];
            const u32 s0 = sha_rotr(w15, 7) ^ sha_rotr(w15, 18) ^ (w15 >> 3);
            const u32 s1 = sha_rotr(w2, 17) ^ sha_rotr(w2, 19) ^ (w2 >> 10);
            w[i & 15] = w[i & 15] + s0 + w[(i + 9) & 15] + s1;
        }
        const u32 t1 = hh + (sha_rotr(e, 6) ^ sha_rotr(e, 11) ^ sha_rotr(e, 25)) + ((e & f) ^ (~e & g)) + sha_k(i) + w[i & 15];
        const u32 t2 = (sha_rotr(a, 2) ^ sha_rotr(a, 13) ^ sha_rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
        hh = g, g = f, f = e, e = d + t1, d = c, c = b, b = a, a = t1 + t2;
    }
    h[0] += a, h[1] += b, h[2] += c, h[3] += d, h[4] += e, h[5] += f, h[6] += g, h[7] += hh;
}

// byte-wise front end (indices depend on the data length: the block lives in private memory, which is fine for a label or a commitment)
struct Sha256Bytes {
    u32 h[8];
    u32 m[16];
    u32 fill;   // bytes in m
    u64 total;  // bytes so far
    __device__ void init() {
        sha256_init(h);
        for (int i = 0; i < 16; i++) m[i] = 0;
        fill = 0, total = 0;
    }
    __device__ void put(u32 byte) {
        m[fill >> 2] |= (byte & 0xffu) << (24 - 8 * (fill & 3));
        total++;
        if (++fill == 64) {
            sha256_compress(h, m);
            for (int i = 0; i < 16; i++) m[i] = 0;
            fill = 0;
        }
    }
    __device__ void finish() {  // h = the digest's words
        const u64 bits = total * 8;
        put(0x80);
        while (fill != 56) put(0);
        m[14] = (u32)(bits >> 32), m[15] = (u32)bits;
        sha256_compress(h, m);
    }
};

// the state in memory is the digest's 32 bytes
__device__ __forceinline__ void fs_state_load(u32 (&st)[8], const u32* mem) {
#pragma unroll
    for (int i = 0; i < 8; i++) st[i] = sha_bswap(mem[i]);
}
__device__ __forceinline__ void fs_state_store(u32* mem, const u32 (&st)[8]) {
#pragma unroll
    for (int i = 0; i < 8; i++) mem[i] = sha_bswap(st[i]);
}

// absorb of NW little-endian 32-bit words (the limbs of field elements as they sit in memory): the message is
// state (8 words) || 0x00 || data, so data word i straddles message words 8 + i and 9 + i.
template <int NW>
__device__ __forceinline__ void fs_absorb_words(u32 (&st)[8], const u32 (&data)[NW]) {
    constexpr int kBytes = 33 + 4 * NW;
    constexpr int kBlocks = (kBytes + 9 + 63) / 64;
    u32 msg[16 * kBlocks];
#pragma unroll
    for (int i = 0; i < 16 * kBlocks; i++) msg[i] = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) msg[i] = st[i];
    u32 tail = 0;  // the domain byte 0x00
#pragma unroll
    for (int i = 0; i < NW; i++) {
        const u32 d = sha_bswap(data[i]);
        msg[8 + i] = (tail << 24) | (d >> 8);
        tail = d & 0xffu;
    }
    msg[8 + NW] = (tail << 24) | 0x00800000u;
    msg[16 * kBlocks - 1] = (u32)kBytes * 8;
    sha256_init(st);
#pragma unroll
    for (int b = 0; b < kBlocks; b++) {
        u32 blk[16];
#pragma unroll
        for (int i = 0; i < 16; i++) blk[i] = msg[16 * b + i];
        sha256_compress(st, blk);
    }
}

// challenge(): one compression; -> the challenge in Montgomery form
__device__ __forceinline__ Fr fs_challenge(u32 (&st)[8]) {
    u32 blk[16];
#pragma unroll
    for (int i = 0; i < 8; i++) blk[i] = st[i];
    blk[8] = 0x01800000u;
#pragma unroll
    for (int i = 9; i < 15; i++) blk[i] = 0;
    blk[15] = 33 * 8;
    sha256_init(st);
    sha256_compress(st, blk);
    Fr c, r2;
#pragma unroll
    for (int i = 0; i < 8; i++) c.l[i] = sha_bswap(st[i]), r2.l[i] = FrCfg::R2(i);
    c.l[7] &= 0x3fffffffu;
    return fp_mul<FrCfg>(c, r2);
}

// a round of a transcript-driven sumcheck: absorb its NE evaluations, draw the challenge
template <int NE>
__device__ __forceinline__ Fr fs_round(u32 (&st)[8], const Fr (&ev)[NE]) {
    u32 data[8 * NE];
#pragma unroll
    for (int t = 0; t < NE; t++)
#pragma unroll
        for (int i = 0; i < 8; i++) data[8 * t + i] = ev[t].l[i];
    fs_absorb_words<8 * NE>(st, data);
    return fs_challenge(st);
}

}  // namespace zk
