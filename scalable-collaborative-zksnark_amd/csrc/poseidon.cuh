// poseidon.cuh -- what the kernels that hash inside a lane share (zk_poseidon.hip: the permutation, hash and Merkle kernels; zk_jubjub.hip:
// the Schnorr challenge): the parameter object and the permutation in registers.  The rule and the layout of the constants block are
// stated in zk_poseidon.hip; the text below is the text that file held, moved here unchanged, so its kernels compile as before.
#pragma once
#include "fp.cuh"

struct zk_ctx;
struct zk_poseidon_params {
    zk_ctx* ctx = nullptr;
    void* d_consts = nullptr;  // 9 Fr of M, then 3 (rf + rp) Fr of round constants
    uint32_t half = 0, rp = 0;  // rf / 2 full rounds on either side of rp partial ones
};

namespace zk {

__device__ __forceinline__ Fr pos_pow5(const Fr& x) {
    const Fr x2 = fr_mul(x, x);
    return fr_mul(fr_mul(x2, x2), x);
}

// the permutation on (s0, s1, s2); consts: the params block.  Every address below is the same in all lanes.
__device__ __forceinline__ void pos_permute(const void* __restrict__ consts, u32 half, u32 rp, Fr& s0, Fr& s1, Fr& s2) {
    const u32 rounds = 2 * half + rp;
#pragma unroll 1
    for (u32 k = 0; k < rounds; k++) {
        s0 = fr_add(s0, fr_load(consts, 9 + 3 * (size_t)k));
        s1 = fr_add(s1, fr_load(consts, 10 + 3 * (size_t)k));
        s2 = fr_add(s2, fr_load(consts, 11 + 3 * (size_t)k));
        s0 = pos_pow5(s0);
        if (k < half || k >= half + rp) {  // wave-uniform: a full round
            s1 = pos_pow5(s1);
            s2 = pos_pow5(s2);
        }
        const Fr t0 = fr_add(fr_add(fr_mul(fr_load(consts, 0), s0), fr_mul(fr_load(consts, 1), s1)), fr_mul(fr_load(consts, 2), s2));
        const Fr t1 = fr_add(fr_add(fr_mul(fr_load(consts, 3), s0), fr_mul(fr_load(consts, 4), s1)), fr_mul(fr_load(consts, 5), s2));
        const Fr t2 = fr_add(fr_add(fr_mul(fr_load(consts, 6), s0), fr_mul(fr_load(consts, 7), s1)), fr_mul(fr_load(consts, 8), s2));
        s0 = t0, s1 = t1, s2 = t2;
    }
}
__device__ __forceinline__ Fr pos_hash2(const void* __restrict__ consts, u32 half, u32 rp, const Fr& l, const Fr& r) {
    Fr s0 = fp_zero<FrCfg>(), s1 = l, s2 = r;
    pos_permute(consts, half, rp, s0, s1, s2);
    return s0;
}

}  // namespace zk
