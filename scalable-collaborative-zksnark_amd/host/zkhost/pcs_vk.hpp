// The verifying key of a structured PolynomialCommitment built on the compiled host: powers_of_g2 = [g2, s_0 g2, ..., s_{n-1} g2]
// (dist-primitive/src/dpoly_comm.rs:59-62) by zk_msm_g2 on the BLS12-381 G2 generator, handed to the library as a zk_pcs_vk
// (g1 = the G1 generator).  Used by examples/pcs_verify.cpp and examples/gate_check.cpp.
#pragma once
#include <cstring>
#include <memory>
#include <vector>

#include "serialize.hpp"

namespace zkhost {

// the BLS12-381 G2 generator, canonical little-endian limbs (x.c0, x.c1, y.c0, y.c1)
static const uint64_t kG2Gen[4][6] = {
    {0xd48056c8c121bdb8ull, 0x0bac0326a805bbefull, 0xb4510b647ae3d177ull, 0xc6e47ad4fa403b02ull, 0x260805272dc51051ull, 0x024aa2b2f08f0a91ull},
    {0xe5ac7d055d042b7eull, 0x334cf11213945d57ull, 0xb5da61bbdc7f5049ull, 0x596bd0d09920b61aull, 0x7dacd3a088274f65ull, 0x13e02b6052719f60ull},
    {0xe193548608b82801ull, 0x923ac9cc3baca289ull, 0x6d429a695160d12cull, 0xadfd9baa8cbdd3a7ull, 0x8cc9cdc6da2e351aull, 0x0ce5d527727d6e11ull},
    {0xaaa9075ff05f79beull, 0x3f370d275cec1da1ull, 0x267492ab572e99abull, 0xcb3e287e85a763afull, 0x32acd2b02bc28b99ull, 0x0606c4a02ea734ccull}};

// n + 1 affine G2 records of 24 Montgomery words (192 bytes) each
inline std::vector<uint64_t> powers_of_g2(Ctx &be, const FrVec &s) {
    std::vector<uint64_t> g2rec(24);
    for (int c = 0; c < 4; ++c) {
        Fq x = Fq::zero();
        std::memcpy(x.v, kG2Gen[c], 48);
        x = Fq::from_canonical(x);
        std::memcpy(&g2rec[6 * c], x.v, 48);
    }
    SrsPtr g2srs = be.srs_register_g2(g2rec.data(), 192, 1);
    std::vector<uint64_t> pg2(g2rec);
    for (size_t i = 0; i < s.size(); ++i) {
        G2 p = be.msm_g2(*g2srs, be.to_device(FrVec{s[i]}), 1);  // normalised: (x, y, 1)
        pg2.insert(pg2.end(), p.begin(), p.begin() + 24);
    }
    return pg2;
}

inline std::shared_ptr<PcsVk> make_pcs_vk(Ctx &be, const FrVec &s) {
    const std::vector<uint64_t> pg2 = powers_of_g2(be, s);
    return be.pcs_vk(nullptr, pg2.data(), 192, s.size() + 1);
}

}  // namespace zkhost
