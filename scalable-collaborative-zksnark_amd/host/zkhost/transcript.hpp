// The Fiat-Shamir transcript of include/zkhip.h on the host (zkhip/transcript.py HostTranscript): a SHA-256 hash chain
//     init(label):   state = SHA256("zkhip-fs-v1" || label)
//     absorb(data):  state = SHA256(state || 0x00 || data)    field elements and points as they sit in proof records (little-endian u64
//                                                             limbs, Montgomery form), integers as one little-endian u64
//     challenge():   d = SHA256(state || 0x01), state = d;    d as a little-endian integer with its top two bits cleared (< 2^254 < r)
// This is the verifier's form: it needs no device.  The prover's transcript lives on the device (device.hpp: Ctx::transcript); the
// non-interactive provers and verifiers above both are in nizk.hpp.
#pragma once
#include <array>
#include <string>

#include "fr.hpp"
#include "sha256.hpp"

namespace zkhost {

class HostTranscript {
  public:
    explicit HostTranscript(const std::string &label) {
        Sha256 h;
        h.update("zkhip-fs-v1", 11);
        h.update(label.data(), label.size());
        h.digest(state_.data());
    }
    HostTranscript &absorb(const void *data, size_t n) {
        const uint8_t tag = 0x00;
        Sha256 h;
        h.update(state_.data(), 32), h.update(&tag, 1), h.update(data, n);
        h.digest(state_.data());
        return *this;
    }
    HostTranscript &absorb_u64(uint64_t v) {  // little-endian hosts only, like every buffer of the C ABI
        return absorb(&v, 8);
    }
    HostTranscript &absorb(const FrVec &v) { return absorb(v.data(), 32 * v.size()); }
    Fr challenge() {
        const uint8_t tag = 0x01;
        Sha256 h;
        h.update(state_.data(), 32), h.update(&tag, 1);
        h.digest(state_.data());
        Fr c;
        std::memcpy(c.v, state_.data(), 32);
        c.v[3] &= 0x3fffffffffffffffull;
        return Fr::from_canonical(c);
    }
    FrVec challenges(size_t count) {
        FrVec out;
        for (size_t i = 0; i < count; ++i) out.push_back(challenge());
        return out;
    }
    const std::array<uint8_t, 32> &state() const { return state_; }
    std::string state_hex() const {
        static const char *d = "0123456789abcdef";
        std::string s;
        for (uint8_t b : state_) s.push_back(d[b >> 4]), s.push_back(d[b & 15]);
        return s;
    }

  private:
    std::array<uint8_t, 32> state_;
};

}  // namespace zkhost
