// zk_find.cuh -- the open-addressing slot protocol shared by zk_lookup_find.hip (K20 / K21: whole entries as keys, NC = 1 or 3 columns)
// and zk_witness.hip (the key table of a lookup plan: the pair (t0, t1) as the key, NC = 2).  zk_lookup_find.hip states the protocol and
// why its result -- the smallest index of an equal entry -- depends on the table alone; here are its three parts:
//   find_hash    the start slot of a key
//   find_insert  the walk of K20: claim the first empty slot by CAS, or meet an equal key there and lower the slot's index
//   find_walk    the walk of K21: plain loads to the slot whose entry equals the key (hit), or to EMPTY (miss)
// Every walk is bounded by the slot count; an index read from a slot is checked to be < N before anything is read through it.
#pragma once
#include "zk_gate.cuh"

namespace zk {

static constexpr u32 kFindEmpty = 0xffffffffu;

template <int NC>
struct FindCols {
    const void* w[NC];  // the rows: f, or a, b, c
    const void* t[NC];  // the table: t, or t0, t1, t2 (the key table of a witness plan: t0, t1)
};

// 64-bit mix of all limbs of a key (a multiply-xorshift chain closed by the finaliser of MurmurHash3)
template <int NC>
__device__ __forceinline__ u64 find_hash(const Fr (&k)[NC]) {
    u64 h = 0x243f6a8885a308d3ull;
#pragma unroll
    for (int j = 0; j < NC; j++)
#pragma unroll
        for (int i = 0; i < 4; i++) {
            h ^= ((u64)k[j].l[2 * i + 1] << 32) | k[j].l[2 * i];
            h *= 0x9e3779b97f4a7c15ull;
            h ^= h >> 29;
        }
    h ^= h >> 33;
    h *= 0xff51afd7ed558ccdull;
    h ^= h >> 33;
    h *= 0xc4ceb9fe1a85ec53ull;
    h ^= h >> 33;
    return h;
}
template <int NC>
__device__ __forceinline__ bool find_equal(const Fr (&k)[NC], const FindCols<NC>& c, size_t v) {  // the key against table entry v
    bool eq = true;
#pragma unroll
    for (int j = 0; j < NC; j++) eq = eq && fp_eq(k[j], fr_load(c.t[j], v));
    return eq;
}

// K20's walk for entry y with key k.  mask = slots - 1; force >= 0: every key starts at slot force & mask (knob find_force_slot).
// false: the walk passed every slot or met a word that is no index (cannot happen: the caller sets its internal flag)
template <int NC>
__device__ __forceinline__ bool find_insert(const Fr (&k)[NC], const FindCols<NC>& c, size_t N, size_t y, u32* __restrict__ slots, u64 mask, long long force) {
    u64 s = (force >= 0 ? (u64)force : find_hash<NC>(k)) & mask;
    for (u64 step = 0; step <= mask; step++, s = (s + 1) & mask) {
        const u32 prev = atomicCAS(&slots[s], kFindEmpty, (u32)y);
        if (prev == kFindEmpty) return true;  // claimed
        if (prev >= N) return false;          // not an index: cannot happen
        if (find_equal<NC>(k, c, prev)) {
            if ((u32)y < prev) atomicMin(&slots[s], (u32)y);  // the slot's index only falls: one that is already smaller stays smaller
            return true;
        }
    }
    return false;
}

// K21's walk for the key k, in a launch after the one that built the slots.  1: hit, v = the slot's index (the smallest index of an
// equal entry); 2: miss; 0: the walk passed every slot or met a word that is no index (cannot happen)
template <int NC>
__device__ __forceinline__ int find_walk(const Fr (&k)[NC], const FindCols<NC>& c, size_t N, const u32* __restrict__ slots, u64 mask, long long force, u32& v) {
    u64 s = (force >= 0 ? (u64)force : find_hash<NC>(k)) & mask;
    v = kFindEmpty;
    for (u64 step = 0; step <= mask; step++, s = (s + 1) & mask) {
        v = slots[s];
        if (v == kFindEmpty) return 2;
        if (v >= N) return 0;  // not an index: cannot happen
        if (find_equal<NC>(k, c, v)) return 1;
    }
    return 0;
}

}  // namespace zk
