// sem_key.hpp — the 64-bit semantic signature of a row of float32 predictions, shared by sr_semantic.hip (whole trees, register
// interpreter) and sr_subtree_sig.hip (every subtree, tape walk):
//     sig = sem_finish( sum_{d<D} sem_term(p[d], d), D )        all arithmetic mod 2^64
// The sum is position-keyed, so no order of lanes, tiles or waves changes it.
#pragma once
#include "evogp_defs.hpp"

namespace evogp {

// the key of a prediction: -0.0 is +0.0, every NaN is the canonical quiet NaN
__device__ inline uint32_t sem_key(float p) {
    const uint32_t u = f2bits(p), mag = u & 0x7FFFFFFFu;
    return mag == 0u ? 0u : (mag > 0x7F800000u ? 0x7FC00000u : u);
}
// the term of row d in a tree's sum
__device__ inline unsigned long long sem_term(float p, unsigned long long d) {
    return mix64((unsigned long long)sem_key(p) ^ ((d + 1ull) * kDedupGold));
}
__device__ inline unsigned long long sem_finish(unsigned long long sum, int D) { return mix64(sum + (unsigned long long)D); }

}  // namespace evogp
