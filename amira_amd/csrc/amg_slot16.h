// amg_slot16.h — the 16-byte slot of the exact-key tables, how a local key is read back out of it, a claim's first-seen
// and its rank: what the table passes (amg_x.h, amg_build_x.hip) share with the per-claim stage (amg_build_x_claims.hip,
// amg_build_x_comp.hip) and the multi-GPU merge (amg_dist_local.hip, amg_dist_merge.hip).
#pragma once
#include "amg_device.h"

struct __attribute__((aligned(16))) Slot16 {
  unsigned long long w1;
  unsigned long long w2;
};
static_assert(sizeof(Slot16) == 16, "slot16");

// token j of a packed canonical tuple: w1 = (low 63 bits << 1) | 1, tag = (high 31 bits << 1) | 1
__device__ __forceinline__ int x_unpack(unsigned long long w1, unsigned int tag, int bits, int j) {
  const unsigned long long lo = w1 >> 1, hi = (unsigned long long)(tag >> 1);
  const int sh = j * bits;
  unsigned long long v = sh < 63 ? ((lo >> sh) | (hi << (63 - sh))) : (hi >> (sh - 63));
  return (int)(v & ((1ull << bits) - 1ull));
}


// First-seen of a claim lives in TWO adjacent words, both holding the complement (so that larger =
// earlier) and both zero-initialised: [2c] is raised with atomicMax by every window that is not
// the creator, [2c + 1] is the creator's own plain store; the larger one wins.  Adjacent, so
// that the per-window check is one 8-byte load.
__device__ __forceinline__ unsigned int x_first_inv(const unsigned int* first2, long long c) {
  const uint2 f = reinterpret_cast<const uint2*>(first2)[c];
  return f.x > f.y ? f.x : f.y;
}

// Rank of token position t among the positions flagged for a bitmap ranking (RankBitmap, amg_internal.h): the bits set
// before t's own.  A token position opens at most one window / adjacency, so the first-seen positions of the claims are
// distinct and the rank of a claim's first-seen position is the claim's place in first-seen order.
__device__ __forceinline__ long long x_rank_of(unsigned int t, const unsigned int* __restrict__ bits,
                                               const long long* __restrict__ prefix) {
  const unsigned int w = bits[t >> 5];
  return prefix[t >> 5] + (long long)__popc(w & ((1u << (t & 31)) - 1u));
}
