// amg_x.h — the exact-key table passes over the 16-byte slot of amg_slot16.h: what the node and edge kernels of
// amg_build_x.hip do between packing a key and writing a window's result.
//
//   keys        x_pack / x_canon_pack / f_canon_pack16: canonical tuple -> (w1, tag)
//   claim ids   XShard, tile_shard: which counter a workgroup's creations take their ids from
//   shared      TilePos, creator_ranks, workgroup_claim_base(s), checked_claim, publish_claim, await_published,
//   steps       raise_first_seen, hashed_slot: one definition each, used by both protocols
//   protocols   one-word keys (x_upsert_one, f_table_phase_one): the compare-and-swap that sets w1 creates the key;
//               two-word keys (x_upsert_own, f_table_phase_own): the compare-and-swap that sets w1 OWNS the slot, the
//               tag in w2 says whose key it is once the owner has published
#pragma once
#include "amg_device.h"
#include "amg_slot16.h"
#include "amg_tile.h"

// ------------------------------------------------------------------ keys
// canonical tuple -> (w1, tag): token j occupies bits [j*bits, (j+1)*bits) of a 94-bit value,
// w1 = (low 63 bits << 1) | 1, tag = (high 31 bits << 1) | 1 — both non-zero by construction
template <class View>
__device__ __forceinline__ void x_pack(const View& w, int k, int flip, int dir, int bits,
                                       unsigned long long& w1, unsigned int& tag) {
  unsigned long long lo = 0, hi = 0;
  int sh = 0;
  for (int j = 0; j < k; ++j, sh += bits) {
    const unsigned long long c = (unsigned long long)(unsigned int)canon_tok(w, k, flip, dir, j);
    if (sh < 63) {
      lo |= c << sh;
      if (sh + bits > 63) hi |= c >> (63 - sh);
    } else {
      hi |= c << (sh - 63);
    }
  }
  w1 = (lo << 1) | 1ull;  // bit 63 of lo (it belongs to hi) falls off here
  tag = ((unsigned int)hi << 1) | 1u;
}

// Compile-time k: direction, canonical tuple and packing as straight-line code (no early-exit
// loop, no per-token branches).  Returns the direction (0: palindrome).
template <int K, bool TWO>
__device__ __forceinline__ int x_canon_pack(const int* w, int flip, int bits, unsigned long long& w1,
                                            unsigned int& tag) {
  int a[K];
#pragma unroll
  for (int j = 0; j < K; ++j) a[j] = w[j];
  int dir = 0;  // the first differing position decides: walk from the last to the first
#pragma unroll
  for (int j = K - 1; j >= 0; --j) {
    const int d = a[j] - (flip - a[K - 1 - j]);
    dir = d != 0 ? (d < 0 ? 1 : -1) : dir;
  }
  if (TWO) {
    unsigned __int128 v = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const unsigned int c = (unsigned int)(dir > 0 ? a[j] : flip - a[K - 1 - j]);
      v |= (unsigned __int128)c << (j * bits);
    }
    w1 = ((unsigned long long)v << 1) | 1ull;
    tag = ((unsigned int)(unsigned long long)(v >> 63) << 1) | 1u;
  } else {
    unsigned long long v = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      const unsigned int c = (unsigned int)(dir > 0 ? a[j] : flip - a[K - 1 - j]);
      v |= (unsigned long long)c << (j * bits);
    }
    w1 = (v << 1) | 1ull;
    tag = 1u;
  }
  return dir;
}

// Canonical orientation + packed key of the window a[0..K-1] for 16-bit tokens (two_v <= 65536),
// K odd.  Forward half-words a[j] | a[j+1] << 16, reverse-complement half-words
// (F | F << 16) - (a[j+1] | a[j] << 16).  Encoding == x_pack with bits = 16.
template <int K, bool TWO>
__device__ __forceinline__ int f_canon_pack16(const int* a, int flip, unsigned long long& w1, unsigned int& tag) {
  int dir = (2 * a[K / 2] < flip) ? 1 : -1;  // 2 x != 2V - 1: an odd k has no palindromes
#pragma unroll
  for (int j = K / 2 - 1; j >= 0; --j) {
    const int s = a[j] + a[K - 1 - j];
    dir = s != flip ? (s < flip ? 1 : -1) : dir;
  }
  const unsigned int ff = (unsigned int)flip | ((unsigned int)flip << 16);
  unsigned int word[K / 2 + 1];
#pragma unroll
  for (int m = 0; m < K / 2; ++m) {
    const unsigned int fw = (unsigned int)a[2 * m] | ((unsigned int)a[2 * m + 1] << 16);
    const unsigned int rc = ff - ((unsigned int)a[K - 1 - 2 * m] | ((unsigned int)a[K - 2 - 2 * m] << 16));
    word[m] = dir > 0 ? fw : rc;
  }
  word[K / 2] = (unsigned int)(dir > 0 ? a[K - 1] : flip - a[0]);
  const unsigned long long v = (unsigned long long)word[0] | ((unsigned long long)word[1] << 32);
  w1 = (v << 1) | 1ull;
  if constexpr (K == 3)
    tag = 1u;
  else  // K == 5
    tag = (((word[1] >> 31) | (word[K / 2] << 1)) << 1) | 1u;
  return dir;
}

// ------------------------------------------------------------------ the second word of a slot
// One-word keys: [63:32] the creator's exact first-seen (complemented), [31:0] claim id + 1.  Two-word keys (the key
// spills into it): [63:32] tag, [31:ib] COARSE token position of the creating window (token index >> cshift),
// [ib-1:0] claim id + 1.  Either way the word is zero until its ONE store publishes it, complete and final, and the
// probe load already tells almost every window that it comes after the creator and cannot be the first occurrence:
// the first-seen words of the claim are then not even read (one random access per window less; the table passes are
// bound by the L2 request rate).
struct XW2 {
  int ib;      // bits of the id field (two-word keys)
  int cshift;  // coarse position = token index >> cshift (two-word keys)
};
// the low half of a two-word key's second word: claim id + 1, and the coarse position beside it
__device__ __forceinline__ unsigned int xw2_id1(unsigned int low, const XW2& f) { return low & ((1u << f.ib) - 1u); }
__device__ __forceinline__ unsigned long long publish_word_two(unsigned int tag, unsigned int tpos, unsigned int claim,
                                                               const XW2& f) {
  return ((unsigned long long)tag << 32) | (unsigned long long)((tpos >> f.cshift) << f.ib) |
         (unsigned long long)(claim + 1u);
}

// ------------------------------------------------------------------ claim ids
// The thread that creates a key gives it a claim id.  A WORKGROUP reserves the ids of its creations with one atomicAdd
// (workgroup_claim_base).  Small inputs have one counter, in the status words, and claim = the value it returned: ids
// are dense.  Large inputs have F_SHARDS + 1 counters, 128 bytes apart (55 k returning atomics on one word are what a
// first-build pass waited for once its creations were cheap: 0.42 of 0.72 ms in the edge pass; one word takes ≈ 100
// per microsecond):
//   * a workgroup adds to the counter of its shard (tile index & 63), and shard s owns every 64th CHUNK of X_CHUNK
//     claim ids (a tile's worth: a workgroup's stores into the per-claim arrays share lines);
//   * the FIRST tiles of the stream — the head launch, which creates the genome's keys, and a few times as many tiles
//     after it, which create the ones it missed — share a counter of their own (shard F_SHARDS) and take the ids
//     [0, base) densely: those keys hold the lowest claims, which the counting sweeps rely on (spread over the shards
//     they lay scattered over 64 k ids and the two counts of a rebuild took 0.2 ms each instead of 0.07).
// The shards' ids start at `base`; ids in use lie below base + X_CHUNK * F_SHARDS * ceil(largest shard count / X_CHUNK);
// ids nobody took keep first-seen == 0 and are skipped wherever claims are listed.
#define F_SHARDS 64
#define F_CTR_STRIDE 16  // counters 128 bytes apart (u64 words)
#define X_CHUNK 1024u
__device__ __forceinline__ unsigned int x_chunk_claim(unsigned int li, unsigned int shard) {
  return (li / X_CHUNK) * (X_CHUNK * F_SHARDS) + shard * X_CHUNK + (li % X_CHUNK);
}
// which counter a workgroup adds to and what its local index li becomes: no shards (shard < 0: one counter, claim = li),
// the first tiles' counter, a shard's.  `ctr` is the one counter or the array of them, `cap` a counter's share of ids.
struct XShard {
  int shard;          // -1, 0 .. F_SHARDS - 1, F_SHARDS (first tiles)
  unsigned int base;  // ids of the first tiles = capacity of their counter
  __device__ __forceinline__ unsigned long long* counter(unsigned long long* ctr) const {
    return shard >= 0 ? ctr + (unsigned int)shard * F_CTR_STRIDE : ctr;
  }
  __device__ __forceinline__ unsigned int limit(unsigned int cap) const { return shard == (int)F_SHARDS ? base : cap; }
  __device__ __forceinline__ unsigned int claim(unsigned int li) const {
    return shard < 0 || shard == (int)F_SHARDS ? li : base + x_chunk_claim(li, (unsigned int)shard);
  }
};
// the shard of tile `tile` (ctrs == nullptr: no shards): the tiles of a HEAD launch and those whose tokens lie below
// head_cap take the first tiles' counter
template <bool HEAD>
__device__ __forceinline__ XShard tile_shard(const unsigned long long* ctrs, unsigned int tile, unsigned int head_cap) {
  return XShard{ctrs ? ((HEAD || tile * (unsigned int)TILE < head_cap) ? (int)F_SHARDS : (int)(tile & (F_SHARDS - 1u))) : -1,
                head_cap};
}
// local index -> claim id.  A counter's share of the claim arrays used up: the host rebuilds larger.
__device__ __forceinline__ unsigned int checked_claim(const XShard& xs, unsigned int li, unsigned int cap,
                                                      unsigned long long* status, int which) {
  if (li >= xs.limit(cap)) {
    status[ST_OVERFLOW] = (unsigned long long)which;
    li = 0;
  }
  return xs.claim(li);
}

// what a window's result array says about its key: claim id, flags; -1: no key (id1 = claim id + 1, 0: none)
__device__ __forceinline__ int claim_word(unsigned int id1, bool last, bool made) {
  return id1 ? (int)((id1 - 1u) | (last ? AMG_LAST_FLAG : 0u) | (made ? AMG_MADE_FLAG : 0u)) : -1;
}

// ------------------------------------------------------------------ steps both protocols take
template <class T>
__device__ __forceinline__ T f_pick(const T (&a)[TILE_ITEMS], int w) {
  return w == 0 ? a[0] : w == 1 ? a[1] : w == 2 ? a[2] : a[3];
}

// Window `it` of a thread starts STRIDE tokens after window it - 1, the first at token tbase; its first-seen value is
// (token << FSH) | low bits (lowbits: FSH bits per item, packed), kept complemented.  (Positions and first-seen values
// are recomputed instead of kept in arrays: the table kernels run 8 waves per SIMD on 64 registers.)
template <int FSH, int STRIDE>
struct TilePos {
  unsigned int tbase, lowbits;
  __device__ __forceinline__ unsigned int tpos(int it) const { return tbase + (unsigned int)it * (unsigned int)STRIDE; }
  __device__ __forceinline__ unsigned int fi(int it) const {
    return ~((tpos(it) << FSH) | ((lowbits >> (it * FSH)) & ((1u << FSH) - 1u)));
  }
};

// where a key lives among the hashed slots tab[off .. off + mask], before `off` is added (tag: the second part of a two-word key; a one-word key that gives up its home slot passes 0)
__device__ __forceinline__ unsigned int hashed_slot(unsigned long long w1, unsigned int tag, unsigned int mask) {
  return (unsigned int)mix64(w1 ^ ((unsigned long long)tag * 0x9E3779B97F4A7C15ull)) & mask;
}

// pre[it] = rank of item `it` among the wave's creators (the items of the mask `created`, item by item, lane by lane);
// returns the wave's number of creators.  Ballots: no LDS, no barrier.
__device__ __forceinline__ unsigned int creator_ranks(unsigned int created, unsigned int (&pre)[TILE_ITEMS]) {
  const unsigned long long below = (1ull << (threadIdx.x & 63u)) - 1ull;
  unsigned int n = 0;
#pragma unroll
  for (int it = 0; it < TILE_ITEMS; ++it) {
    const unsigned long long m = __ballot((created >> it) & 1u);
    pre[it] = n + (unsigned int)__popcll(m & below);
    n += (unsigned int)__popcll(m);
  }
  return n;
}

// One atomicAdd per workgroup reserves the local indices of its creators: returns the first index of this WAVE's n.
// s_wave: TILE_THREADS / 64 wave totals + the workgroup's base.  Every thread of the workgroup calls it (barriers).
__device__ __forceinline__ unsigned int workgroup_claim_base(unsigned int n, unsigned long long* counter,
                                                             unsigned int* s_wave) {
  const unsigned int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0) s_wave[wave] = n;
  __syncthreads();
  unsigned int before = 0, total = 0, base = 0;
#pragma unroll
  for (unsigned int w = 0; w < TILE_THREADS / 64; ++w) {
    const unsigned int cnt = s_wave[w];
    before += w < wave ? cnt : 0u;
    total += cnt;
  }
  if (total) {  // workgroup-uniform
    if (threadIdx.x == 0) s_wave[TILE_THREADS / 64] = (unsigned int)atomicAdd(counter, (unsigned long long)total);
    __syncthreads();
    base = s_wave[TILE_THREADS / 64] + before;
  }
  return base;
}

// The same for a workgroup with two kinds of creators, n_t of the first and n_l of the second in this wave: the second
// kind takes the indices after the first kind's from the same counter, or (counter_l != nullptr) indices of its own from
// another.  s_wave: TILE_THREADS / 64 packed wave totals + the two bases.
__device__ __forceinline__ void workgroup_claim_bases(unsigned int n_t, unsigned int n_l, unsigned long long* counter_t,
                                                      unsigned long long* counter_l, unsigned int* s_wave,
                                                      unsigned int& base_t, unsigned int& base_l) {
  const unsigned int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0) s_wave[wave] = n_t | (n_l << 16);
  __syncthreads();
  unsigned int before_t = 0, before_l = 0, total_t = 0, total_l = 0;
#pragma unroll
  for (unsigned int w = 0; w < TILE_THREADS / 64; ++w) {
    const unsigned int cnt = s_wave[w];
    before_t += w < wave ? (cnt & 0xffffu) : 0u;
    before_l += w < wave ? (cnt >> 16) : 0u;
    total_t += cnt & 0xffffu;
    total_l += cnt >> 16;
  }
  base_t = base_l = 0;
  if (total_t + total_l) {  // workgroup-uniform
    if (threadIdx.x == 0) {
      unsigned int bt, bl;
      if (counter_l) {
        bt = total_t ? (unsigned int)atomicAdd(counter_t, (unsigned long long)total_t) : 0u;
        bl = total_l ? (unsigned int)atomicAdd(counter_l, (unsigned long long)total_l) : 0u;
      } else {
        bt = (unsigned int)atomicAdd(counter_t, (unsigned long long)(total_t + total_l));
        bl = bt + total_t;
      }
      s_wave[TILE_THREADS / 64] = bt;
      s_wave[TILE_THREADS / 64 + 1] = bl;
    }
    __syncthreads();
    base_t = s_wave[TILE_THREADS / 64] + before_t;
    base_l = s_wave[TILE_THREADS / 64 + 1] + before_l;
  }
}

// What a creator leaves behind: its first-seen in its OWN word of the claim with a plain store — everybody else raises
// the claim's other word with atomicMax (raise_first_seen; both zero-initialised, first-seen = the larger of the two),
// so nothing has to be ordered against the publication of the id (a release fence here writes back the L2: measured
// 7x slower) and a creation costs no read-modify-write beyond the compare-and-swap that took the slot — the claim's
// slot, and the slot's second word in one store.
__device__ __forceinline__ void publish_claim(Slot16* tab, unsigned int slot, unsigned int claim, unsigned long long w2,
                                              unsigned int fi, unsigned int* first2,
                                              unsigned int* __restrict__ slot_by_claim) {
  first2[2u * claim + 1u] = fi;
  slot_by_claim[claim] = slot;
  __hip_atomic_store(&tab[slot].w2, w2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The second word of a slot that holds the key while the word is not there yet.  Whoever publishes it does so without
// waiting for anybody, after at most its own workgroup's barrier and atomicAdd, and the caller's workgroup has
// published its own creations before it waits here: there is no cycle.
// Given up: the build fails (ST_MISC), and the word returned — claim 0, no tag, no position — keeps the caller in bounds.
__device__ __forceinline__ unsigned long long await_published(const unsigned long long* w2, unsigned long long* status) {
  for (unsigned int spins = 0;; ++spins) {
    const unsigned long long w = ld_u64(w2);
    if (w != 0ull) return w;
    if (spins > (1u << 22)) {  // seconds: never expected; fail the build instead of hanging
      status[ST_MISC] = 1ull;
      return 1ull;
    }
    __builtin_amdgcn_s_sleep(2);
  }
}

// A window of a found key that may precede the creator's keeps the minimum first-seen.  Plain (possibly stale, at
// worst zero) reads: both words only grow, so a stale value can only cause a superfluous atomicMax, never a missed one.
__device__ __forceinline__ void raise_first_seen(unsigned int* first2, unsigned int claim, unsigned int fi) {
  if (x_first_inv(first2, claim) < fi) atomicMax(first2 + 2u * claim, fi);
}

// ------------------------------------------------------------------ one-word keys
// Find or create the slot of key w1 starting at `idx`; `v` is the content of that first slot as a PLAIN load
// returned it.
//
// Plain loads are served by the issuing XCD's L2 and may be stale, but a slot only ever moves empty -> w1 -> id, each
// step once: a cached view that shows a foreign key, or our key with its id, is final and is trusted (no fabric
// transaction: agent-scope loads cost one 64-byte fabric request each, ~100 G/s, atomics ~27 G/s, L2 hits ~255 G/s).
// Anything less (empty, id missing) is settled by the compare-and-swap itself or by an agent-scope re-read of w2.
// (Serving the first tiles from a separate launch with agent-scope loads only, so that no L2 caches a hot slot before
// it is complete, was measured and bought nothing.)  The thread whose compare-and-swap sets w1 has created the key.
// No step waits for another thread (lanes of one wave must never wait for each other inside a loop).
// Returns the slot or -1; w2v = the slot's second word as seen (zero: the claim id is not published yet).
// off: the hashed slots are tab[off .. off + mask] (slots below `off` are addressed directly: home slots of the edge
// pass, probed with limit 0 — taken, found or given up after that one slot).
// BUCKET: the slots probed are those of ONE 128-byte line (8 slots), starting at idx and wrapping inside the line —
// the bucket region of the node table (k_nodes_m), probed `limit` + 1 slots deep, after which the key goes to its
// hashed slot.
template <bool BUCKET = false>
__device__ __forceinline__ int x_upsert_one(Slot16* tab, unsigned int mask, unsigned long long w1, unsigned int idx,
                                            ulonglong2 v, unsigned int limit, const unsigned long long* abort_flag,
                                            unsigned long long& w2v, bool& created, unsigned int off = 0u) {
  created = false;
  w2v = 0;
  unsigned int probes = 0;
  while (true) {
    Slot16* s = tab + idx;
    unsigned long long c1 = v.x;
    if (c1 == w1 && (unsigned int)v.y != 0u) {
      w2v = v.y;
      return (int)idx;
    }
    if (c1 == 0ull) {
      c1 = atomicCAS(&s->w1, 0ull, w1);  // looks empty: the compare-and-swap returns the truth
      if (c1 == 0ull) {
        created = true;
        return (int)idx;
      }
    }
    if (c1 == w1) {
      w2v = ld_u64(&s->w2);  // the id is missing in the cached view, or somebody else has just taken the slot for our key
      return (int)idx;
    }
    if (probes >= limit) return -1;
    if ((probes & 63u) == 63u && *reinterpret_cast<const volatile unsigned long long*>(abort_flag)) return -1;
    ++probes;
    idx = BUCKET ? ((idx & ~7u) | ((idx + 1u) & 7u)) : off + ((idx - off + 1u) & mask);
    v = *reinterpret_cast<const ulonglong2*>(tab + idx);
  }
}

// One table phase for the four items of a thread: probe, insert, claim ids, first-seen.  Out: id1[it] = claim id + 1
// of every valid item that has a slot, 0 otherwise; *made = the items that created their key.
// pos: where the items' windows are (TilePos).  homed / off: items whose idx[] is a HOME slot (a directly addressed
// slot below `off`: taken, found, or — when another key sits there — given up for the key's hashed slot in
// tab[off .. off + mask]).
// HOME_PROBES: slots of its line a homed item looks at before it goes to its hashed slot (1: the home slot alone —
// the edge pass; > 1: a bucket line of the node table, k_nodes_m).
// LONE: items of the mask `lone` are keys the caller KNOWS to occur once in the whole input (edge classes with an end
// node of coverage 1): no probe, no compare-and-swap — they take a claim like every creator and write their slot,
// key and id in one 16-byte store, to tab[lone_base + claim] (a region behind the table that is never probed or
// cleared; the ranking reads the key back from there through slot_by_claim like any other).  lone_xs: the shard the
// lone claims of a first tile come from (below).
template <int FSH, int STRIDE = 1, int HOME_PROBES = 1, bool LONE = false>
__device__ __forceinline__ void f_table_phase_one(Slot16* tab, unsigned int mask, unsigned int valid,
                                                  const unsigned long long (&w1)[TILE_ITEMS],
                                                  const unsigned int (&idx)[TILE_ITEMS],
                                                  const ulonglong2 (&v)[TILE_ITEMS], const TilePos<FSH, STRIDE> pos,
                                                  unsigned int* first2, unsigned int* __restrict__ slot_by_claim,
                                                  unsigned long long* ctr, const XShard xs, unsigned int cap,
                                                  unsigned int probe_limit, unsigned long long* status, int which,
                                                  unsigned int (&id1)[TILE_ITEMS], unsigned int* s_wave,
                                                  unsigned int* made, unsigned int homed = 0u, unsigned int off = 0u,
                                                  unsigned int lone = 0u, unsigned int lone_base = 0u,
                                                  XShard lone_xs = XShard{-1, 0u}) {
  unsigned long long w2[TILE_ITEMS];  // the slot's second word as seen
  int slot[TILE_ITEMS];
  // ---- the key with its id, as the first probe load returned it: done (almost every window of a
  // rebuild).  Anything else goes through x_upsert_one below, one item at a time, in ONE copy of that code.
  unsigned int need = 0, created = 0;
#pragma unroll
  for (int it = 0; it < TILE_ITEMS; ++it) {
    id1[it] = 0;
    w2[it] = 0;
    slot[it] = (int)idx[it];
    if (!(valid & (1u << it))) continue;
    if (LONE && (lone & (1u << it))) {  // v[it] was not even loaded
      created |= 1u << it;
      continue;
    }
    if (v[it].x == w1[it] && (unsigned int)v[it].y != 0u)
      w2[it] = v[it].y;
    else
      need |= 1u << it;
  }
  while (need) {
    const int it = __ffs((int)need) - 1;
    need &= need - 1u;
    bool born;
    unsigned long long w2v;
    // (the slot is loaded again rather than picked out of v[]: a register array indexed at run time
    // lives in scratch memory)
    const unsigned int ix = f_pick(idx, it);
    const bool home = (homed >> it) & 1u;
    int sl;
    if (home)
      sl = x_upsert_one<(HOME_PROBES > 1)>(tab, mask, f_pick(w1, it), ix, *reinterpret_cast<const ulonglong2*>(tab + ix),
                                           (unsigned int)(HOME_PROBES - 1), status + ST_OVERFLOW, w2v, born, off);
    else
      sl = x_upsert_one(tab, mask, f_pick(w1, it), ix, *reinterpret_cast<const ulonglong2*>(tab + ix), probe_limit,
                        status + ST_OVERFLOW, w2v, born, off);
    if (sl < 0 && home) {  // other keys live in the home slot(s): this one goes where its key hashes to
      const unsigned int ix2 = off + hashed_slot(f_pick(w1, it), 0u, mask);
      sl = x_upsert_one(tab, mask, f_pick(w1, it), ix2, *reinterpret_cast<const ulonglong2*>(tab + ix2), probe_limit,
                        status + ST_OVERFLOW, w2v, born, off);
    }
    if (sl < 0) {
      status[ST_OVERFLOW] = (unsigned long long)which;
      valid &= ~(1u << it);
    }
#pragma unroll
    for (int j = 0; j < TILE_ITEMS; ++j)
      if (j == it) {
        slot[j] = sl;
        w2[j] = w2v;
      }
    if (born) created |= 1u << it;
  }
  *made = created;
  // ---- claim ids of the workgroup's creators
  unsigned int pre[TILE_ITEMS];
  const unsigned int n = creator_ranks(created, pre);
  unsigned int base = 0, lbase = 0;
  // LONE: the lone classes of a workgroup take the ids after its table creations — or, in the first tiles of the stream
  // (xs = the dense counter), ids of the tile's SHARD like everywhere else: they are never counted (one occurrence, the
  // creator's), and with them kept out, the dense ids hold the genome's classes alone, within the one LDS range of the
  // counting sweeps (with them the head's classes reached 36 k ids and the first-build edge count needed a second
  // sweep of 0.13 ms)
  XShard lxs = xs;
  if constexpr (LONE) {
    unsigned int lpre[TILE_ITEMS];  // pre[] ranks all creators of the wave: split it into the lone ones and the table's
    const unsigned int nl = creator_ranks(lone, lpre);
#pragma unroll
    for (int it = 0; it < TILE_ITEMS; ++it) pre[it] = ((lone >> it) & 1u) ? lpre[it] : pre[it] - lpre[it];
    const bool split = xs.shard == (int)F_SHARDS && lone_xs.shard >= 0;  // workgroup-uniform
    if (split) lxs = XShard{lone_xs.shard, xs.base};
    workgroup_claim_bases(n - nl, nl, xs.counter(ctr), split ? lxs.counter(ctr) : nullptr, s_wave, base, lbase);
  } else {
    base = workgroup_claim_base(n, xs.counter(ctr), s_wave);
  }
  if (created) {
#pragma unroll
    for (int it = 0; it < TILE_ITEMS; ++it)
      if (created & (1u << it)) {
        const bool is_lone = LONE && ((lone >> it) & 1u);
        const unsigned int claim = checked_claim(is_lone ? lxs : xs, (is_lone ? lbase : base) + pre[it], cap, status, which);
        id1[it] = claim + 1u;
        const unsigned long long pub = ((unsigned long long)pos.fi(it) << 32) | (unsigned long long)(claim + 1u);
        if (is_lone) {
          first2[2u * claim + 1u] = pos.fi(it);
          slot_by_claim[claim] = lone_base + claim;
          *reinterpret_cast<ulonglong2*>(tab + lone_base + claim) = make_ulonglong2(w1[it], pub);
        } else {
          publish_claim(tab, (unsigned int)slot[it], claim, pub, pos.fi(it), first2, slot_by_claim);
        }
      }
  }
  // ---- found keys: wait for an id that is still on its way, then keep the minimum first-seen
  unsigned int check = 0;
#pragma unroll
  for (int it = 0; it < TILE_ITEMS; ++it) {
    if (!(valid & (1u << it)) || (created & (1u << it))) continue;
    if (w2[it] == 0ull) w2[it] = await_published(&tab[slot[it]].w2, status);
    id1[it] = (unsigned int)w2[it];
    if (pos.fi(it) > (unsigned int)(w2[it] >> 32)) check |= 1u << it;  // can this window precede the creator's?
  }
#pragma unroll
  for (int it = 0; it < TILE_ITEMS; ++it)
    if (check & (1u << it)) raise_first_seen(first2, id1[it] - 1u, pos.fi(it));
}

// ------------------------------------------------------------------ two-word keys: the slot is owned through w1
// The thread whose compare-and-swap takes w1 OWNS the slot; the second word — tag, coarse position, claim id — arrives
// in ONE store when the id is published: two memory-side operations per creation (a first build makes 5.4 M keys, and
// the rate at which the memory side executes them is what a first build costs over a rebuild).  A slot is empty, owned
// (w1 set, w2 zero) or published (w2 complete, never changed again).  A thread that
// finds w1 equal to its own while w2 is still zero cannot tell yet whether the slot holds its key (the low 63 bits agree;
// the tag decides): it remembers the slot and looks again AFTER its own workgroup has published this round's creations —
// the owner publishes after its workgroup's barrier and one atomicAdd, waiting for nobody, so there is no cycle — and
// if the tag turns out to be another key's it goes on probing by itself (a key it then creates takes its claim id with
// an atomicAdd of its own).  That needs two keys that agree in 63 bits to meet in one probe chain while one of them
// is unpublished: rare, but it has to be right.
// state: 0 found (w2v complete), 1 created (this thread owns the slot), 2 pending (w1 equal, w2 not published yet)
template <bool BUCKET>
__device__ __forceinline__ int x_upsert_own(Slot16* tab, unsigned int mask, unsigned long long w1, unsigned int tag,
                                            unsigned int idx, ulonglong2 v, unsigned int limit,
                                            const unsigned long long* abort_flag, unsigned long long& w2v, int& state,
                                            unsigned int off = 0u) {
  state = 0;
  w2v = 0;
  unsigned int probes = 0;
  while (true) {
    Slot16* s = tab + idx;
    unsigned long long c1 = v.x, c2 = v.y;
    if (c1 == 0ull) {
      c1 = atomicCAS(&s->w1, 0ull, w1);  // looks empty: the CAS returns the truth
      if (c1 == 0ull) {
        state = 1;
        return (int)idx;
      }
      c2 = 0ull;  // (whatever the cached view said about w2 belongs to no key yet)
    }
    if (c1 == w1) {
      if (c2 == 0ull) c2 = ld_u64(&s->w2);  // not published in the view we have: one look with agent scope
      if (c2 == 0ull) {
        state = 2;
        return (int)idx;
      }
      if ((unsigned int)(c2 >> 32) == tag) {  // (a published second word is complete and final)
        w2v = c2;
        return (int)idx;
      }
    }
    if (probes >= limit) return -1;
    if ((probes & 63u) == 63u && *reinterpret_cast<const volatile unsigned long long*>(abort_flag)) return -1;
    ++probes;
    idx = BUCKET ? ((idx & ~7u) | ((idx + 1u) & 7u)) : off + ((idx - off + 1u) & mask);
    v = *reinterpret_cast<const ulonglong2*>(tab + idx);
  }
}

// The table phase of f_table_phase_one for two-word keys (no lone items; xf: the fields of the second word).
template <int FSH, int STRIDE = 1, int HOME_PROBES = 1>
__device__ __forceinline__ void f_table_phase_own(Slot16* tab, unsigned int mask, unsigned int valid,
                                                  const unsigned long long (&w1)[TILE_ITEMS],
                                                  const unsigned int (&tag)[TILE_ITEMS],
                                                  const unsigned int (&idx0)[TILE_ITEMS],
                                                  const ulonglong2 (&v)[TILE_ITEMS], const TilePos<FSH, STRIDE> pos,
                                                  const XW2 f, unsigned int* first2,
                                                  unsigned int* __restrict__ slot_by_claim, unsigned long long* ctr,
                                                  const XShard xs, unsigned int cap, unsigned int probe_limit,
                                                  unsigned long long* status, int which, unsigned int (&id1)[TILE_ITEMS],
                                                  unsigned int* s_wave, unsigned int* made, unsigned int homed = 0u,
                                                  unsigned int off = 0u) {
  // a key that met a pending slot in its bucket line goes straight to its hashed slot in the redo rounds below: with
  // more than one slot of the line probed, a later thread could create the same key in the line's NEXT slot (two claims
  // for one key).  One probe per line is what was measured fastest anyway.
  static_assert(HOME_PROBES == 1, "the own-slot protocol looks at one slot of a bucket line");
  unsigned long long* const myctr = xs.counter(ctr);
  int slot[TILE_ITEMS];  // where the item is: its slot once settled, the slot to go on from while it is not
  unsigned int need = 0, at_home = homed;
  // (id1[] holds the low half of the published second word of a FOUND key until the end, claim id + 1 of a created one)
#pragma unroll
  for (int it = 0; it < TILE_ITEMS; ++it) {
    id1[it] = 0;
    slot[it] = (int)idx0[it];
    if (!(valid & (1u << it))) continue;
    const unsigned long long c1 = v[it].x, c2 = v[it].y;
    // the key with its id, as the first probe load returned it: done (almost every window of a rebuild)
    if (c1 == w1[it] && (unsigned int)(c2 >> 32) == tag[it] && (unsigned int)c2 != 0u)
      id1[it] = (unsigned int)c2;
    else
      need |= 1u << it;
  }
  // ---- the round every workgroup runs: one item at a time through the table from slot[it] on, in ONE copy of that
  // code — found / created / pending
  unsigned int created = 0, pending = 0;
  while (need) {
    const int it = __ffs((int)need) - 1;
    need &= need - 1u;
    int state;
    unsigned long long w2v;
    const unsigned long long kw = f_pick(w1, it);
    const unsigned int ix = (unsigned int)f_pick(slot, it);
    const unsigned int tg = f_pick(tag, it);
    int sl;
    if ((at_home >> it) & 1u) {
      sl = x_upsert_own<(HOME_PROBES > 1)>(tab, mask, kw, tg, ix, *reinterpret_cast<const ulonglong2*>(tab + ix),
                                           (unsigned int)(HOME_PROBES - 1), status + ST_OVERFLOW, w2v, state, off);
      if (sl < 0) {  // other keys live in the home slot(s): this one goes where its key hashes to
        at_home &= ~(1u << it);
        const unsigned int ix2 = off + hashed_slot(kw, tg, mask);
        sl = x_upsert_own<false>(tab, mask, kw, tg, ix2, *reinterpret_cast<const ulonglong2*>(tab + ix2), probe_limit,
                                 status + ST_OVERFLOW, w2v, state, off);
      }
    } else {
      sl = x_upsert_own<false>(tab, mask, kw, tg, ix, *reinterpret_cast<const ulonglong2*>(tab + ix), probe_limit,
                               status + ST_OVERFLOW, w2v, state, off);
    }
    if (sl < 0) {
      status[ST_OVERFLOW] = (unsigned long long)which;
      valid &= ~(1u << it);
      state = 0;
      w2v = 0;
    }
#pragma unroll
    for (int j = 0; j < TILE_ITEMS; ++j)
      if (j == it) {
        slot[j] = sl;
        id1[j] = (unsigned int)w2v;
      }
    if (sl >= 0 && state == 1) created |= 1u << it;
    if (sl >= 0 && state == 2) pending |= 1u << it;
  }
  unsigned int made_all = created;
  // claim ids of the round's creators and their publication
  {
    unsigned int pre[TILE_ITEMS];
    const unsigned int n = creator_ranks(created, pre);
    const unsigned int base = workgroup_claim_base(n, myctr, s_wave);
    if (created) {
#pragma unroll
      for (int it = 0; it < TILE_ITEMS; ++it)
        if (created & (1u << it)) {
          const unsigned int claim = checked_claim(xs, base + pre[it], cap, status, which);
          id1[it] = claim + 1u;
          publish_claim(tab, (unsigned int)slot[it], claim, publish_word_two(tag[it], pos.tpos(it), claim, f), pos.fi(it),
                        first2, slot_by_claim);
        }
    }
  }
  // the slots that were owned but not published when this thread met them
  unsigned int redo = 0;
#pragma unroll
  for (int it = 0; it < TILE_ITEMS; ++it) {
    if (!(pending & (1u << it))) continue;
    const unsigned long long w = await_published(&tab[slot[it]].w2, status);
    if ((unsigned int)(w >> 32) == tag[it])
      id1[it] = (unsigned int)w;
    else
      redo |= 1u << it;  // another key with the same low 63 bits lives there
  }
  // ---- an item that met a half-equal key (the same low 63 bits, another tag) goes on from the next slot BY ITSELF:
  // rare, so a key it creates takes its claim id with an atomicAdd of its own instead of the workgroup's scan — no
  // barrier, nobody else involved.  One step per loop iteration and lane (probe a slot, or look once more at a second
  // word that is not there yet — which is why this loop does not call await_published): a lane that has just taken a
  // slot publishes in the same iteration, so no lane of a wave ever spins waiting for another lane of the same wave.
  // (The slot the item stopped at holds its own w1.)
  while (redo) {
    const int it = __ffs((int)redo) - 1;
    redo &= redo - 1u;
    const unsigned int stopped = (unsigned int)f_pick(slot, it);
    const unsigned long long kw = tab[stopped].w1;
    const unsigned int tg = f_pick(tag, it);
    unsigned int at;
    if ((at_home >> it) & 1u) {
      at_home &= ~(1u << it);
      at = off + hashed_slot(kw, tg, mask);
    } else {
      at = off + ((stopped - off + 1u) & mask);
    }
    unsigned int got = 0, probes = 0, polls = 0;
    bool born = false, lost = false;
    while (true) {
      Slot16* sp = tab + at;
      unsigned long long c1 = sp->w1, c2 = 0ull;
      if (c1 == 0ull) {
        c1 = atomicCAS(&sp->w1, 0ull, kw);
        if (c1 == 0ull) {  // taken: claim id, first-seen, publication — all in this iteration
          const unsigned int claim = checked_claim(xs, (unsigned int)atomicAdd(myctr, 1ull), cap, status, which);
          publish_claim(tab, at, claim, publish_word_two(tg, pos.tpos(it), claim, f), pos.fi(it), first2, slot_by_claim);
          got = claim + 1u;
          born = true;
          break;
        }
      }
      if (c1 == kw) {
        c2 = ld_u64(&sp->w2);
        if (c2 == 0ull) {  // owned, not published yet: look again in the next iteration
          if (++polls > (1u << 22)) {  // (as await_published gives up)
            status[ST_MISC] = 1ull;
            lost = true;
            break;
          }
          __builtin_amdgcn_s_sleep(2);
          continue;
        }
        if ((unsigned int)(c2 >> 32) == tg) {
          got = (unsigned int)c2;
          break;
        }
      }
      if (++probes > probe_limit) {
        lost = true;
        break;
      }
      at = off + ((at - off + 1u) & mask);
    }
    if (lost) {
      status[ST_OVERFLOW] = (unsigned long long)which;
      valid &= ~(1u << it);
    }
    if (born) made_all |= 1u << it;
#pragma unroll
    for (int j = 0; j < TILE_ITEMS; ++j)
      if (j == it) {
        slot[j] = (int)at;
        id1[j] = got;
      }
  }
  *made = made_all;
  // ---- found keys: keep the minimum first-seen (can this window precede the creator's?  coarse positions: same or
  // earlier bucket); id1 turns from the slot's second word into claim id + 1
  unsigned int check = 0;
#pragma unroll
  for (int it = 0; it < TILE_ITEMS; ++it) {
    if (!(valid & (1u << it))) {
      id1[it] = 0;
      continue;
    }
    if (made_all & (1u << it)) continue;
    const unsigned int lw = id1[it];
    id1[it] = xw2_id1(lw, f);
    if ((pos.tpos(it) >> f.cshift) <= (lw >> f.ib)) check |= 1u << it;
  }
#pragma unroll
  for (int it = 0; it < TILE_ITEMS; ++it)
    if (check & (1u << it)) raise_first_seen(first2, id1[it] - 1u, pos.fi(it));
}

// field widths of a two-word slot's second word for `max_claims` ids over T tokens
static inline XW2 xw2_for(size_t max_claims, long long T) {
  XW2 f;
  f.ib = ilog2_ceil((uint64_t)max_claims + 2);
  if (f.ib > 31) f.ib = 31;  // claims < 2^30 (slots are capped there)
  const int cb = 32 - f.ib;  // bits left for the coarse position (0: every window checks first-seen)
  const int tb = ilog2_ceil((uint64_t)(T > 0 ? T : 1) + 1);
  f.cshift = cb <= 0 ? 31 : (tb > cb ? tb - cb : 0);
  return f;
}
