// amg_bases.h — what every kernel that walks nucleotide bases shares (amg_sketch.hip: k_minhash and k_bs_*;
// amg_kcount.hip: k_kc_insert / k_kc_query / k_kc_emit):
//   km_*         a k-mer (k <= 32) as up to four 64-bit words: cut out of bases staged in LDS, reverse-complemented,
//                compared and hashed a WORD at a time
//   BaseStream   a stream of bases cut into segments, last_offset_le the search for a position's segment
//   base_tile    the tile walker: 1024 window starts + their halo staged once, every thread's four windows keyed
//                by the caller's function (the sketch's hash, the counts' packed key)
//   block_emit   the survivors of a tile compacted behind one shared counter
//   host side    km_max_hash (the scaled cut), offsets_check, KM_BY_WORDS (a kernel by the words of its k-mers)
//
// sourmash's sketch (amg_sketch.hip holds the definition and its source): canonical k-mer = the bytewise smaller of
// the k-mer and its reverse complement, hash = first 64 bits of MurmurHash3_x64_128(canonical k-mer, seed 42).  A
// k-mer that holds a character outside ACGT is skipped (force = True).
//
// A byte loop per k-mer (cut the window, copy it, build the reverse complement, compare, feed the hash a byte at a
// time out of a private array) is ~400 instructions and a round trip through scratch memory per base.  Here the staged
// bases are ASCII upper case with 0 for anything outside ACGT; a k-mer is NW + 1 aligned LDS words funnel-shifted into
// NW; "no 0 byte" is one SWAR test per word; the complement of eight bases is three logic operations
// (A 0x41 <-> T 0x54 differ by 0x15, C 0x43 <-> G 0x47 by 0x04, and bit 1 tells the two pairs apart); the reversal is
// a byte swap per word and one funnel shift by the padding; MurmurHash3 takes its 8-byte blocks as they are.
#pragma once
#include "amg_device.h"

#define KM_MAX_K 32

// what the staging loop stores for a base: upper-case A / C / G / T, 0 for everything else
__device__ __forceinline__ unsigned char km_stage(unsigned char c) {
  if (c >= 'a' && c <= 'z') c = (unsigned char)(c - 32);
  return (c == 'A' || c == 'C' || c == 'G' || c == 'T') ? c : (unsigned char)0;
}

__device__ __forceinline__ unsigned long long km_rotl(unsigned long long x, int r) { return (x << r) | (x >> (64 - r)); }
__device__ __forceinline__ unsigned long long km_fmix(unsigned long long k) {
  k ^= k >> 33;
  k *= 0xFF51AFD7ED558CCDull;
  k ^= k >> 33;
  k *= 0xC4CEB9FE1A85EC53ull;
  k ^= k >> 33;
  return k;
}

// bytes [0, n) of a word kept, the rest cleared (n in 0 .. 8)
__device__ __forceinline__ unsigned long long km_low_bytes(unsigned long long x, int n) {
  return n >= 8 ? x : (n <= 0 ? 0ull : x & ((1ull << (8 * n)) - 1ull));
}

// The k-mer that starts at byte i of `lds` (8-byte aligned, at least 8 readable bytes behind the k-mer's last word) as
// NW little-endian words, bytes beyond k cleared.  Returns false when a base outside ACGT is among its k.
template <int NW>
__device__ __forceinline__ bool km_load(const unsigned char* lds, int i, int k, unsigned long long (&f)[NW]) {
  const unsigned long long* W = reinterpret_cast<const unsigned long long*>(lds + (i & ~7));
  const int s8 = (i & 7) * 8;
  unsigned long long x[NW + 1];
#pragma unroll
  for (int j = 0; j <= NW; ++j) x[j] = W[j];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < NW; ++j) {
    unsigned long long v = s8 ? (x[j] >> s8) | (x[j + 1] << (64 - s8)) : x[j];
    const int n = k - 8 * j;   // bytes of the k-mer in this word (>= 1)
    v = km_low_bytes(v, n);
    f[j] = v;
    const unsigned long long t = n >= 8 ? v : v | (~0ull << (8 * n));   // padding must not look like a bad base
    ok = ok && (((t - 0x0101010101010101ull) & ~t & 0x8080808080808080ull) == 0ull);
  }
  return ok;
}

// complement of eight staged bases (bytes that are 0 come out as rubbish: the caller masks)
__device__ __forceinline__ unsigned long long km_comp8(unsigned long long x) {
  return x ^ 0x1515151515151515ull ^ (((x >> 1) & 0x0101010101010101ull) * 0x11ull);
}

// reverse complement of a k-mer of NW words: the 8 NW bytes reversed (word order + a byte swap each) put the k-mer's
// last base first after `pad` = 8 NW - k bytes of padding, which one funnel shift removes
template <int NW>
__device__ __forceinline__ void km_revcomp(const unsigned long long (&f)[NW], int k, unsigned long long (&r)[NW]) {
  const int pad8 = (8 * NW - k) * 8;
  unsigned long long t[NW + 1];
#pragma unroll
  for (int j = 0; j < NW; ++j) t[j] = __builtin_bswap64(f[NW - 1 - j]);
  t[NW] = 0ull;
#pragma unroll
  for (int j = 0; j < NW; ++j) {
    const unsigned long long v = pad8 ? (t[j] >> pad8) | (t[j + 1] << (64 - pad8)) : t[j];
    r[j] = km_low_bytes(km_comp8(v), k - 8 * j);
  }
}

// a <= b as byte strings (the first byte is the low byte of word 0)
template <int NW>
__device__ __forceinline__ bool km_not_greater(const unsigned long long (&a)[NW], const unsigned long long (&b)[NW]) {
#pragma unroll
  for (int j = 0; j < NW; ++j) {
    if (a[j] != b[j]) return __builtin_bswap64(a[j]) < __builtin_bswap64(b[j]);
  }
  return true;
}

// first 64 bits of MurmurHash3_x64_128 (Austin Appleby, public domain) of the k bytes held in NW words
template <int NW>
__device__ __forceinline__ unsigned long long km_murmur_h1(const unsigned long long (&x)[NW], int len, unsigned long long seed) {
  const unsigned long long c1 = 0x87C37B91114253D5ull, c2 = 0x4CF5AD432745937Full;
  unsigned long long h1 = seed, h2 = seed;
  int used = 0;
  if constexpr (NW >= 2) {
#pragma unroll
    for (int blk = 0; blk + 1 < NW; blk += 2) {
      if (len - 8 * blk >= 16) {
        unsigned long long k1 = x[blk], k2 = x[blk + 1];
        k1 *= c1; k1 = km_rotl(k1, 31); k1 *= c2; h1 ^= k1;
        h1 = km_rotl(h1, 27); h1 += h2; h1 = h1 * 5 + 0x52DCE729ull;
        k2 *= c2; k2 = km_rotl(k2, 33); k2 *= c1; h2 ^= k2;
        h2 = km_rotl(h2, 31); h2 += h1; h2 = h2 * 5 + 0x38495AB5ull;
        used = blk + 2;
      }
    }
  }
  const int t = len - 8 * used;   // 0 .. 15 bytes of tail, in words used and used + 1 (cleared beyond the k-mer)
  unsigned long long k1 = 0ull, k2 = 0ull;
#pragma unroll
  for (int j = 0; j < NW; ++j) {
    if (j == used) k1 = x[j];
    if (j == used + 1) k2 = x[j];
  }
  if (t > 8) { k2 *= c2; k2 = km_rotl(k2, 33); k2 *= c1; h2 ^= k2; }
  if (t > 0) { k1 *= c1; k1 = km_rotl(k1, 31); k1 *= c2; h1 ^= k1; }
  h1 ^= (unsigned long long)len;
  h2 ^= (unsigned long long)len;
  h1 += h2; h2 += h1;
  h1 = km_fmix(h1); h2 = km_fmix(h2);
  h1 += h2;
  return h1;
}

// hash of the canonical form of the k-mer at byte i of the staged bases; false: skipped (a base outside ACGT)
template <int NW>
__device__ __forceinline__ bool km_canonical_hash(const unsigned char* lds, int i, int k, unsigned long long* out) {
  unsigned long long f[NW], r[NW];
  if (!km_load<NW>(lds, i, k, f)) return false;
  km_revcomp<NW>(f, k, r);
  *out = km_not_greater<NW>(f, r) ? km_murmur_h1<NW>(f, k, 42ull) : km_murmur_h1<NW>(r, k, 42ull);
  return true;
}

// ------------------------------------------------------------------ a stream of bases, walked in tiles
// segment s is stream[seg_off[s] .. seg_off[s + 1]) and lies at bases[seg_src[s] ..] (seg_src == nullptr: nothing is
// gathered, the stream is `bases` itself)
struct BaseStream {
  const unsigned char* bases;
  long long n_bases;
  const long long* seg_off;
  long long n_seg;
  const long long* seg_src;
};

// the last offset <= t among off[lo .. hi): off[lo] <= t < off[hi] on entry
__device__ __forceinline__ long long last_offset_le(const long long* off, long long lo, long long hi, long long t) {
  while (hi - lo > 1) {
    const long long mid = (lo + hi) >> 1;
    if (off[mid] <= t) lo = mid; else hi = mid;
  }
  return lo;
}

#define BT_TILE 1024  // window starts per workgroup of 256 threads

// what base_tile hands a thread for its window starts t0 + threadIdx.x + 256 it: whether a valid window starts there
// (inside one segment, no base outside ACGT), its key and its segment
struct BaseWin {
  bool valid[4];
  unsigned long long key[4];
  long long seg[4];
};

// Stages the tile that starts at stream position t0 (BT_TILE + k - 1 bases: upper case, 0 for anything outside ACGT)
// and keys every thread's four windows with KEY: km_canonical_hash<NW> for a sketch, amg_kcount.hip's kc_key<NW> for
// the counts (NW = (k + 7) / 8).  The tile's segments are found by two searches over all offsets per block, then every
// thread looks among those few (a search over all of them per window was half of k_minhash's time).  Where nothing is
// gathered the staging does not wait for them: one barrier.  A gathered base needs its segment: search, barrier,
// stage, barrier.  All 256 threads call.
template <bool GATHER, bool (*KEY)(const unsigned char* lds, int i, int k, unsigned long long* key)>
__device__ __forceinline__ void base_tile(const BaseStream& s, int k, long long t0, BaseWin& w) {
  constexpr int STAGED = BT_TILE + KM_MAX_K + 24;
  __shared__ __attribute__((aligned(8))) unsigned char s_b[STAGED];
  __shared__ long long s_seg[2];
  if constexpr (!GATHER)
    for (int i = threadIdx.x; i < STAGED; i += 256) {
      const long long t = t0 + i;
      s_b[i] = (i < BT_TILE + k - 1 && t < s.n_bases) ? km_stage(s.bases[t]) : (unsigned char)0;
    }
  if (threadIdx.x < 2) {
    const long long t = threadIdx.x == 0 ? t0 : (t0 + BT_TILE - 1 < s.n_bases ? t0 + BT_TILE - 1 : s.n_bases - 1);
    s_seg[threadIdx.x] = last_offset_le(s.seg_off, 0, s.n_seg, t);
  }
  __syncthreads();
  const long long seg_lo = s_seg[0], seg_hi = s_seg[1] + 1;
  if constexpr (GATHER) {
    for (int i = threadIdx.x; i < STAGED; i += 256) {
      const long long t = t0 + i;
      unsigned char b = 0;
      if (i < BT_TILE + k - 1 && t < s.n_bases) {
        const long long g = last_offset_le(s.seg_off, seg_lo, seg_hi, t);
        // (a halo byte behind the tile's last segment belongs to no window that starts in this tile)
        if (t < s.seg_off[g + 1]) b = km_stage(s.bases[s.seg_src[g] + (t - s.seg_off[g])]);
      }
      s_b[i] = b;
    }
    __syncthreads();
  }
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int i = threadIdx.x + it * 256;
    const long long t = t0 + i;
    w.valid[it] = false;
    w.key[it] = 0ull;
    w.seg[it] = 0;
    if (t + k > s.n_bases) continue;
    w.seg[it] = last_offset_le(s.seg_off, seg_lo, seg_hi, t);
    if (t + k > s.seg_off[w.seg[it] + 1]) continue;  // the window runs over the end of its segment
    w.valid[it] = KEY(s_b, i, k, &w.key[it]);
  }
}

// The survivors of a tile (bit `it` of keep: this thread's window `it` stays) get consecutive places behind *counter:
// a block scan and one returning atomicAdd per block.  store(place, it) is called for the places below cap only;
// *counter still ends at the number of survivors there were.  All 256 threads call.
template <class Store>
__device__ __forceinline__ void block_emit(unsigned int keep, unsigned long long* counter, long long cap, Store store) {
  __shared__ unsigned int s_wave[4];
  __shared__ unsigned long long s_base;
  unsigned int total;
  const unsigned int off = block_exscan_256((unsigned int)__popc(keep), &total, s_wave);
  if (threadIdx.x == 0) s_base = total ? atomicAdd(counter, (unsigned long long)total) : 0ull;
  __syncthreads();
  unsigned long long o = s_base + off;
#pragma unroll
  for (int it = 0; it < 4; ++it)
    if (keep & (1u << it)) {
      if ((long long)o < cap) store(o, it);
      ++o;
    }
}

// ------------------------------------------------------------------ host side
// sourmash (>= 4, Rust core: max_hash_for_scaled): 2^64 - 1 for scaled 1, otherwise (u64::MAX as f64 / scaled as f64)
// as u64 — a truncation.  (The old Python helper rounded; the two agree whenever the quotient is >= 2^53, i.e. for
// scaled <= 2048, which covers the reference's 1 and 10.)  scaled >= 1.
static inline unsigned long long km_max_hash(uint64_t scaled) {
  if (scaled <= 1) return ~0ull;
  const double q = 18446744073709551616.0 / (double)scaled;  // u64::MAX as f64 == 2^64
  return q >= 18446744073709551615.0 ? ~0ull : (unsigned long long)q;
}

// offsets of n pieces start at 0 and never decrease; the two messages are the caller's
static inline int offsets_check(const int64_t* off, int64_t n, const char* not_zero, const char* not_monotone) {
  if (off[0] != 0) return amg_fail(AMG_E_ARG, "%s", not_zero);
  for (int64_t s = 0; s < n; ++s)
    if (off[s + 1] < off[s]) return amg_fail(AMG_E_ARG, "%s", not_monotone);
  return AMG_OK;
}

// `expr` with NW = the words of a k-mer of k bases (1 .. 4): a kernel's instantiation, say
#define KM_BY_WORDS(k, expr) \
  ((k) <= 8 ? [&] { constexpr int NW = 1; return expr; }() : (k) <= 16 ? [&] { constexpr int NW = 2; return expr; }() \
   : (k) <= 24 ? [&] { constexpr int NW = 3; return expr; }() : [&] { constexpr int NW = 4; return expr; }())
