// amg_scan.hip — exclusive prefix sums in ONE launch (decoupled look-back, hand-written for wave64).
//
// The passes scan short arrays all the time (flags -> positions, counts -> offsets: ~18 scans per cleaning
// sweep over 0.5 - 20 M elements).  A library scan is two launches (state initialisation + scan) through a
// generic dispatch layer; here a scan is one kernel and needs no initialisation launch:
//   * a workgroup takes its tile number from a counter that only ever grows (tile = ticket - the number of
//     tiles all earlier scans used: the host keeps that sum), so tiles start in order and a tile never waits for
//     one that has not started;
//   * a tile publishes {state, epoch, value} as ONE 64-bit word with a relaxed agent-scope store — value and
//     flag travel together, so no fence is needed (a release fence writes the XCD's L2 back) — first its own
//     sum (state 1), then its inclusive prefix (state 2); the status words are never cleared: a word whose
//     epoch is not the current scan's is simply "not there yet" (the buffer is zeroed when the 14-bit epoch wraps);
//   * the first wave of a tile looks back 64 predecessors at a time until it meets an inclusive prefix.
// Values are sums of non-negative counts below 2^48.
//
// What a tile HOLDS is the loader's business.  A lane takes E consecutive elements per row with one vector load
// (16 bytes where the element allows it), scans them serially in registers and gives only their sum to the
// row / wave / tile scan; at emit time every element gets the row's prefix plus the running sum inside the lane.  A
// wave's row is 64 E consecutive elements, a tile SC_THREADS x ROWS x E:
//
//   loader                                                  E   ROWS   elements per tile
//   LoadByteSet                                            16     2        16 384
//   LoadApplyKill                                           8     2         8 192
//   LoadArr<u32> LoadArrN<u32> LoadNonzero LoadBitsPopc     4     4         8 192
//   LoadArr<i64> LoadArrN<i64> LoadPairWidth<2>             2     8         8 192
//   LoadFlagWords (32 bytes per element)                    2     8         8 192
//   LoadPairWidth<1> (with EmitEdges)                       1    16         8 192
//
// The rows are what was measured to be fastest on the sweep of bench.py (profiles/scan_lanes_NOTES.md), and they say
// where a scan's time goes.  It is not the tickets and the look-back: with 8 rows for every loader (tiles of 65 536
// bytes, 16 384 words) the small scans were up to twice as slow as with one element per lane and 8 192-element tiles,
// because an array of a few MB then keeps a few dozen of the 256 CUs busy, and the side clears, which the scan's
// workgroups share, had 192 workgroups instead of 1 536.  What pays is the lane group itself: 1 / E of the cross-lane
// steps per element (32-bit ones where the wave's sum fits), 1 / E of the load instructions, half the registers or
// less, so more waves per SIMD.  So E is as wide as a 16-byte load, and ROWS brings the tile back to 8 192 elements
// (bytes: 16 384).  Where every element writes scattered words (EmitEdges), consecutive elements in one lane make a
// wave's stores touch twice the lines: one element per lane there, as before.
//
// Inputs are carve-outs of scratch buffers as often as whole allocations, so a base pointer may sit anywhere.  The
// lanes' groups are laid on the ALIGNED grid of the array: with `mis` = the elements by which the base lies past a
// vector boundary, lane group g holds elements [g E - mis, g E - mis + E), and the tiles cover n + mis positions.
// A wave whose span lies inside the array loads vectors; the waves that hold the head (mis elements before the
// array) or the tail take element-wise loads of clamped indices, so no load touches a byte outside
// [in, in + lim) and no store one outside the output's n elements.
#include <type_traits>

#include "amg_rows.h"

#define SC_THREADS 512  // 8 waves per workgroup
#define SC_VAL_MASK ((1ull << 48) - 1ull)

__device__ __forceinline__ unsigned long long sc_word(unsigned int state, unsigned int epoch, unsigned long long v) {
  return ((unsigned long long)state << 62) | ((unsigned long long)(epoch & 0x3fffu) << 48) | (v & SC_VAL_MASK);
}

// What is scanned is what a LOADER makes of element i — an array entry, or something computed on the way that would
// otherwise be a kernel of its own writing an array only the scan reads (the passes launch ~150 kernels per cleaning
// sweep and every launch costs ~5 us however little it does):
//   LoadArr<T>      in[i]
//   LoadFlagWords   the ranking bitmaps of amg_build_x.hip / amg_dist.hip: 32 flag bytes folded into bitmap word i
//                   (stored as a side effect), the value scanned is its popcount
//   LoadBitsPopc    popcount of bitmap word i
//   LoadPairWidth   directed edges of edge class i: a self-loop has one, every other class two
//   LoadArrN<T>, LoadNonzero, LoadByteSet   in[i] / (in[i] != 0) with the terminator built in
// What happens to the exclusive prefix of element i of the first array is an EMITTER's business: EmitOut stores it in
// out[i]; a compaction's emitter scatters element i to its place itself, so no position array is written and read back
// by a kernel of its own (EmitEdges, EmitLiveKeys).  A scan may also zero a few ranges no scan element touches (`side`,
// grid-stride over its workgroups, after their tiles are published): the clear_many launch before it goes away.
// Two scans that do not depend on each other travel as ONE launch (k_exscan<LA, LB>: tiles [0, tiles_a) scan the first
// array, the tiles behind them the second, whose look-back stops at its own first tile); each array has the tile size
// of its own loader.
//
// A loader says
//   E, ROWS, BATCH   elements per lane and row, rows per wave, rows whose loads are in flight together
//   Sum              the type a WAVE's sum of values fits in (32 bits halve the cross-lane steps)
//   lim()            elements from here on count 0 and are not loaded
//   mis()            elements by which the base lies past a vector boundary, 0 <= mis < E
//   vec()            whether the aligned groups may be loaded as vectors at all
// and is used in two steps, so that the loads of a wave's rows are all in flight before the first is waited for:
// raw_vec(i0) / raw_elems(i0, lim) only load the group [i0, i0 + E) — the first as one vector (the group lies inside
// the array and is aligned), the second element by element from indices clamped into [0, lim) — and
// keep<FULL>(i0, lim, raw) makes the group's values of it, 0 outside [0, lim), in a compact form (Keep: at(k, j) is
// value j, sum(k) their sum) and does any store the loader has (a store between two rows' loads, or a value computed
// inside a bounds check, made every row wait for the one before).  FULL: the whole group lies inside [0, lim).
#define SC_NO_LIM 0x7fffffffffffffffll

__device__ __forceinline__ bool sc_in(long long i, long long lim) { return (unsigned long long)i < (unsigned long long)lim; }
__device__ __forceinline__ long long sc_clamp(long long i, long long lim) { return i < 0 ? 0 : (i < lim ? i : lim - 1); }
template <class T>
__host__ __device__ __forceinline__ int sc_mis(const T* p, int e) {
  return (int)(((unsigned long long)reinterpret_cast<uintptr_t>(p) / sizeof(T)) % (unsigned int)e);
}
// bytes -> 1 where the byte is not 0, four at a time
__device__ __forceinline__ unsigned int sc_nz_bytes(unsigned int w) {
  return ((((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) & 0x80808080u) >> 7;
}

// E elements of T as one 16-byte (or 8-byte) register group
template <class T, int E_>
struct alignas(sizeof(T) * E_) ScPack {
  T v[E_];
};
template <class T, int E_>
__device__ __forceinline__ ScPack<T, E_> sc_pack_vec(const T* in, long long i0) {
  return *reinterpret_cast<const ScPack<T, E_>*>(in + i0);
}
template <class T, int E_>
__device__ __forceinline__ ScPack<T, E_> sc_pack_elems(const T* in, long long i0, long long lim) {
  ScPack<T, E_> p;
#pragma unroll
  for (int j = 0; j < E_; ++j) p.v[j] = in[sc_clamp(i0 + j, lim)];
  return p;
}
template <bool FULL, class T, int E_>
__device__ __forceinline__ ScPack<T, E_> sc_pack_mask(const ScPack<T, E_>& r, long long i0, long long lim) {
  ScPack<T, E_> k;
#pragma unroll
  for (int j = 0; j < E_; ++j) k.v[j] = (FULL || sc_in(i0 + j, lim)) ? r.v[j] : (T)0;
  return k;
}

// a lane group's sum, value by value
template <class L>
__device__ __forceinline__ typename L::Sum sc_sum_at(const typename L::Keep& k) {
  typename L::Sum s = 0;
#pragma unroll
  for (int j = 0; j < L::E; ++j) s += (typename L::Sum)L::at(k, j);
  return s;
}

// what the array loaders share: T in[], E = 16 / sizeof(T) elements per lane, the values kept as loaded
template <class T>
struct ScArr {
  static constexpr int E = 16 / (int)sizeof(T), ROWS = 16 / E, BATCH = ROWS;
  using Raw = ScPack<T, E>;
  using Keep = Raw;
  const T* in;
  __host__ __device__ __forceinline__ int mis() const { return sc_mis(in, E); }
  __device__ __forceinline__ bool vec() const { return true; }
  __device__ __forceinline__ Raw raw_vec(long long i0) const { return sc_pack_vec<T, E>(in, i0); }
  __device__ __forceinline__ Raw raw_elems(long long i0, long long lim) const { return sc_pack_elems<T, E>(in, i0, lim); }
  template <bool FULL>
  __device__ __forceinline__ Keep keep(long long i0, long long lim, const Raw& r) const {
    return sc_pack_mask<FULL>(r, i0, lim);
  }
};
template <class T>
struct LoadArr : ScArr<T> {
  using Sum = unsigned long long;
  using Keep = typename ScArr<T>::Keep;
  __host__ __device__ LoadArr(const T* p) : ScArr<T>{p} {}
  __device__ __forceinline__ long long lim() const { return SC_NO_LIM; }
  static __device__ __forceinline__ unsigned long long at(const Keep& k, int j) { return (unsigned long long)k.v[j]; }
  static __device__ __forceinline__ Sum sum(const Keep& k) { return sc_sum_at<LoadArr<T>>(k); }
};
template <class T>
struct LoadArrN : ScArr<T> {  // in[i] for i < n, 0 from there on (the scan's terminator: no cleared element behind the array)
  using Sum = unsigned long long;
  using Keep = typename ScArr<T>::Keep;
  long long n;
  __host__ __device__ LoadArrN(const T* p, long long n_) : ScArr<T>{p}, n(n_) {}
  __device__ __forceinline__ long long lim() const { return n; }
  static __device__ __forceinline__ unsigned long long at(const Keep& k, int j) { return (unsigned long long)k.v[j]; }
  static __device__ __forceinline__ Sum sum(const Keep& k) { return sc_sum_at<LoadArrN<T>>(k); }
};
struct LoadNonzero : ScArr<unsigned int> {  // 1 where in[i] != 0, i < n
  using Sum = unsigned int;
  long long n;
  __host__ __device__ LoadNonzero(const unsigned int* p, long long n_) : ScArr<unsigned int>{p}, n(n_) {}
  __device__ __forceinline__ long long lim() const { return n; }
  static __device__ __forceinline__ unsigned long long at(const Keep& k, int j) { return k.v[j] != 0u ? 1ull : 0ull; }
  static __device__ __forceinline__ Sum sum(const Keep& k) { return sc_sum_at<LoadNonzero>(k); }
};
struct LoadBitsPopc : ScArr<unsigned int> {
  using Sum = unsigned int;
  long long n_words;
  __host__ __device__ LoadBitsPopc(const unsigned int* p, long long n_) : ScArr<unsigned int>{p}, n_words(n_) {}
  __device__ __forceinline__ long long lim() const { return n_words; }
  static __device__ __forceinline__ unsigned long long at(const Keep& k, int j) { return (unsigned long long)__popc(k.v[j]); }
  static __device__ __forceinline__ Sum sum(const Keep& k) { return sc_sum_at<LoadBitsPopc>(k); }
};
template <int E_>  // (2 for the widths alone; 1 where the classes' edges are written: EmitEdges)
struct LoadPairWidth {
  static constexpr int E = E_, ROWS = 16 / E_, BATCH = ROWS;
  using Sum = unsigned int;
  using Raw = ScPack<unsigned long long, E_>;
  struct Keep {
    unsigned int v[E_];
  };
  const unsigned long long* pkey;
  long long n_pairs;  // elements from here on count 0 (the scan's terminator)
  __device__ __forceinline__ long long lim() const { return n_pairs; }
  __host__ __device__ __forceinline__ int mis() const { return sc_mis(pkey, E); }
  __device__ __forceinline__ bool vec() const { return true; }
  __device__ __forceinline__ Raw raw_vec(long long i0) const { return sc_pack_vec<unsigned long long, E_>(pkey, i0); }
  __device__ __forceinline__ Raw raw_elems(long long i0, long long lim) const {
    return sc_pack_elems<unsigned long long, E_>(pkey, i0, lim);
  }
  template <bool FULL>
  __device__ __forceinline__ Keep keep(long long i0, long long lim, const Raw& r) const {
    Keep k;
#pragma unroll
    for (int j = 0; j < E_; ++j) {
      const unsigned long long key = r.v[j];
      const unsigned int lo = (unsigned int)((key >> 32) & 0x7fffffffull);
      const unsigned int hi = (unsigned int)(key & 0xffffffffull) - 1u;
      k.v[j] = (FULL || sc_in(i0 + j, lim)) ? (lo == hi ? 1u : 2u) : 0u;
    }
    return k;
  }
  static __device__ __forceinline__ unsigned long long at(const Keep& k, int j) { return (unsigned long long)k.v[j]; }
  static __device__ __forceinline__ Sum sum(const Keep& k) { return sc_sum_at<LoadPairWidth<E_>>(k); }
};
struct LoadByteSet {  // 1 where byte i is set, i < n
  static constexpr int E = 16, ROWS = 2, BATCH = ROWS;
  using Sum = unsigned int;
  struct Raw {
    unsigned int w[4];
  };
  using Keep = Raw;  // a byte of 0 or 1 per element
  const unsigned char* in;
  long long n;
  __device__ __forceinline__ long long lim() const { return n; }
  __host__ __device__ __forceinline__ int mis() const { return sc_mis(in, E); }
  __device__ __forceinline__ bool vec() const { return true; }
  __device__ __forceinline__ Raw raw_vec(long long i0) const {
    const uint4 q = *reinterpret_cast<const uint4*>(in + i0);
    return Raw{{q.x, q.y, q.z, q.w}};
  }
  __device__ __forceinline__ Raw raw_elems(long long i0, long long lim) const {
    unsigned int b[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) b[j] = in[sc_clamp(i0 + j, lim)];
    Raw r;
#pragma unroll
    for (int q = 0; q < 4; ++q) r.w[q] = b[4 * q] | (b[4 * q + 1] << 8) | (b[4 * q + 2] << 16) | (b[4 * q + 3] << 24);
    return r;
  }
  template <bool FULL>
  __device__ __forceinline__ Keep keep(long long i0, long long lim, const Raw& r) const {
    Keep k;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      unsigned int m = 0xffffffffu;
      if (!FULL) {
        m = 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) m |= sc_in(i0 + 4 * q + j, lim) ? 0xffu << (8 * j) : 0u;
      }
      k.w[q] = sc_nz_bytes(r.w[q] & m);
    }
    return k;
  }
  static __device__ __forceinline__ unsigned long long at(const Keep& k, int j) {
    return (unsigned long long)((k.w[j >> 2] >> (8 * (j & 3))) & 1u);
  }
  // (counted, not added up value by value: the values would stay in registers from here to the emit)
  static __device__ __forceinline__ Sum sum(const Keep& k) { return (Sum)(__popc(k.w[0]) + __popc(k.w[1]) + __popc(k.w[2]) + __popc(k.w[3])); }
};
struct LoadApplyKill {  // node removal: a marked live node dies; kill[i] is left as "removed now" and counted
  static constexpr int E = 8, ROWS = 2, BATCH = ROWS;
  using Sum = unsigned int;
  struct Raw {
    unsigned int kill[2], alive[2];
  };
  struct Keep {  // a byte of 0 or 1 per element
    unsigned int w[2];
  };
  unsigned char* kill;
  unsigned char* alive;
  long long n;
  __device__ __forceinline__ long long lim() const { return n; }
  __host__ __device__ __forceinline__ int mis() const { return sc_mis(kill, E); }
  // (both arrays are loaded and stored as 8-byte vectors of the same elements: they must sit alike on the 8-byte grid)
  __device__ __forceinline__ bool vec() const {
    return ((reinterpret_cast<uintptr_t>(kill) ^ reinterpret_cast<uintptr_t>(alive)) & 7u) == 0u;
  }
  __device__ __forceinline__ Raw raw_vec(long long i0) const {
    const uint2 k = *reinterpret_cast<const uint2*>(kill + i0), a = *reinterpret_cast<const uint2*>(alive + i0);
    return Raw{{k.x, k.y}, {a.x, a.y}};
  }
  __device__ __forceinline__ Raw raw_elems(long long i0, long long lim) const {
    unsigned int k[8], a[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const long long i = sc_clamp(i0 + j, lim);
      k[j] = kill[i];
      a[j] = alive[i];
    }
    Raw r;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      r.kill[q] = k[4 * q] | (k[4 * q + 1] << 8) | (k[4 * q + 2] << 16) | (k[4 * q + 3] << 24);
      r.alive[q] = a[4 * q] | (a[4 * q + 1] << 8) | (a[4 * q + 2] << 16) | (a[4 * q + 3] << 24);
    }
    return r;
  }
  template <bool FULL>
  __device__ __forceinline__ Keep keep(long long i0, long long lim, const Raw& r) const {
    Keep f;
#pragma unroll
    for (int q = 0; q < 2; ++q) f.w[q] = sc_nz_bytes(r.kill[q]) & sc_nz_bytes(r.alive[q]);
    if (FULL) {
      *reinterpret_cast<uint2*>(kill + i0) = uint2{f.w[0], f.w[1]};
      if (f.w[0] | f.w[1])  // (the dying nodes' bytes go to 0, the others are written back as they were)
        *reinterpret_cast<uint2*>(alive + i0) = uint2{r.alive[0] & ~(f.w[0] * 0xffu), r.alive[1] & ~(f.w[1] * 0xffu)};
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const unsigned int sh = 8u * (unsigned int)(j & 3);
        if (sc_in(i0 + j, lim)) {
          const bool d = ((f.w[j >> 2] >> sh) & 1u) != 0u;
          if (d) alive[i0 + j] = 0;
          kill[i0 + j] = d ? 1 : 0;
        } else {
          f.w[j >> 2] &= ~(0xffu << sh);
        }
      }
    }
    return f;
  }
  static __device__ __forceinline__ unsigned long long at(const Keep& k, int j) {
    return (unsigned long long)((k.w[j >> 2] >> (8 * (j & 3))) & 1u);
  }
  // (counted, not added up value by value: the values would stay in registers from here to the emit)
  static __device__ __forceinline__ Sum sum(const Keep& k) { return (Sum)(__popc(k.w[0]) + __popc(k.w[1])); }
};
struct LoadFlagWords {  // (flags on a 16-byte boundary: an element is two 16-byte loads)
  static constexpr int E = 2, ROWS = 8, BATCH = 8;
  using Sum = unsigned int;
  const unsigned char* flags;
  unsigned int* bits;
  long long n_words;  // elements from here on count 0 (the scan's terminator: its prefix is the number of set bits)
  struct Raw {
    uint4 q[4];
  };
  struct Keep {  // the bitmap words
    unsigned int w[2];
  };
  __device__ __forceinline__ long long lim() const { return n_words; }
  __host__ __device__ __forceinline__ int mis() const { return 0; }
  __device__ __forceinline__ bool vec() const { return true; }
  __device__ __forceinline__ Raw raw_vec(long long i0) const {
    const uint4* p = reinterpret_cast<const uint4*>(flags + 32 * i0);
    return Raw{{p[0], p[1], p[2], p[3]}};
  }
  __device__ __forceinline__ Raw raw_elems(long long i0, long long lim) const {
    const uint4* p0 = reinterpret_cast<const uint4*>(flags + 32 * sc_clamp(i0, lim));
    const uint4* p1 = reinterpret_cast<const uint4*>(flags + 32 * sc_clamp(i0 + 1, lim));
    return Raw{{p0[0], p0[1], p1[0], p1[1]}};
  }
  template <bool FULL>
  __device__ __forceinline__ Keep keep(long long i0, long long lim, const Raw& r) const {
    auto nib = [](unsigned int x) { return (x & 1u) | ((x >> 7) & 2u) | ((x >> 14) & 4u) | ((x >> 21) & 8u); };
    Keep k;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const uint4 a = r.q[2 * j], b = r.q[2 * j + 1];
      const unsigned int w = nib(a.x) | (nib(a.y) << 4) | (nib(a.z) << 8) | (nib(a.w) << 12) | (nib(b.x) << 16) |
                             (nib(b.y) << 20) | (nib(b.z) << 24) | (nib(b.w) << 28);
      k.w[j] = (FULL || sc_in(i0 + j, lim)) ? w : 0u;
      if (FULL || sc_in(i0 + j, lim)) bits[i0 + j] = w;
    }
    return k;
  }
  static __device__ __forceinline__ unsigned long long at(const Keep& k, int j) { return (unsigned long long)__popc(k.w[j]); }
  static __device__ __forceinline__ Sum sum(const Keep& k) { return (Sum)(__popc(k.w[0]) + __popc(k.w[1])); }
};

struct LoadNone {  // no second array: never instantiated in the kernel, 0 tiles on the host
  static constexpr int E = 1, ROWS = 1, BATCH = 1;
  __host__ __device__ __forceinline__ int mis() const { return 0; }
};

template <class L>
struct ScTile {  // elements per workgroup
  static constexpr long long N = (long long)SC_THREADS * L::ROWS * L::E;
};

// the values of a wave's rows: lane group [wi0 + (64 r + lane) E, + E) of row r, 0 outside [0, min(n, lim))
template <class L>
__device__ __forceinline__ void load_rows(const L& ld, long long wi0, long long n, int lane, typename L::Keep* keep) {
  constexpr int E = L::E, ROWS = L::ROWS, BATCH = L::BATCH;
  const long long lim = n < ld.lim() ? n : ld.lim();
  if (lim <= 0 || wi0 >= lim) {  // (wave-uniform: nothing to load)
#pragma unroll
    for (int r = 0; r < ROWS; ++r) keep[r] = typename L::Keep{};
    return;
  }
  // (wave-uniform) the wave's span lies inside the array: vectors; the head and the tail: elements
  const bool full = ld.vec() && wi0 >= 0 && wi0 + 64ll * E * ROWS <= lim;
  // unconditional loads (element-wise ones from clamped indices: lanes past the end load the last element again): a
  // load under a branch of its own is waited for inside that branch
  if (full) {
#pragma unroll
    for (int b = 0; b < ROWS; b += BATCH) {
      typename L::Raw raw[BATCH];
#pragma unroll
      for (int r = 0; r < BATCH; ++r) raw[r] = ld.raw_vec(wi0 + (long long)((b + r) * 64 + lane) * E);
      asm volatile("" ::: "memory");  // (keeps the loads ahead of the first store of keep)
#pragma unroll
      for (int r = 0; r < BATCH; ++r)
        keep[b + r] = ld.template keep<true>(wi0 + (long long)((b + r) * 64 + lane) * E, lim, raw[r]);
      asm volatile("" ::: "memory");
    }
  } else {  // a row at a time (E loads in flight, each with an address of its own): the two waves of an array that hold
            // its head and its tail come here, and every wave of a loader that says !vec()
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      const long long i0 = wi0 + (long long)(r * 64 + lane) * E;
      const typename L::Raw raw = ld.raw_elems(i0, lim);
      asm volatile("" ::: "memory");
      keep[r] = ld.template keep<false>(i0, lim, raw);
      asm volatile("" ::: "memory");
    }
  }
}

// An emitter's loads (pre) are issued for all elements of a wave while the tile looks back; operator() stores (val: the
// value element i was scanned with).  EmitOut is the one the kernel stores for itself, a lane's E prefixes as vectors.
struct EmitOut {
  static constexpr bool OUT = true, WAVE = false;
  long long* out;
  struct Pre {};
  __device__ __forceinline__ Pre pre(long long) const { return Pre{}; }
  __device__ __forceinline__ void operator()(long long i, unsigned long long excl, const Pre&, unsigned long long) const {
    out[i] = (long long)excl;
  }
};
// edge classes -> directed edges (the scan of LoadPairWidth): class i writes its one or two edges at excl; total[0] =
// the number of directed edges (element n_pairs)
struct EmitEdges {
  static constexpr bool OUT = false, WAVE = false;
  const unsigned long long* pkey;
  const unsigned int* pcnt;
  const unsigned long long* pfirst;
  long long n_pairs;
  long long* total;
  int* e_src;
  int* e_tgt;
  signed char* e_sdir;
  signed char* e_tdir;
  unsigned int* e_cov;
  unsigned char* e_alive;
  struct Pre {
    unsigned long long key, first;
    unsigned int cnt;
  };
  __device__ __forceinline__ Pre pre(long long i) const {
    const long long j = i < n_pairs ? i : 0;  // (the terminator loads class 0: unused)
    return Pre{pkey[j], pfirst[j], pcnt[j]};
  }
  __device__ __forceinline__ void operator()(long long i, unsigned long long excl, const Pre& p, unsigned long long) const {
    if (i >= n_pairs) {
      total[0] = (long long)excl;
      return;
    }
    const unsigned long long key = p.key, first = p.first;
    const int lo = (int)((key >> 32) & 0x7fffffffull);
    const int hi = (int)((key & 0xffffffffull) - 1ull);
    const int X = (first & 1ull) ? lo : hi, Y = (first & 1ull) ? hi : lo;
    const signed char dX = (first & 2ull) ? 1 : -1, dY = (first & 4ull) ? 1 : -1;
    const long long e = (long long)excl;
    const unsigned int cnt = p.cnt;
    e_src[e] = X; e_tgt[e] = Y; e_sdir[e] = dX; e_tdir[e] = dY; e_alive[e] = 1;
    if (lo == hi) {  // E1 and E2 fall in the same class: one edge, +2 per traversal
      e_cov[e] = cnt * 2u;
    } else {
      e_cov[e] = cnt;
      e_src[e + 1] = Y; e_tgt[e + 1] = X; e_sdir[e + 1] = (signed char)-dY;
      e_tdir[e + 1] = (signed char)-dX; e_cov[e + 1] = cnt; e_alive[e + 1] = 1;
    }
  }
};
// live edges -> the dense list of their rows and ids (the scan of LoadByteSet over the edges' alive bytes): live edge i
// writes {its row, i} at its prefix, a dead edge nothing; total[0] = the number of live edges (element n_edges).  Nothing
// is written at or beyond total.  An edge's source is loaded only where the edge is alive: a few edges in a thousand
// survive the filter of a first graph, and loading the sources of all of them would be the pass over the edges this
// saves.  A load under a test of its own is waited for under that test, one round trip to memory each, so a wave does
// not test its elements one by one: every lane takes the live ones out of its own ROWS x 16, two a round, the loads of
// a round in flight together (a lane with nothing left loads edge 0); a wave has as many rounds as half its fullest
// lane holds.  A row with SC_LIVE_DENSE live edges and more loads the sources of all its edges instead, in one go.
#define SC_LIVE_DENSE 64
struct EmitLiveKeys {
  static constexpr bool OUT = false, WAVE = true;
  const int* e_src;
  const signed char* e_sdir;
  long long n_edges;
  long long* total;
  unsigned int* keys;
  unsigned int* edge_of;
  struct Pre {};
  __device__ __forceinline__ Pre pre(long long) const { return Pre{}; }
  template <int ROWS>
  static __device__ __forceinline__ unsigned int pick(const unsigned int* a, int r) {
    unsigned int x = a[0];
#pragma unroll
    for (int k = 1; k < ROWS; ++k) x = r == k ? a[k] : x;
    return x;
  }
  // the wave's elements [wi0, wi0 + 1024 ROWS): keep[r] holds the lane's 16 of row r as bytes of 0 or 1, base +
  // lane_excl[r] is the prefix of the first of them
  template <int ROWS>
  __device__ __forceinline__ void wave(long long wi0, int lane, unsigned long long base, const unsigned int* lane_excl,
                                       const LoadByteSet::Keep* keep) const {
    static_assert(ROWS <= 8, "the lane's elements are kept as two 64-bit masks");
    auto nib = [](unsigned int w) { return ((w * 0x01020408u) >> 24) & 0xfu; };  // bytes of 0 or 1 -> bits
    unsigned int m[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
      m[r] = nib(keep[r].w[0]) | (nib(keep[r].w[1]) << 4) | (nib(keep[r].w[2]) << 8) | (nib(keep[r].w[3]) << 12);
    // the terminator (elements from n_edges on count 0, so its prefix is the lane's up to it)
    const long long t = n_edges - wi0;
    if (t >= 0 && t < 1024ll * ROWS) {  // (wave-uniform)
      const int tr = (int)(t >> 10), tj = (int)t & 15;
      if (lane == ((int)(t >> 4) & 63))
        total[0] = (long long)(base + pick<ROWS>(lane_excl, tr) + __popc(pick<ROWS>(m, tr) & ((1u << tj) - 1u)));
    }
    unsigned long long q[2] = {0ull, 0ull};  // what is left to the rounds: bit 16 r + j
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      const unsigned int live = __builtin_amdgcn_readlane(lane_excl[r] + __popc(m[r]), 63) -
                                __builtin_amdgcn_readlane(lane_excl[r], 0);
      if (live < SC_LIVE_DENSE) {  // (wave-uniform)
        q[r >> 2] |= (unsigned long long)m[r] << (16 * (r & 3));
        continue;
      }
      const long long i0 = wi0 + (long long)(r * 64 + lane) * 16;
      int s[16];
      signed char d[16];
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        const long long i = sc_clamp(i0 + j, n_edges);
        s[j] = e_src[i];
        d[j] = e_sdir[i];
      }
      unsigned long long at = base + lane_excl[r];
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        if ((m[r] >> j) & 1u) {
          keys[at] = adj_row_of(s[j], d[j]);
          edge_of[at] = (unsigned int)(i0 + j);
          ++at;
        }
      }
    }
    while (__ballot((q[0] | q[1]) != 0ull)) {
      long long idx[2];
      unsigned long long at[2];
      bool ok[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const bool lo = q[0] != 0ull;
        const unsigned long long w = lo ? q[0] : q[1];
        ok[u] = w != 0ull;
        const int pos = ok[u] ? __ffsll((long long)w) - 1 + (lo ? 0 : 64) : 0;
        if (lo) q[0] &= q[0] - 1ull; else q[1] &= q[1] - 1ull;
        const int r = pos >> 4, j = pos & 15;
        idx[u] = wi0 + (long long)(r * 64 + lane) * 16 + j;
        at[u] = base + pick<ROWS>(lane_excl, r) + __popc(pick<ROWS>(m, r) & ((1u << j) - 1u));
      }
      int s[2];
      signed char d[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const long long i = ok[u] ? idx[u] : 0;
        s[u] = e_src[i];
        d[u] = e_sdir[i];
      }
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        if (ok[u]) {
          keys[at[u]] = adj_row_of(s[u], d[u]);
          edge_of[at[u]] = (unsigned int)idx[u];
        }
      }
    }
  }
};

// One tile of one array: tile `tile` of the launch, the (tile - seg0)-th of its array of n elements.
template <class L, class Emit>
__device__ __forceinline__ void scan_tile(const L& ld, const Emit& emit, long long n, long long tile, long long seg0,
                                          unsigned long long* status, unsigned int epoch, unsigned long long* s_wave,
                                          unsigned long long* s_excl) {
  constexpr int E = L::E, ROWS = L::ROWS;
  using Sum = typename L::Sum;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // the wave's first element; the first wave of an array whose base is not on a vector boundary begins before it
  const long long wi0 = (tile - seg0) * ScTile<L>::N + (long long)wave * (64 * E * ROWS) - ld.mis();
  // ---- the wave's elements as ROWS coalesced rows of 64 lane groups; a lane's group summed, inclusive scan of every
  // row's sums, rows chained
  typename L::Keep keep[ROWS];
  load_rows(ld, wi0, n, lane, keep);
  Sum lane_excl[ROWS];  // what the wave holds before the lane's group
  Sum row_off = 0;
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    const Sum s = L::sum(keep[r]);
    Sum v = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const Sum o = __shfl_up(v, d, 64);
      if (lane >= d) v += o;
    }
    lane_excl[r] = v - s + row_off;
    row_off += __shfl(v, 63, 64);
  }
  if (lane == 0) s_wave[wave] = (unsigned long long)row_off;  // the wave's sum
  __syncthreads();
  unsigned long long wave_excl = 0, tile_sum = 0;
#pragma unroll
  for (int w = 0; w < SC_THREADS / 64; ++w) {
    const unsigned long long s = s_wave[w];
    wave_excl += w < wave ? s : 0ull;
    tile_sum += s;
  }
  // the emitter's loads, in flight during the look-back
  typename Emit::Pre pre[ROWS][E];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
#pragma unroll
    for (int j = 0; j < E; ++j)
      pre[r][j] = emit.pre(sc_clamp(wi0 + (long long)(r * 64 + lane) * E + j, n));  // (unconditional, see load_rows)
  }
  // ---- look-back (first wave): sum of everything before this tile
  if (wave == 0) {
    unsigned long long excl = 0;
    if (tile == seg0) {
      if (lane == 0)
        __hip_atomic_store(status + tile, sc_word(2u, epoch, tile_sum), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
      if (lane == 0)
        __hip_atomic_store(status + tile, sc_word(1u, epoch, tile_sum), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      for (long long look = tile - 1;; look -= 64) {
        const long long idx = look - lane;
        unsigned int state = 2u;  // before the array's first tile: an inclusive prefix of 0
        unsigned long long val = 0;
        if (idx >= seg0) {
          unsigned long long w;
          do {  // the tile at idx has started (tickets are taken in order) and publishes without waiting for anybody
            w = __hip_atomic_load(status + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          } while ((unsigned int)((w >> 48) & 0x3fffu) != (epoch & 0x3fffu) || (w >> 62) == 0ull);
          state = (unsigned int)(w >> 62);
          val = w & SC_VAL_MASK;
        }
        const unsigned long long full = __ballot(state == 2u);
        // lanes up to the nearest inclusive prefix count; nothing further back does
        const int stop = full ? __ffsll((long long)full) - 1 : 63;
        unsigned long long part = lane <= stop ? val : 0ull;
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) part += __shfl_xor(part, d, 64);
        excl += part;
        if (full) break;
      }
      if (lane == 0)
        __hip_atomic_store(status + tile, sc_word(2u, epoch, excl + tile_sum), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (lane == 0) *s_excl = excl;
  }
  __syncthreads();
  // ---- every element its own prefix: the tile's, the wave's, the lane's, and the running sum inside the lane
  const unsigned long long base = *s_excl + wave_excl;
  if constexpr (Emit::WAVE) {  // (an emitter that knows the loader's Keep and takes the wave's elements as they are)
    emit.template wave<ROWS>(wi0, lane, base, lane_excl, keep);
  } else {
    // (wave-uniform: a lane's prefixes go out as 16-byte pairs where its group begins on a 16-byte boundary of out)
    bool pairs = false;
    if constexpr (Emit::OUT) pairs = (reinterpret_cast<uintptr_t>(emit.out + wi0) & 15u) == 0u;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      const long long i0 = wi0 + (long long)(r * 64 + lane) * E;
      unsigned long long p[E];
      unsigned long long run = base + (unsigned long long)lane_excl[r];
#pragma unroll
      for (int j = 0; j < E; ++j) {
        p[j] = run;
        run += L::at(keep[r], j);
      }
      bool done = false;
      if constexpr (Emit::OUT && E % 2 == 0) {
        if (pairs && i0 >= 0 && i0 + E <= n) {
#pragma unroll
          for (int j = 0; j < E; j += 2)
            *reinterpret_cast<ulonglong2*>(emit.out + i0 + j) = ulonglong2{p[j], p[j + 1]};
          done = true;
        }
      }
      if (!done) {
#pragma unroll
        for (int j = 0; j < E; ++j)
          if (sc_in(i0 + j, n)) emit(i0 + j, p[j], pre[r][j], L::at(keep[r], j));
      }
      __builtin_amdgcn_sched_barrier(0);  // (a row's E prefixes live at a time, not the wave's ROWS x E)
    }
  }
}

template <class Load, class LoadB, class Emit>
__global__ __launch_bounds__(SC_THREADS) void k_exscan(Load load, Emit emit_a, long long n_a, LoadB load_b,
                                                        long long* __restrict__ out_b, long long n_b, long long tiles_a,
                                                        unsigned long long* counter, unsigned long long ticket_base,
                                                        unsigned long long* status, unsigned int epoch, ClearArgs side) {
  __shared__ unsigned long long s_wave[SC_THREADS / 64];
  __shared__ unsigned long long s_excl;
  __shared__ unsigned int s_tile;
  if (threadIdx.x == 0) s_tile = (unsigned int)(atomicAdd(counter, 1ull) - ticket_base);
  __syncthreads();
  const long long tile = s_tile;
  // the second array's tiles (block-uniform; never taken with LoadNone: tiles_a is then the whole grid); its look-back
  // ends at its own first tile
  if constexpr (!std::is_same<LoadB, LoadNone>::value) {
    if (tile >= tiles_a)
      scan_tile(load_b, EmitOut{out_b}, n_b, tile, tiles_a, status, epoch, s_wave, &s_excl);
    else
      scan_tile(load, emit_a, n_a, tile, 0, status, epoch, s_wave, &s_excl);
  } else {
    scan_tile(load, emit_a, n_a, tile, 0, status, epoch, s_wave, &s_excl);
  }
  if (side.n) clear_args_part(side, blockIdx.x, gridDim.x);
}

// tiles of an array of n elements: the lane groups lie on the array's aligned grid, so the tiles cover n + mis positions
template <class L>
static unsigned long long scan_tiles(const L& ld, size_t n) {
  return n ? ((unsigned long long)n + (unsigned long long)ld.mis() + ScTile<L>::N - 1) / ScTile<L>::N : 0ull;
}

// side: ranges zeroed by the scan's workgroups (nothing the scan reads or writes; zeroed by clear_many when there is
// nothing to scan)
template <class Load, class Emit, class LoadB = LoadNone>
static int exscan_emit(amg_ctx* c, Load load, Emit emit, size_t n, LoadB load_b = LoadNone{}, long long* out_b = nullptr,
                       size_t n_b = 0, const ClearList* side = nullptr) {
  if (side && side->overflow) return amg_fail(AMG_E_ARG, "exscan: more than %d ranges in one list", CLEAR_MAX);
  if (n == 0 && n_b == 0) return side ? clear_many(c, *side) : AMG_OK;
  const unsigned long long tiles_a = scan_tiles(load, n);
  const unsigned long long tiles = tiles_a + scan_tiles(load_b, n_b);
  // [0] the ticket counter, [8 ...] one status word per tile
  const size_t need = (size_t)(tiles + 8) * sizeof(unsigned long long);
  if (need > c->scan_state.cap || c->scan_epoch >= 0x3fffu) {
    if (need > c->scan_state.cap) {
      AMGCHK(c->scan_state.ensure(need * 2));
      c->scan_tickets = 0;
      HIPCHK(hipMemsetAsync(c->scan_state.p, 0, c->scan_state.cap, c->stream));
    } else {  // the epoch wraps: forget every old status word (the ticket counter keeps counting)
      HIPCHK(hipMemsetAsync(c->scan_state.as<unsigned long long>() + 8, 0,
                            c->scan_state.cap - 8 * sizeof(unsigned long long), c->stream));
    }
    c->scan_epoch = 0;
  }
  const unsigned int epoch = ++c->scan_epoch;
  unsigned long long* st = c->scan_state.as<unsigned long long>();
  ClearArgs sa;
  sa.n = 0;
  if (side) sa = clear_args(*side);
  hipLaunchKernelGGL((k_exscan<Load, LoadB, Emit>), dim3((unsigned int)tiles), dim3(SC_THREADS), 0, c->stream, load, emit,
                     (long long)n, load_b, out_b, (long long)n_b, (long long)tiles_a, st, c->scan_tickets, st + 8, epoch, sa);
  c->scan_tickets += tiles;
  return AMG_OK;
}

template <class Load, class LoadB = LoadNone>
static int exscan(amg_ctx* c, Load load, long long* out, size_t n, LoadB load_b = LoadNone{}, long long* out_b = nullptr,
                  size_t n_b = 0) {
  return exscan_emit(c, load, EmitOut{out}, n, load_b, out_b, n_b);
}

int prim_exscan_u32_to_i64(amg_ctx* c, const unsigned int* in, long long* out, size_t n) {
  return exscan(c, LoadArr<unsigned int>{in}, out, n);
}

int prim_exscan_i64(amg_ctx* c, const long long* in, long long* out, size_t n) {
  return exscan(c, LoadArr<long long>{in}, out, n);
}

// two independent scans of n + 1 elements each (in[n] counts 0: out[n] = the sum), one launch
int prim_exscan_u32_pair(amg_ctx* c, const unsigned int* in_a, long long* out_a, const unsigned int* in_b, long long* out_b,
                         size_t n) {
  return exscan(c, LoadArrN<unsigned int>{in_a, (long long)n}, out_a, n + 1, LoadArrN<unsigned int>{in_b, (long long)n}, out_b,
                n + 1);
}

int prim_exscan_i64_pair(amg_ctx* c, const long long* in_a, long long* out_a, const long long* in_b, long long* out_b,
                         size_t n) {
  return exscan(c, LoadArrN<long long>{in_a, (long long)n}, out_a, n + 1, LoadArrN<long long>{in_b, (long long)n}, out_b,
                n + 1);
}

// out[i] = set bytes before byte i for i <= n; side: ranges zeroed on the way
int prim_exscan_bytes_set(amg_ctx* c, const unsigned char* in, long long* out, size_t n, const ClearList* side) {
  return exscan_emit(c, LoadByteSet{in, (long long)n}, EmitOut{out}, n + 1, LoadNone{}, nullptr, 0, side);
}

// alive[i] = 0 and kill[i] = 1 where kill[i] was set on a live node (kill[i] = 0 elsewhere); out[i] = nodes removed
// before node i for i <= n
int prim_exscan_apply_kill(amg_ctx* c, unsigned char* kill, unsigned char* alive, long long* out, size_t n) {
  return exscan(c, LoadApplyKill{kill, alive, (long long)n}, out, n + 1);
}

// out_keep = exscan(len[i] != 0), out_off = exscan(len[i]) over n + 1 elements, one launch
int prim_exscan_keep_and_len(amg_ctx* c, const unsigned int* len, long long* out_keep, long long* out_off, size_t n) {
  return exscan(c, LoadNonzero{len, (long long)n}, out_keep, n + 1, LoadArrN<unsigned int>{len, (long long)n}, out_off, n + 1);
}

// flags[32 n_words] -> bits[n_words]; out[i] = set bits before word i for i <= n_words (out[n_words] = number of set bits)
int prim_exscan_flag_words(amg_ctx* c, const unsigned char* flags, unsigned int* bits, long long* out, size_t n_words) {
  return exscan(c, LoadFlagWords{flags, bits, (long long)n_words}, out, n_words + 1);
}

int prim_exscan_bits_popc(amg_ctx* c, const unsigned int* bits, long long* out, size_t n_words) {
  return exscan(c, LoadBitsPopc{bits, (long long)n_words}, out, n_words + 1);
}

// out[i] = first directed edge of edge class i, out[n_pairs] = number of directed edges
int prim_exscan_pair_width(amg_ctx* c, const unsigned long long* pkey, long long* out, size_t n_pairs) {
  return exscan(c, LoadPairWidth<2>{pkey, (long long)n_pairs}, out, n_pairs + 1);
}

// edge classes -> directed edges in one launch: class i's edges go to the exclusive prefix of the classes' widths (one
// for a self-loop, two otherwise), *total = the number of directed edges; side: ranges zeroed on the way
int prim_exscan_emit_edges(amg_ctx* c, const unsigned long long* pkey, const unsigned int* pcnt,
                           const unsigned long long* pfirst, size_t n_pairs, long long* total, int* e_src, int* e_tgt,
                           signed char* e_sdir, signed char* e_tdir, unsigned int* e_cov, unsigned char* e_alive,
                           const ClearList* side) {
  return exscan_emit(c, LoadPairWidth<1>{pkey, (long long)n_pairs},
                     EmitEdges{pkey, pcnt, pfirst, (long long)n_pairs, total, e_src, e_tgt, e_sdir, e_tdir, e_cov, e_alive},
                     n_pairs + 1, LoadNone{}, nullptr, 0, side);
}

// live edges -> {row, edge id} pairs in edge order at keys / edge_of, *total = their number; side: ranges zeroed on the way
int prim_exscan_live_edges(amg_ctx* c, const unsigned char* e_alive, const int* e_src, const signed char* e_sdir, size_t n_edges,
                           long long* total, unsigned int* keys, unsigned int* edge_of, const ClearList* side) {
  return exscan_emit(c, LoadByteSet{e_alive, (long long)n_edges},
                     EmitLiveKeys{e_src, e_sdir, (long long)n_edges, total, keys, edge_of}, n_edges + 1, LoadNone{}, nullptr, 0,
                     side);
}

// ------------------------------------------------------------------ amg_scan_probe (tests: one scan on host arrays)
// kind & 0xff: what is scanned (below); (kind >> 8) & 0xff: the elements by which the scanned array is laid past a
// 256-byte boundary on the device (kind 3: both byte arrays, kind 6: the alive bytes, kind 7: the first array, the second
// by (kind >> 16) & 0xff), so that the head, the body and the tail of an array that is no allocation of its own can be
// met.  0xff fills every byte of aux before the scan.
extern "C" int amg_scan_probe(amg_ctx* c, int kind, const void* in, int64_t n, int64_t* out, void* aux) {
  if (!c || kind < 0 || n < 0 || (n > 0 && !in) || !out) return amg_fail(AMG_E_ARG, "scan_probe: bad arguments");
  const size_t mis = (size_t)((kind >> 8) & 0xff), mis_b = (size_t)((kind >> 16) & 0xff);
  if ((kind >> 24) || (mis_b && (kind & 0xff) != 7)) return amg_fail(AMG_E_ARG, "scan_probe: bad misalignment bits");
  kind &= 0xff;
  size_t in_bytes = 0, out_words = (size_t)n + 1, aux_bytes = 0, elem = 1;
  switch (kind) {
    case 0: in_bytes = (size_t)n; aux_bytes = (size_t)n; break;                  // bytes set; aux: a side-cleared range
    case 1: in_bytes = 8 * (size_t)n; elem = 8; break;                             // pair widths
    case 2: in_bytes = 32 * (size_t)n; aux_bytes = 4 * (size_t)n; elem = 32; break;  // flag words; aux: the bitmap words
    case 3: in_bytes = 2 * (size_t)n; aux_bytes = 2 * (size_t)n; break;            // apply kill; aux: kill, alive after
    case 4: in_bytes = 4 * (size_t)n; out_words = 2 * ((size_t)n + 1); elem = 4; break;  // keep (len != 0) and len
    case 5: in_bytes = 20 * (size_t)n; out_words = 1; aux_bytes = 30 * (size_t)n; elem = 8; break;  // edges of classes
    case 6: in_bytes = 6 * (size_t)n; out_words = 1; aux_bytes = 8 * (size_t)n; break;     // live edges: src, alive, sdir
    case 7: in_bytes = 8 * (size_t)n; out_words = 2 * ((size_t)n + 1); elem = 4; break;  // two arrays of n words each
    default: return amg_fail(AMG_E_ARG, "scan_probe: unknown kind %d", kind);
  }
  const size_t shift = mis * elem;  // bytes
  if (shift > 256 || mis_b * elem > 256) return amg_fail(AMG_E_ARG, "scan_probe: misalignment of %zu bytes (256 at most)", shift);
  char* d = nullptr;
  const size_t in_cap = ((in_bytes + 255) & ~(size_t)255) + 768, out_cap = (out_words * 8 + 255) & ~(size_t)255;
  const size_t aux_cap = ((aux_bytes + 256) & ~(size_t)255) + 256;
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&d), in_cap + out_cap + aux_cap));
  // kind 3 scans a copy in aux, kind 6 shifts the alive bytes alone (the sources stay whole words)
  char* din = d + (kind == 3 || kind == 6 ? 0 : shift);
  long long* dout = reinterpret_cast<long long*>(d + in_cap);
  char* daux = d + in_cap + out_cap + (kind == 3 ? shift : 0);
  char* dalive = d + ((4 * (size_t)n + 255) & ~(size_t)255) + shift;  // kind 6: alive, sdir behind it
  char* dsecond = d + ((shift + 4 * (size_t)n + 255) & ~(size_t)255) + mis_b * elem;  // kind 7: the second array
  int rc = AMG_OK;
  do {
    if (kind == 6 && n) {
      const char* h = static_cast<const char*>(in);
      if (hipMemcpy(din, h, 4 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
          hipMemcpy(dalive, h + 4 * (size_t)n, 2 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess) {
        rc = amg_fail(AMG_E_HIP, "h2d");
        break;
      }
    } else if (kind == 7 && n) {
      const char* h = static_cast<const char*>(in);
      if (hipMemcpy(din, h, 4 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
          hipMemcpy(dsecond, h + 4 * (size_t)n, 4 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess) {
        rc = amg_fail(AMG_E_HIP, "h2d");
        break;
      }
    } else if (in_bytes && hipMemcpy(din, in, in_bytes, hipMemcpyHostToDevice) != hipSuccess) {
      rc = amg_fail(AMG_E_HIP, "h2d");
      break;
    }
    if (hipMemset(d + in_cap + out_cap, 0xff, aux_cap) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
      rc = amg_fail(AMG_E_HIP, "memset");
      break;
    }
    switch (kind) {
      case 0: {
        ClearList side;
        side.add(daux, (size_t)n);
        rc = prim_exscan_bytes_set(c, reinterpret_cast<unsigned char*>(din), dout, (size_t)n, &side);
        break;
      }
      case 1: rc = prim_exscan_pair_width(c, reinterpret_cast<unsigned long long*>(din), dout, (size_t)n); break;
      case 2:
        rc = prim_exscan_flag_words(c, reinterpret_cast<unsigned char*>(din), reinterpret_cast<unsigned int*>(daux), dout,
                                    (size_t)n);
        break;
      case 3:
        if (n && (hipMemcpy(daux, din, 2 * (size_t)n, hipMemcpyDeviceToDevice) != hipSuccess ||
                  hipDeviceSynchronize() != hipSuccess)) {
          rc = amg_fail(AMG_E_HIP, "d2d");
          break;
        }
        rc = prim_exscan_apply_kill(c, reinterpret_cast<unsigned char*>(daux), reinterpret_cast<unsigned char*>(daux) + n,
                                    dout, (size_t)n);
        break;
      case 4:
        rc = prim_exscan_keep_and_len(c, reinterpret_cast<unsigned int*>(din), dout, dout + n + 1, (size_t)n);
        break;
      case 5: {
        const size_t E = 2 * (size_t)n;
        int* src = reinterpret_cast<int*>(daux);
        int* tgt = src + E;
        unsigned int* cov = reinterpret_cast<unsigned int*>(tgt + E);
        signed char* sdir = reinterpret_cast<signed char*>(cov + E);
        signed char* tdir = sdir + E;
        unsigned char* alive = reinterpret_cast<unsigned char*>(tdir + E);
        rc = prim_exscan_emit_edges(c, reinterpret_cast<unsigned long long*>(din),
                                    reinterpret_cast<unsigned int*>(din + 16 * (size_t)n),
                                    reinterpret_cast<unsigned long long*>(din + 8 * (size_t)n), (size_t)n, dout, src, tgt,
                                    sdir, tdir, cov, alive, nullptr);
        break;
      }
      case 6: {
        unsigned int* keys = reinterpret_cast<unsigned int*>(daux);
        rc = prim_exscan_live_edges(c, reinterpret_cast<unsigned char*>(dalive), reinterpret_cast<int*>(din),
                                    reinterpret_cast<signed char*>(dalive + (size_t)n), (size_t)n, dout, keys, keys + n,
                                    nullptr);
        break;
      }
      case 7:
        rc = prim_exscan_u32_pair(c, reinterpret_cast<unsigned int*>(din), dout, reinterpret_cast<unsigned int*>(dsecond),
                                  dout + n + 1, (size_t)n);
        break;
    }
    if (rc != AMG_OK) break;
    if (hipStreamSynchronize(c->stream) != hipSuccess) { rc = amg_fail(AMG_E_HIP, "scan_probe: stream"); break; }
    if (hipMemcpy(out, dout, out_words * 8, hipMemcpyDeviceToHost) != hipSuccess) { rc = amg_fail(AMG_E_HIP, "d2h"); break; }
    if (aux && aux_bytes && hipMemcpy(aux, daux, aux_bytes, hipMemcpyDeviceToHost) != hipSuccess) { rc = amg_fail(AMG_E_HIP, "d2h"); break; }
  } while (false);
  (void)hipFree(d);
  return rc;
}
