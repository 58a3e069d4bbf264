// amg_scan.hip — exclusive prefix sums in ONE launch (decoupled look-back, hand-written for wave64).
//
// The passes scan short arrays all the time (flags -> positions, counts -> offsets: ~25 scans per cleaning
// sweep over 0.5 - 6 M elements).  A library scan is two launches (state initialisation + scan) through a
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
#include "amg_rows.h"

#define SC_THREADS 512                  // 8 waves per workgroup
#define SC_ROWS 16                       // rows of 64 per wave: a wave scans 1024 consecutive elements
#define SC_TILE (SC_THREADS * SC_ROWS)   // 8192 elements per workgroup
// What a scan costs beyond ~8 us grows with its number of tiles rather than its bytes (measured with 4 096-element
// tiles: ~30 ns per tile, 100 us for 12.5 M bytes): every tile takes a ticket from one counter word and looks back over
// the tiles still in flight, 64 per round trip to the status words.  Larger tiles make both shorter; 16 waves a tile
// would spill (128 registers per lane at most).
#define SC_VAL_MASK ((1ull << 48) - 1ull)

__device__ __forceinline__ unsigned long long sc_word(unsigned int state, unsigned int epoch, unsigned long long v) {
  return ((unsigned long long)state << 62) | ((unsigned long long)(epoch & 0x3fffu) << 48) | (v & SC_VAL_MASK);
}

// What is scanned is what a LOADER makes of element i — an array entry, or something computed on the way that would
// otherwise be a kernel of its own writing an array only the scan reads (the passes launch ~200 kernels per cleaning
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
// array, the tiles behind them the second, whose look-back stops at its own first tile).
// A loader is used in two steps, so that the 16 loads of a wave's rows are all in flight before the first is waited
// for: raw(i) only loads (i < lim), val(i, raw) makes the scanned value of it and does any store the loader has (a
// store between two rows' loads, or a value computed inside a bounds check, made every row wait for the one before).
#define SC_NO_LIM 0x7fffffffffffffffll
template <class T>
struct LoadArr {
  const T* in;
  using Raw = T;
  __device__ __forceinline__ long long lim() const { return SC_NO_LIM; }
  __device__ __forceinline__ Raw raw(long long i) const { return in[i]; }
  __device__ __forceinline__ unsigned long long val(long long, Raw r) const { return (unsigned long long)r; }
};
template <class T>
struct LoadArrN {  // in[i] for i < n, 0 from there on (the scan's terminator: no cleared element behind the array)
  const T* in;
  long long n;
  using Raw = T;
  __device__ __forceinline__ long long lim() const { return n; }
  __device__ __forceinline__ Raw raw(long long i) const { return in[i]; }
  __device__ __forceinline__ unsigned long long val(long long, Raw r) const { return (unsigned long long)r; }
};
struct LoadNonzero {  // 1 where in[i] != 0, i < n
  const unsigned int* in;
  long long n;
  using Raw = unsigned int;
  __device__ __forceinline__ long long lim() const { return n; }
  __device__ __forceinline__ Raw raw(long long i) const { return in[i]; }
  __device__ __forceinline__ unsigned long long val(long long, Raw r) const { return r != 0u ? 1ull : 0ull; }
};
struct LoadByteSet {  // 1 where byte i is set, i < n
  const unsigned char* in;
  long long n;
  using Raw = unsigned char;
  __device__ __forceinline__ long long lim() const { return n; }
  __device__ __forceinline__ Raw raw(long long i) const { return in[i]; }
  __device__ __forceinline__ unsigned long long val(long long, Raw r) const { return r != 0 ? 1ull : 0ull; }
};
struct LoadApplyKill {  // node removal: a marked live node dies; kill[i] is left as "removed now" and counted
  unsigned char* kill;
  unsigned char* alive;
  long long n;
  struct Raw {  // (a word each: two bytes packed into one register are waited for at once)
    unsigned int kill, alive;
  };
  __device__ __forceinline__ long long lim() const { return n; }
  __device__ __forceinline__ Raw raw(long long i) const { return Raw{kill[i], alive[i]}; }
  __device__ __forceinline__ unsigned long long val(long long i, Raw r) const {
    const bool f = r.kill != 0u && r.alive != 0u;
    if (f) alive[i] = 0;
    kill[i] = f ? 1 : 0;
    return f ? 1ull : 0ull;
  }
};
struct LoadFlagWords {
  const unsigned char* flags;
  unsigned int* bits;
  long long n_words;  // elements from here on count 0 (the scan's terminator: its prefix is the number of set bits)
  struct Raw {
    uint4 a, b;
  };
  __device__ __forceinline__ long long lim() const { return n_words; }
  __device__ __forceinline__ Raw raw(long long i) const {
    const uint4* p = reinterpret_cast<const uint4*>(flags + 32 * i);
    return Raw{p[0], p[1]};
  }
  __device__ __forceinline__ unsigned long long val(long long i, const Raw& r) const {
    auto nib = [](unsigned int x) { return (x & 1u) | ((x >> 7) & 2u) | ((x >> 14) & 4u) | ((x >> 21) & 8u); };
    const uint4 a = r.a, b = r.b;
    const unsigned int w = nib(a.x) | (nib(a.y) << 4) | (nib(a.z) << 8) | (nib(a.w) << 12) | (nib(b.x) << 16) |
                           (nib(b.y) << 20) | (nib(b.z) << 24) | (nib(b.w) << 28);
    bits[i] = w;
    return (unsigned long long)__popc(w);
  }
};
struct LoadBitsPopc {
  const unsigned int* bits;
  long long n_words;
  using Raw = unsigned int;
  __device__ __forceinline__ long long lim() const { return n_words; }
  __device__ __forceinline__ Raw raw(long long i) const { return bits[i]; }
  __device__ __forceinline__ unsigned long long val(long long, Raw r) const { return (unsigned long long)__popc(r); }
};
struct LoadPairWidth {
  const unsigned long long* pkey;
  long long n_pairs;  // elements from here on count 0 (the scan's terminator)
  using Raw = unsigned long long;
  __device__ __forceinline__ long long lim() const { return n_pairs; }
  __device__ __forceinline__ Raw raw(long long i) const { return pkey[i]; }
  __device__ __forceinline__ unsigned long long val(long long, Raw key) const {
    const unsigned int lo = (unsigned int)((key >> 32) & 0x7fffffffull);
    const unsigned int hi = (unsigned int)(key & 0xffffffffull) - 1u;
    return lo == hi ? 1ull : 2ull;
  }
};

struct LoadNone {
  using Raw = unsigned char;
  __device__ __forceinline__ long long lim() const { return 0; }
  __device__ __forceinline__ Raw raw(long long) const { return 0; }
  __device__ __forceinline__ unsigned long long val(long long, Raw) const { return 0ull; }
};

// the values of a wave's rows: element w0 + 64 r + lane of row r, 0 from min(n, lim) on
template <class L>
__device__ __forceinline__ void load_rows(const L& ld, long long w0, long long n, int lane, unsigned long long* x) {
  const long long lim = n < ld.lim() ? n : ld.lim();
  if (w0 >= lim) {  // (wave-uniform: nothing to load)
#pragma unroll
    for (int r = 0; r < SC_ROWS; ++r) x[r] = 0ull;
    return;
  }
  // unconditional loads (lanes past the end load the last element again): a load under a branch of its own is
  // waited for inside that branch
  typename L::Raw raw[SC_ROWS];
#pragma unroll
  for (int r = 0; r < SC_ROWS; ++r) {
    const long long i = w0 + r * 64 + lane;
    raw[r] = ld.raw(i < lim ? i : lim - 1);
  }
  asm volatile("" ::: "memory");  // (keeps the loads ahead of the first store of val)
#pragma unroll
  for (int r = 0; r < SC_ROWS; ++r) {
    const long long i = w0 + r * 64 + lane;
    x[r] = i < lim ? ld.val(i, raw[r]) : 0ull;
  }
}

// An emitter's loads (pre) are issued for all rows of a wave while the tile looks back; operator() stores (val: the
// value element i was scanned with).
struct EmitOut {
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
// writes {its row, i} at excl, a dead edge nothing; total[0] = the number of live edges (element n_edges).  Nothing is
// written at or beyond total.  An edge's source is loaded under the alive test: a few edges in a thousand survive the
// filter of a first graph, and loading the sources of all of them would be the pass over the edges this saves.
struct EmitLiveKeys {
  const int* e_src;
  const signed char* e_sdir;
  long long n_edges;
  long long* total;
  unsigned int* keys;
  unsigned int* edge_of;
  struct Pre {};
  __device__ __forceinline__ Pre pre(long long) const { return Pre{}; }
  __device__ __forceinline__ void operator()(long long i, unsigned long long excl, const Pre&, unsigned long long val) const {
    if (i >= n_edges) {
      total[0] = (long long)excl;
      return;
    }
    if (val == 0ull) return;
    keys[excl] = adj_row_of(e_src[i], e_sdir[i]);
    edge_of[excl] = (unsigned int)i;
  }
};
template <class Load, class LoadB, class Emit>
__global__ __launch_bounds__(SC_THREADS) void k_exscan(Load load, Emit emit_a, long long n_a, LoadB load_b,
                                                        long long* __restrict__ out_b, long long n_b, long long tiles_a,
                                                        unsigned long long* counter, unsigned long long ticket_base,
                                                        unsigned long long* status, unsigned int epoch, ClearArgs side) {
  __shared__ unsigned long long s_wave[SC_THREADS / 64];
  __shared__ unsigned long long s_excl;
  __shared__ unsigned int s_tile;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) s_tile = (unsigned int)(atomicAdd(counter, 1ull) - ticket_base);
  __syncthreads();
  const long long tile = s_tile;
  // the second array's tiles (block-uniform; never taken with LoadNone: tiles_a is then the whole grid)
  const bool second = tile >= tiles_a;
  const long long seg0 = second ? tiles_a : 0;  // first tile of this tile's array: where its look-back ends
  const long long n = second ? n_b : n_a;
  const long long w0 = (tile - seg0) * SC_TILE + (long long)wave * (64 * SC_ROWS);
  // ---- the wave's 1024 elements as 16 coalesced rows; inclusive scan of every row, rows chained
  unsigned long long x[SC_ROWS], inc[SC_ROWS];
  if (second)
    load_rows(load_b, w0, n, lane, x);
  else
    load_rows(load, w0, n, lane, x);
  unsigned long long row_off = 0;
#pragma unroll
  for (int r = 0; r < SC_ROWS; ++r) {
    unsigned long long v = x[r];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned long long o = __shfl_up(v, d, 64);
      if (lane >= d) v += o;
    }
    inc[r] = v + row_off;
    row_off += __shfl(v, 63, 64);
  }
  if (lane == 0) s_wave[wave] = row_off;  // the wave's sum
  __syncthreads();
  unsigned long long wave_excl = 0, tile_sum = 0;
#pragma unroll
  for (int w = 0; w < SC_THREADS / 64; ++w) {
    const unsigned long long s = s_wave[w];
    wave_excl += w < wave ? s : 0ull;
    tile_sum += s;
  }
  // the emitter's loads, in flight during the look-back
  typename Emit::Pre pre[SC_ROWS];
  if (!second) {
#pragma unroll
    for (int r = 0; r < SC_ROWS; ++r) {
      const long long i = w0 + r * 64 + lane;
      pre[r] = emit_a.pre(i < n ? i : n - 1);  // (unconditional, see load_rows)
    }
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
    if (lane == 0) s_excl = excl;
  }
  __syncthreads();
  const unsigned long long base = s_excl + wave_excl;
#pragma unroll
  for (int r = 0; r < SC_ROWS; ++r) {
    const long long i = w0 + r * 64 + lane;
    if (i < n) {
      if (second)
        out_b[i] = (long long)(base + inc[r] - x[r]);
      else
        emit_a(i, base + inc[r] - x[r], pre[r], x[r]);
    }
  }
  if (side.n) clear_args_part(side, blockIdx.x, gridDim.x);
}

// side: ranges zeroed by the scan's workgroups (nothing the scan reads or writes; zeroed by clear_many when there is
// nothing to scan)
template <class Load, class Emit, class LoadB = LoadNone>
static int exscan_emit(amg_ctx* c, Load load, Emit emit, size_t n, LoadB load_b = LoadNone{}, long long* out_b = nullptr,
                       size_t n_b = 0, const ClearList* side = nullptr) {
  if (side && side->overflow) return amg_fail(AMG_E_ARG, "exscan: more than %d ranges in one list", CLEAR_MAX);
  if (n == 0 && n_b == 0) return side ? clear_many(c, *side) : AMG_OK;
  const unsigned long long tiles_a = (n + SC_TILE - 1) / SC_TILE;
  const unsigned long long tiles = tiles_a + (n_b + SC_TILE - 1) / SC_TILE;
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
  return exscan(c, LoadPairWidth{pkey, (long long)n_pairs}, out, n_pairs + 1);
}

// edge classes -> directed edges in one launch: class i's edges go to the exclusive prefix of the classes' widths (one
// for a self-loop, two otherwise), *total = the number of directed edges; side: ranges zeroed on the way
int prim_exscan_emit_edges(amg_ctx* c, const unsigned long long* pkey, const unsigned int* pcnt,
                           const unsigned long long* pfirst, size_t n_pairs, long long* total, int* e_src, int* e_tgt,
                           signed char* e_sdir, signed char* e_tdir, unsigned int* e_cov, unsigned char* e_alive,
                           const ClearList* side) {
  return exscan_emit(c, LoadPairWidth{pkey, (long long)n_pairs},
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
extern "C" int amg_scan_probe(amg_ctx* c, int kind, const void* in, int64_t n, int64_t* out, void* aux) {
  if (!c || n < 0 || (n > 0 && !in) || !out) return amg_fail(AMG_E_ARG, "scan_probe: bad arguments");
  size_t in_bytes = 0, out_words = (size_t)n + 1, aux_bytes = 0;
  switch (kind) {
    case 0: in_bytes = (size_t)n; aux_bytes = (size_t)n; break;                  // bytes set; aux: a side-cleared range
    case 1: in_bytes = 8 * (size_t)n; break;                                       // pair widths
    case 2: in_bytes = 32 * (size_t)n; aux_bytes = 4 * (size_t)n; break;           // flag words; aux: the bitmap words
    case 3: in_bytes = 2 * (size_t)n; aux_bytes = 2 * (size_t)n; break;            // apply kill; aux: kill, alive after
    case 4: in_bytes = 4 * (size_t)n; out_words = 2 * ((size_t)n + 1); break;      // keep (len != 0) and len
    case 5: in_bytes = 20 * (size_t)n; out_words = 1; aux_bytes = 30 * (size_t)n; break;  // edges of classes
    case 6: in_bytes = 6 * (size_t)n; out_words = 1; aux_bytes = 8 * (size_t)n; break;     // live edges: src, alive, sdir
    default: return amg_fail(AMG_E_ARG, "scan_probe: unknown kind %d", kind);
  }
  char* d = nullptr;
  const size_t in_cap = (in_bytes + 255) & ~(size_t)255, out_cap = (out_words * 8 + 255) & ~(size_t)255;
  const size_t aux_cap = (aux_bytes + 256) & ~(size_t)255;
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&d), in_cap + out_cap + aux_cap));
  char* din = d;
  long long* dout = reinterpret_cast<long long*>(d + in_cap);
  char* daux = d + in_cap + out_cap;
  int rc = AMG_OK;
  do {
    if (in_bytes && hipMemcpy(din, in, in_bytes, hipMemcpyHostToDevice) != hipSuccess) { rc = amg_fail(AMG_E_HIP, "h2d"); break; }
    if (hipMemset(daux, 0xff, aux_cap) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
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
        rc = prim_exscan_live_edges(c, reinterpret_cast<unsigned char*>(din + 4 * (size_t)n), reinterpret_cast<int*>(din),
                                    reinterpret_cast<signed char*>(din + 5 * (size_t)n), (size_t)n, dout, keys, keys + n,
                                    nullptr);
        break;
      }
    }
    if (rc != AMG_OK) break;
    if (hipStreamSynchronize(c->stream) != hipSuccess) { rc = amg_fail(AMG_E_HIP, "scan_probe: stream"); break; }
    if (hipMemcpy(out, dout, out_words * 8, hipMemcpyDeviceToHost) != hipSuccess) { rc = amg_fail(AMG_E_HIP, "d2h"); break; }
    if (aux && aux_bytes && hipMemcpy(aux, daux, aux_bytes, hipMemcpyDeviceToHost) != hipSuccess) { rc = amg_fail(AMG_E_HIP, "d2h"); break; }
  } while (false);
  (void)hipFree(d);
  return rc;
}
