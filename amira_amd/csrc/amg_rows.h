// amg_rows.h — adjacency rows on the device: which row an edge belongs to, a row's edge ids put in ascending order
// (= list order of the reference: edge ids follow insertion order), and how a walker reads a row.  Two units make rows
// with the ordering back end below: amg_adjacency.hip the full lists of the graph as built, amg_live_rows.hip the lists
// of the live edges (and tip clipping's row summary).
#pragma once
#include "amg_device.h"

// row 2n = forward list of node n, row 2n + 1 = its backward list
__device__ __forceinline__ unsigned int adj_row_of(int src, int sdir) { return 2u * (unsigned int)src + (sdir > 0 ? 0u : 1u); }

// ------------------------------------------------------------------ a row's ids in ascending order
// The ids of a row lie at ids[off .. off + cnt) in any order.  Rows of 1 and 2 ids are placed inline, rows of
// 3 .. WAVE_ROW_MAX by the wave, longer ones are listed and left to a second kernel: a workgroup per row up to HUGE_ROW,
// the first HUB_BLOCKS workgroups for the rows beyond.  emit(row, off, cnt, rank, id) places one id, whichever tier
// ranked it.
#define WAVE_ROW_MAX 64
#define HUGE_ROW 1024
#define HUB_BLOCKS 8  // workgroups that take the rows beyond HUGE_ROW: each owns one bitmap of the caller's hub_bits

// Rows of 3 .. 64 edge ids in ascending order by the WAVE, one row at a time: every lane that holds such a row (`mine`)
// is served in turn — lane j takes the row's j-th id, its rank is the number of smaller ids (one shuffle per id of the
// row), emit(row, row's offset, row's length, rank, id) places it (rank: any integer type).  A thread per row with an
// insertion sort in a private array was the tail of the list kernels: a row of thirty ids is ~500 dependent scratch
// accesses of ONE lane (0.9 ms for the genome rows of a graph that carries the residual error nodes of eight read
// sets), here ~30 shuffles of a wave.
// Every lane of the wave must call (no early returns before).
template <class Emit>
__device__ __forceinline__ void wave_rows_in_order(bool mine, unsigned int row, long long off, int cnt,
                                                   const unsigned int* __restrict__ ids, Emit emit) {
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(mine);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    todo &= todo - 1ull;
    const long long o = __shfl(off, leader, 64);
    const int n = __shfl(cnt, leader, 64);
    const unsigned int rw = __shfl(row, leader, 64);
    const unsigned int x = lane < n ? ids[o + lane] : 0xffffffffu;
    int rank = 0;
    for (int q = 0; q < n; ++q) rank += __shfl(x, q, 64) < x ? 1 : 0;
    if (lane < n) emit(rw, o, n, rank, x);
  }
}

// What a thread that holds a row (`mine`: cnt >= 1) does with it: places one or two ids itself, lists a row longer than
// a wave for long_rows_in_order (n_long zeroed before), and takes part in the wave's rows.  Every lane of the wave must
// call.
template <class Emit>
__device__ __forceinline__ void short_rows_in_order(bool mine, unsigned int row, long long off, int cnt,
                                                    const unsigned int* __restrict__ ids, unsigned int* __restrict__ long_rows,
                                                    unsigned long long* n_long, Emit emit) {
  if (mine && cnt > WAVE_ROW_MAX) {
    long_rows[atomicAdd(n_long, 1ull)] = row;
    mine = false;
  } else if (mine && cnt <= 2) {  // (most rows)
    const unsigned int a = ids[off], b = cnt == 2 ? ids[off + 1] : a;
    emit(row, off, cnt, 0, a < b ? a : b);
    if (cnt == 2) emit(row, off, cnt, 1, a < b ? b : a);
    mine = false;
  }
  wave_rows_in_order(mine, row, off, cnt, ids, emit);
}

// A row longer than HUGE_ROW: ranking by counting is quadratic in the row (a hub with a million neighbours would hold
// one workgroup for an hour), so such a row goes through a bitmap over the id space instead — clear, set one bit per
// id, prefix-count the words, read the ids off in order: O(ids / 32 + row) for a workgroup, whatever the row's length.
// bits: this workgroup's scratch of `words` words; emit(rank, id).  All 256 threads of the workgroup call it.
template <class Emit>
__device__ __forceinline__ void huge_row_in_order(const unsigned int* __restrict__ ids, long long cnt, unsigned int* bits,
                                                  long long words, unsigned int* s_wave /*[4]*/, Emit emit) {
  for (long long w = threadIdx.x; w < words; w += 256) bits[w] = 0u;
  __threadfence();
  __syncthreads();
  for (long long j = threadIdx.x; j < cnt; j += 256) atomicOr(&bits[ids[j] >> 5], 1u << (ids[j] & 31u));
  __threadfence();
  __syncthreads();
  const long long per = (words + 255) / 256;
  const long long w0 = (long long)threadIdx.x * per, w1 = w0 + per < words ? w0 + per : words;
  unsigned int mine = 0;
  for (long long w = w0; w < w1; ++w)
    mine += (unsigned int)__popc(__hip_atomic_load(bits + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  unsigned int total;
  unsigned int rank = block_exscan_256(mine, &total, s_wave);
  for (long long w = w0; w < w1; ++w) {
    unsigned int v = __hip_atomic_load(bits + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (v) {
      const int b = __ffs((int)v) - 1;
      v &= v - 1u;
      emit((long long)rank++, (unsigned int)(w * 32 + b));
    }
  }
  __syncthreads();
}

// The listed long rows, by a grid of workgroups of 256 threads: a workgroup per row up to HUGE_ROW, where every element
// finds its rank among the row's (distinct) ids by counting the smaller ones; the rows beyond go to the first HUB_BLOCKS
// workgroups, each with its own slice of `hub_words` words of hub_bits.  span(row) gives where the row's ids lie in
// `ids`.
struct RowSpan {
  long long off;
  int cnt;
};
template <class Span, class Emit>
__device__ __forceinline__ void long_rows_in_order(const unsigned int* __restrict__ long_rows, unsigned long long n_long,
                                                   Span span, const unsigned int* __restrict__ ids, unsigned int* hub_bits,
                                                   long long hub_words, unsigned int* s_wave /*[4]*/, Emit emit) {
  for (unsigned long long q = blockIdx.x; q < n_long; q += gridDim.x) {
    const unsigned int row = long_rows[q];
    const RowSpan s = span(row);
    // emit may write where span reads (the record of a live row holds its offset and count and receives its first
    // entry): nobody emits before everybody has read.  One barrier per long row, for every caller.
    __syncthreads();
    if (s.cnt > HUGE_ROW) continue;
    for (int j = threadIdx.x; j < s.cnt; j += 256) {
      const unsigned int x = ids[s.off + j];
      int rank = 0;
      for (int i = 0; i < s.cnt; ++i) rank += ids[s.off + i] < x ? 1 : 0;
      emit(row, s.off, s.cnt, rank, x);
    }
  }
  if (blockIdx.x >= HUB_BLOCKS) return;
  for (unsigned long long q = blockIdx.x; q < n_long; q += HUB_BLOCKS) {  // (block-uniform: every thread takes the same rows)
    const unsigned int row = long_rows[q];
    const RowSpan s = span(row);
    if (s.cnt <= HUGE_ROW) continue;  // (huge_row_in_order starts with a barrier: everybody has read the span by then)
    huge_row_in_order(ids + s.off, (long long)s.cnt, hub_bits + (long long)blockIdx.x * hub_words, hub_words, s_wave,
                      [&](long long rank, unsigned int id) { emit(row, s.off, s.cnt, rank, id); });
  }
}

// ------------------------------------------------------------------ how a walker reads a row
// Two views answer the same three questions: a row's live count, its first entry in list order, the target of its q-th
// entry.  GView (amg_internal.h) reads the live lists; RView reads tip clipping's one-pass row summary, both made by
// amg_live_rows.hip.
// INVARIANT the tip walk keeps and RView relies on: an ENTRY is only taken from a row of a node with at most two live
// edges in all (the walk starts at a node of degree 1 and only moves on to nodes of degree 1 or 2; the closed test looks
// at path nodes alone), so both edges of every row it reads are in the slots.  Of rows with more than two live edges
// only the count is read (a neighbour's degree).
struct RView {
  const int4* rows;  // {live count, edge id of ticket 0, of ticket 1, unused}
  const int* e_tgt;
  const signed char* e_tdir;
  const unsigned char* n_alive;
  const unsigned int* n_cov;
  const long long* n_first;
  const int* n_comp;
};

__device__ __forceinline__ int row_count(const GView& g, long long row) { return g.lrows[row].y; }
__device__ __forceinline__ int row_first(const GView& g, long long row, int* tgt, int* tdir) {
  const int4 rw = g.lrows[row];
  *tgt = rw.z;
  *tdir = rw.w;
  return rw.y;
}
__device__ __forceinline__ int row_target(const GView& g, long long row, int q) {
  const int4 rw = g.lrows[row];
  return q == 0 ? rw.z : g.lent[rw.x + q].x;
}
__device__ __forceinline__ int row_count(const RView& g, long long row) { return g.rows[row].x; }
__device__ __forceinline__ int row_first(const RView& g, long long row, int* tgt, int* tdir) {
  const int4 rw = g.rows[row];
  if (rw.x == 0) return 0;
  // list order is edge-id order: of two edges the smaller id is first
  const int e = (rw.x == 1 || rw.y < rw.z) ? rw.y : rw.z;
  *tgt = g.e_tgt[e];
  *tdir = (int)g.e_tdir[e];
  return rw.x;
}
__device__ __forceinline__ int row_target(const RView& g, long long row, int q) {
  const int4 rw = g.rows[row];
  return g.e_tgt[q == 0 ? rw.y : rw.z];
}

// get_degree (:326-329): live edge classes on both sides
template <class View>
__device__ __forceinline__ int node_degree(const View& g, int n) {
  return row_count(g, 2ll * n) + row_count(g, 2ll * n + 1);
}

// get_forward_node_from_node (:722-741) / get_backward_node_from_node (:781-802):
// forward needs EXACTLY one live forward edge, backward takes the FIRST live backward edge.
// returns 0 = no edge, 1 = edge but cannot extend, 2 = extend
template <class View>
__device__ __forceinline__ int lin_step(const View& g, int n, bool use_forward, int* tgt, int* tdir) {
  const long long row = 2ll * n + (use_forward ? 0 : 1);
  int t = 0, d = 0;
  const int cnt = row_first(g, row, &t, &d);
  if (cnt == 0 || (use_forward && cnt != 1)) return 0;
  *tgt = t;
  *tdir = d;
  const int deg = node_degree(g, *tgt);
  return ((deg == 1 || deg == 2) && *tgt != n) ? 2 : 1;
}

// tip clipping's row summary (amg_live_rows.hip): row_summary_reserve hands the range to zero to the caller's clear
// list, row_summary fills the cleared rows and returns the view of them.  (Declared here, not with the unit's other
// host entries in amg_internal.h: RView is a device-side view and lives in this header.)
int row_summary_reserve(amg_ctx* c, ClearList* cl);
RView row_summary(amg_ctx* c);
