// amg_live_rows.hip — the adjacency of the LIVE edges, which every walker reads (tip clipping, the re-threading search
// of the correction, the junction search of bubble popping: GView, amg_internal.h): its lists (ensure_live_adj) and tip clipping's
// one-pass row summary where no lists exist (row_summary).  What a removal or a build does to the lists' state
// (LiveLists): amg_state.h.  The removals themselves are amg_filter.hip's; the full lists of the graph as built are
// amg_adjacency.hip's; a row's ids are put in order by amg_rows.h.
#include "amg_rows.h"

// ------------------------------------------------------------------ the lists from the live edges
// One scan over the edges' alive bytes squeezes the removed edges out in edge order: its emitter writes the dense list of
// live edges with their rows itself (prim_exscan_live_edges; no position per edge is written and read back).  The rows
// are then made from that list WITHOUT a sort (a library radix sort of a few ten thousand pairs is a dozen launches).
// The live edges of a row are few (one side of one node), so:
//   k_lr_count   every live edge adds 1 to its row's counter                          (rows zeroed before)
//   k_lr_alloc   every live edge takes a ticket of its row; ticket 0 reserves the row's stretch of the entry
//                array — stretches are handed out per workgroup with ONE atomicAdd (their order is irrelevant)
//   k_lr_fill    every live edge drops its edge id into its row's stretch at its ticket (any order)
//   k_lr_finish  the ticket-0 edge of a row puts the row's ids in ascending order (= list order of the reference: edge
//                ids follow insertion order; short_rows_in_order, amg_rows.h) and writes the entries {target, direction}
//                and the row record; rows longer than a wave's 64 lanes are left to k_lr_long (hub nodes)
// The walkers then never touch a dead edge (a hub node of an uncorrected graph lists hundreds of them), and the lists
// of the removed edges are never made at all.
__global__ void k_lr_count(const unsigned int* __restrict__ keys, long long n_live, int4* __restrict__ lrows) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_live) atomicAdd(&lrows[keys[i]].y, 1);
}

// (LR_PER edges per thread: the pool word takes ~90 returning atomics per microsecond, and a workgroup per 256 of a
// million live edges spent 45 of this kernel's 64 us queueing there)
#define LR_PER 8
__global__ __launch_bounds__(256) void k_lr_alloc(const unsigned int* __restrict__ keys, long long n_live,
                                                  int4* __restrict__ lrows, unsigned int* __restrict__ tick,
                                                  unsigned long long* pool) {
  __shared__ unsigned int s_wave[4];
  __shared__ unsigned long long s_base;
  const long long i0 = (long long)blockIdx.x * (256 * LR_PER) + threadIdx.x;
  unsigned int cnt[LR_PER], key[LR_PER], mine = 0;
#pragma unroll
  for (int j = 0; j < LR_PER; ++j) {
    const long long i = i0 + (long long)j * 256;
    cnt[j] = 0;
    key[j] = 0;
    if (i < n_live) {
      key[j] = keys[i];
      const unsigned int t = (unsigned int)atomicAdd(&lrows[key[j]].z, 1);
      tick[i] = t;
      if (t == 0) cnt[j] = (unsigned int)lrows[key[j]].y | 0x80000000u;  // final: k_lr_count is a launch of its own
      mine += cnt[j] & 0x7fffffffu;
    }
  }
  unsigned int total;
  unsigned int off = block_exscan_256(mine, &total, s_wave);
  if (threadIdx.x == 0) s_base = total ? atomicAdd(pool, (unsigned long long)total) : 0ull;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < LR_PER; ++j)
    if (cnt[j] & 0x80000000u) {  // this edge drew ticket 0 of its row: it places the row's stretch
      lrows[key[j]].x = (int)(s_base + off);
      off += cnt[j] & 0x7fffffffu;
    }
}

// (a row with ONE live edge — most rows: a node of a cleaned graph has one forward and one backward neighbour — is
// finished right here: entry and row record written by the edge that drew its only ticket, which is marked done; the
// ticket-0 pass that puts rows in order then touches the rows with two edges and more alone.  On the 7.4 M rows of a
// rebuilt graph of eight read sets that pass took 0.92 ms with every row going through it.)
#define LR_DONE 0xffffffffu
__global__ void k_lr_fill(const unsigned int* __restrict__ keys, const unsigned int* __restrict__ edge_of,
                          unsigned int* __restrict__ tick, long long n_live, int4* __restrict__ lrows,
                          const int* __restrict__ e_tgt, const signed char* __restrict__ e_tdir,
                          unsigned int* __restrict__ tmp, int2* __restrict__ lent) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_live) return;
  const unsigned int key = keys[i], e = edge_of[i];
  const int4 rw = lrows[key];
  if (rw.y == 1) {
    const int t = e_tgt[e], d = (int)e_tdir[e];
    lent[rw.x] = make_int2(t, d);
    lrows[key] = make_int4(rw.x, 1, t, d);
    tick[i] = LR_DONE;
    return;
  }
  tmp[rw.x + tick[i]] = e;
}

// what the ordering steps do with the id ranked `rank` in its row: the entry goes to its place, and the first entry
// completes the row record {offset, live count, first target, first direction}
struct LiveEmit {
  const int* __restrict__ e_tgt;
  const signed char* __restrict__ e_tdir;
  int4* __restrict__ lrows;
  int2* __restrict__ lent;
  __device__ __forceinline__ void operator()(unsigned int row, long long off, int cnt, long long rank, unsigned int e) const {
    const int t = e_tgt[e], d = (int)e_tdir[e];
    lent[off + rank] = make_int2(t, d);
    if (rank == 0) lrows[row] = make_int4((int)off, cnt, t, d);
  }
};

__global__ __launch_bounds__(256) void k_lr_finish(const unsigned int* __restrict__ keys, const unsigned int* __restrict__ tick,
                                                   long long n_live, const unsigned int* __restrict__ tmp,
                                                   const int* __restrict__ e_tgt, const signed char* __restrict__ e_tdir,
                                                   int4* __restrict__ lrows, int2* __restrict__ lent,
                                                   unsigned int* __restrict__ long_rows, unsigned long long* n_long) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const bool mine = i < n_live && tick[i] == 0u;  // the ticket-0 edge of a row with two live edges or more
  unsigned int key = 0;
  int off = 0, cnt = 0;
  if (mine) {
    key = keys[i];
    off = lrows[key].x;
    cnt = lrows[key].y;
  }
  short_rows_in_order(mine, key, (long long)off, cnt, tmp, long_rows, n_long, LiveEmit{e_tgt, e_tdir, lrows, lent});
}

__global__ __launch_bounds__(256) void k_lr_long(const unsigned int* __restrict__ long_rows,
                                                 const unsigned long long* __restrict__ n_long,
                                                 const unsigned int* __restrict__ tmp, const int* __restrict__ e_tgt,
                                                 const signed char* __restrict__ e_tdir, int4* __restrict__ lrows,
                                                 int2* __restrict__ lent, unsigned int* hub_bits, long long hub_words) {
  __shared__ unsigned int s_wave[4];
  // (the record a row's span is read from is the one LiveEmit rewrites: long_rows_in_order's barrier)
  long_rows_in_order(
      long_rows, *n_long, [&](unsigned int row) { return RowSpan{(long long)lrows[row].x, lrows[row].y}; }, tmp, hub_bits,
      hub_words, s_wave, LiveEmit{e_tgt, e_tdir, lrows, lent});
}

// The live lists after NODES died: a row of a dead node empties, the other rows drop their entries with a dead
// target, in place and in order — one pass over the row records with the targets' alive bytes out of the L2, where
// making the lists again from the live edges is a flag, a scan and five passes over them
__global__ void k_lr_patch(int4* __restrict__ lrows, int2* __restrict__ lent, long long n_rows,
                           const unsigned char* __restrict__ n_alive) {
  long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rows) return;
  const int4 rw = lrows[r];
  if (rw.y == 0) return;
  if (!n_alive[r >> 1]) {
    lrows[r] = make_int4(rw.x, 0, 0, 0);
    return;
  }
  if (rw.y == 1) {
    if (!n_alive[rw.z]) lrows[r] = make_int4(rw.x, 0, 0, 0);
    return;
  }
  int w = 0;
  int2 first = make_int2(0, 0);
  for (int j = 0; j < rw.y; ++j) {
    const int2 e = lent[rw.x + j];
    if (!n_alive[e.x]) continue;
    if (w != j) lent[rw.x + w] = e;
    if (w == 0) first = e;
    ++w;
  }
  if (w != rw.y) lrows[r] = make_int4(rw.x, w, first.x, first.y);
}

int ensure_live_adj(amg_ctx* c) {
  if (c->live_lists == LiveLists::Current) return AMG_OK;
  hipStream_t st = c->stream;
  if (c->live_lists == LiveLists::BehindNodes) {
    hipLaunchKernelGGL(k_lr_patch, dim3(nblk(2 * c->n_nodes, 256)), dim3(256), 0, st, c->ladj_rows.as<int4>(),
                       c->ladj.as<int2>(), 2 * c->n_nodes, c->node_alive.as<unsigned char>());
    live_lists_made(c);
    return AMG_OK;
  }
  const long long rows = 2 * c->n_nodes, E = c->n_edges;
  AMGCHK(c->ladj_rows.ensure((size_t)(rows + 2) * sizeof(int4)));
  // the dense list {row, edge id}: two arrays of E + 2 words, and behind them the number of live edges
  AMGCHK(c->ladj_pos.ensure((size_t)(E + 3) * sizeof(long long)));
  unsigned int* keys = c->ladj_pos.as<unsigned int>();
  unsigned int* edge_of = keys + (E + 2);
  long long* d_total = c->ladj_pos.as<long long>() + (E + 2);
  unsigned long long* ctr = c->status.as<unsigned long long>() + ST_COMPACT_A;  // [0] entries handed out, [1] long rows
  {  // the rows and counters are zeroed by the scan's workgroups
    ClearList cl;
    cl.add(c->ladj_rows.p, (size_t)(rows + 2) * sizeof(int4));
    cl.add(ctr, 2 * sizeof(unsigned long long));
    AMGCHK(prim_exscan_live_edges(c, c->edge_alive.as<unsigned char>(), c->edge_src.as<int>(), c->edge_sdir.as<signed char>(),
                                  (size_t)E, d_total, keys, edge_of, &cl));
  }
  long long total = 0;
  {
    FetchList l;
    l.add(d_total);
    AMGCHK(fetch(c, l, reinterpret_cast<unsigned long long*>(&total)));
  }
  AMGCHK(c->ladj.ensure((size_t)(total + 1) * sizeof(int2)));
  AMGCHK(c->ladj_keys.ensure(3 * (size_t)(total + 2) * sizeof(unsigned int)));
  unsigned int* tick = c->ladj_keys.as<unsigned int>();
  unsigned int* tmp = tick + (total + 2);
  unsigned int* long_rows = tmp + (total + 2);
  if (total > 0) {
    hipLaunchKernelGGL(k_lr_count, dim3(nblk(total, 256)), dim3(256), 0, st, keys, total, c->ladj_rows.as<int4>());
    hipLaunchKernelGGL(k_lr_alloc, dim3(nblk(total, 256 * LR_PER)), dim3(256), 0, st, keys, total, c->ladj_rows.as<int4>(),
                       tick, ctr);
    hipLaunchKernelGGL(k_lr_fill, dim3(nblk(total, 256)), dim3(256), 0, st, keys, edge_of, tick, total,
                       c->ladj_rows.as<int4>(), c->edge_tgt.as<int>(), c->edge_tdir.as<signed char>(), tmp, c->ladj.as<int2>());
    hipLaunchKernelGGL(k_lr_finish, dim3(nblk(total, 256)), dim3(256), 0, st, keys, tick, total, tmp, c->edge_tgt.as<int>(),
                       c->edge_tdir.as<signed char>(), c->ladj_rows.as<int4>(), c->ladj.as<int2>(), long_rows, ctr + 1);
    const long long hub_words = (E + 31) / 32 + 1;  // (scratch of the hub rows: HUB_BLOCKS bitmaps over the edge ids)
    AMGCHK(c->hub_bits.ensure((size_t)HUB_BLOCKS * (size_t)hub_words * sizeof(unsigned int)));
    hipLaunchKernelGGL(k_lr_long, dim3(64), dim3(256), 0, st, long_rows, ctr + 1, tmp, c->edge_tgt.as<int>(),
                       c->edge_tdir.as<signed char>(), c->ladj_rows.as<int4>(), c->ladj.as<int2>(),
                       c->hub_bits.as<unsigned int>(), hub_words);
  }
  live_lists_made(c);
  return AMG_OK;
}

GView make_view(amg_ctx* c) {
  GView g;
  g.lent = c->ladj.as<int2>();
  g.lrows = c->ladj_rows.as<int4>();
  g.n_alive = c->node_alive.as<unsigned char>();
  g.n_cov = c->node_cov.as<unsigned int>();
  g.n_tok = c->node_tokens.as<int>();
  g.n_first = c->node_first.as<long long>();
  g.n_comp = c->node_comp.as<int>();
  g.k = c->k;
  g.flip = c->two_v - 1;
  return g;
}

// ------------------------------------------------------------------ row summary for the tip walk
// Tip clipping asks little of a row: how many live edges it has and, on rows of nodes with one or two live edges in
// all, which they are.  One pass over the directed edges answers that — no scan, no compaction, no read-back, no
// entry array: every live edge takes a ticket of its row {count, e0, e1, -} and the holders of tickets 0 and 1 leave
// their edge ids in the row's two slots (rows zeroed before).  Which two edges of a longer row land there depends on
// the order of the atomics; the walk never looks (RView, amg_rows.h).
__global__ void k_row_tickets(const unsigned char* __restrict__ e_alive, const int* __restrict__ e_src,
                              const signed char* __restrict__ e_sdir, long long n_edges, int4* __restrict__ rows) {
  long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_edges || !e_alive[e]) return;
  int* r = reinterpret_cast<int*>(rows + adj_row_of(e_src[e], e_sdir[e]));
  const int t = atomicAdd(r, 1);
  if (t < 2) r[1 + t] = (int)e;
}

// The summary lives in ladj_rows, which is free exactly while the state of the lists is Absent, and leaves that state
// alone: whoever needs lists next makes them from the edges, never by patching rows that are not lists.
int row_summary_reserve(amg_ctx* c, ClearList* cl) {
  const size_t bytes = (size_t)(2 * c->n_nodes + 2) * sizeof(int4);
  AMGCHK(c->ladj_rows.ensure(bytes));
  cl->add(c->ladj_rows.p, bytes);
  return AMG_OK;
}

RView row_summary(amg_ctx* c) {
  if (c->n_edges > 0)
    hipLaunchKernelGGL(k_row_tickets, dim3(nblk(c->n_edges, 256)), dim3(256), 0, c->stream,
                       c->edge_alive.as<unsigned char>(), c->edge_src.as<int>(), c->edge_sdir.as<signed char>(), c->n_edges,
                       c->ladj_rows.as<int4>());
  RView v;
  v.rows = c->ladj_rows.as<int4>();
  v.e_tgt = c->edge_tgt.as<int>();
  v.e_tdir = c->edge_tdir.as<signed char>();
  v.n_alive = c->node_alive.as<unsigned char>();
  v.n_cov = c->node_cov.as<unsigned int>();
  v.n_first = c->node_first.as<long long>();
  v.n_comp = c->node_comp.as<int>();
  return v;
}
