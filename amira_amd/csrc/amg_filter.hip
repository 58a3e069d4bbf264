// amg_filter.hip — coverage filter, listed node / edge removals, the live adjacency the walkers use, tip clipping
// and the component filter on the device (reference construct_graph.py:402-540, 679-861, 950-958).
#include "amg_device.h"

// ------------------------------------------------------------------ filter_graph (:523-540)
// list_nodes_to_remove (:496-503): coverage < minNodeCoverage
__global__ void k_filter_nodes(const unsigned int* __restrict__ cov, unsigned char* __restrict__ alive,
                               long long n, unsigned int min_cov) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && alive[i] && cov[i] < min_cov) alive[i] = 0;
}

// list_edges_to_remove (:505-521): coverage < minEdgeCoverage or a doomed endpoint
__global__ void k_filter_edges(const int* __restrict__ src, const int* __restrict__ tgt,
                               const unsigned int* __restrict__ cov,
                               const unsigned char* __restrict__ node_alive,
                               unsigned char* __restrict__ alive, long long n, unsigned int min_cov) {
  long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n || !alive[e]) return;
  // (an edge's coverage is at least 1: with the usual threshold of 1 the coverage array is not read at all)
  if ((min_cov > 1 && cov[e] < min_cov) || !node_alive[src[e]] || !node_alive[tgt[e]]) alive[e] = 0;
}

// remove_node_from_reads (:442-461): one wave per read; windows of removed nodes become
// None (-2) and the read joins _readsToCorrect
// Wave-per-read kernels move ~60 windows per read: one read per wave is bound by the chain
// offsets -> ids -> flags of a single short read.  Each wave therefore takes READS_PER_WAVE
// consecutive reads and issues every load of one stage for all of them before using any.
#define READS_PER_WAVE 8  // (2 / 4 / 8: filter stage 0.27 / 0.22 / 0.21 ms)
__global__ __launch_bounds__(256) void k_mask_reads(int* __restrict__ tok_node,
                                                    const long long* __restrict__ read_off,
                                                    long long n_reads,
                                                    const unsigned char* __restrict__ node_alive,
                                                    unsigned char* __restrict__ read_fix) {
  const long long rbase = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * READS_PER_WAVE;
  if (rbase >= n_reads) return;
  const int lane = threadIdx.x & 63;
  const long long off_l = (lane <= READS_PER_WAVE && rbase + lane <= n_reads) ? read_off[rbase + lane] : 0;
  long long a[READS_PER_WAVE], b[READS_PER_WAVE];
  int v[READS_PER_WAVE];
#pragma unroll
  for (int j = 0; j < READS_PER_WAVE; ++j) {
    a[j] = __shfl(off_l, j, 64);
    b[j] = rbase + j < n_reads ? __shfl(off_l, j + 1, 64) : a[j];
  }
#pragma unroll
  for (int j = 0; j < READS_PER_WAVE; ++j) v[j] = a[j] + lane < b[j] ? tok_node[a[j] + lane] : -1;
  bool dead[READS_PER_WAVE];
#pragma unroll
  for (int j = 0; j < READS_PER_WAVE; ++j) dead[j] = v[j] >= 0 && !node_alive[v[j]];
#pragma unroll
  for (int j = 0; j < READS_PER_WAVE; ++j) {
    if (dead[j]) tok_node[a[j] + lane] = -2;
    bool hit = dead[j];
    for (long long t = a[j] + 64 + lane; t < b[j]; t += 64) {  // reads longer than one wave
      const int n = tok_node[t];
      if (n >= 0 && !node_alive[n]) {
        tok_node[t] = -2;
        hit = true;
      }
    }
    if (__any(hit) && lane == 0) read_fix[rbase + j] = 1;
  }
}

static int apply_removals(amg_ctx* c, unsigned int min_edge_cov) {
  hipStream_t st = c->stream;
  // NODES died, and every edge that dies with them has a dead end (no edge falls to a coverage threshold of its own):
  // live lists that exist stay and are brought up to date when somebody walks them again (ensure_live_adj: k_lr_patch)
  if (c->ladj_valid && min_edge_cov <= 1 && !getenv("AMG_NO_LADJ_PATCH")) c->ladj_stale = true;  // (A/B + test switch)
  else if (!c->ladj_stale || min_edge_cov > 1) c->ladj_stale = false;
  c->ladj_valid = false;
  c->pristine = false;
  if (min_edge_cov > 1) c->edge_own_deaths = true;
  c->match_valid = false;  // node-id patterns of a cached K6 result may name removed nodes
  if (c->n_edges > 0)
    hipLaunchKernelGGL(k_filter_edges, dim3(nblk(c->n_edges, 256)), dim3(256), 0, st,
                       c->edge_src.as<int>(), c->edge_tgt.as<int>(), c->edge_cov.as<unsigned int>(),
                       c->node_alive.as<unsigned char>(), c->edge_alive.as<unsigned char>(),
                       c->n_edges, min_edge_cov);
  if (c->n_reads > 0)
    hipLaunchKernelGGL(k_mask_reads, dim3(nblk(c->n_reads, 4 * READS_PER_WAVE)), dim3(256), 0, st,
                       c->tok_node.as<int>(), c->read_off.as<long long>(), c->n_reads,
                       c->node_alive.as<unsigned char>(), c->read_fix.as<unsigned char>());
  return AMG_OK;
}

extern "C" int amg_filter(amg_ctx* c, uint32_t min_node_cov, uint32_t min_edge_cov) {
  NEED_BUILT(c);
  stages_reset(c);
  stage_begin(c, "filter");
  if (c->n_nodes > 0)
    hipLaunchKernelGGL(k_filter_nodes, dim3(nblk(c->n_nodes, 256)), dim3(256), 0, c->stream,
                       c->node_cov.as<unsigned int>(), c->node_alive.as<unsigned char>(),
                       c->n_nodes, min_node_cov);
  AMGCHK(apply_removals(c, min_edge_cov));
  stage_end(c);
  c->have_corrected = false;
  return AMG_OK;
}

// ------------------------------------------------------------------ remove_node (:463-484)
__global__ void k_kill_listed(const int* __restrict__ ids, long long n, long long n_nodes,
                              unsigned char* __restrict__ alive) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int v = ids[i];
  if (v >= 0 && v < n_nodes) alive[v] = 0;
}

extern "C" int amg_remove_nodes(amg_ctx* c, const int32_t* node_ids, int64_t n) {
  NEED_BUILT(c);
  if (n < 0 || (n > 0 && !node_ids)) return amg_fail(AMG_E_ARG, "bad node list");
  if (n == 0) return AMG_OK;
  AMGCHK(c->s0.ensure((size_t)n * sizeof(int)));
  HIPCHK(hipMemcpyAsync(c->s0.p, node_ids, (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_kill_listed, dim3(nblk(n, 256)), dim3(256), 0, c->stream, c->s0.as<int>(),
                     (long long)n, c->n_nodes, c->node_alive.as<unsigned char>());
  AMGCHK(apply_removals(c, 0));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->have_corrected = false;
  return AMG_OK;
}


// ------------------------------------------------------------------ graph view for walkers
// (GView: amg_internal.h)

// Live adjacency straight from the live edges: flag + scan squeezes the removed edges out in edge
// order, a stable sort by row (2 * source + side) groups them, so a row lists its live edges in
// the order of the reference's forward / backward lists (edge ids ascend in insertion order).
__global__ void k_live_keys(const unsigned char* __restrict__ e_alive, const int* __restrict__ e_src,
                            const signed char* __restrict__ e_sdir, const long long* __restrict__ pos,
                            long long n_edges, unsigned int* __restrict__ keys, unsigned int* __restrict__ vals) {
  long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_edges || !e_alive[e]) return;
  const long long o = pos[e];
  keys[o] = 2u * (unsigned int)e_src[e] + (e_sdir[e] > 0 ? 0u : 1u);
  vals[o] = (unsigned int)e;
}

// Rows from the dense list of live edges WITHOUT a sort (a library radix sort of a few ten thousand pairs is a
// dozen launches).  The live edges of a row are few (one side of one node), so:
//   k_lr_count   every live edge adds 1 to its row's counter                          (rows zeroed before)
//   k_lr_alloc   every live edge takes a ticket of its row; ticket 0 reserves the row's stretch of the entry
//                array — stretches are handed out per workgroup with ONE atomicAdd (their order is irrelevant)
//   k_lr_fill    every live edge drops its edge id into its row's stretch at its ticket (any order)
//   k_lr_finish  the ticket-0 edge of a row sorts the row's ids ascending (= list order of the reference: edge ids
//                follow insertion order) and writes the entries {target, direction} and the row record; rows longer
//                than a wave's 64 lanes are left to k_lr_long, a workgroup per long row (hub nodes)
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

__global__ __launch_bounds__(256) void k_lr_finish(const unsigned int* __restrict__ keys, const unsigned int* __restrict__ tick,
                                                   long long n_live, const unsigned int* __restrict__ tmp,
                                                   const int* __restrict__ e_tgt, const signed char* __restrict__ e_tdir,
                                                   int4* __restrict__ lrows, int2* __restrict__ lent,
                                                   unsigned int* __restrict__ long_rows, unsigned long long* n_long) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  bool mine = i < n_live && tick[i] == 0u;  // the ticket-0 edge of a row with two live edges or more
  unsigned int key = 0;
  int off = 0, cnt = 0;
  if (mine) {
    key = keys[i];
    off = lrows[key].x;
    cnt = lrows[key].y;
    if (cnt > WAVE_ROW_MAX) {
      long_rows[atomicAdd(n_long, 1ull)] = key;
      mine = false;
    } else if (cnt == 2) {  // (most of what is left)
      unsigned int a = tmp[off], b = tmp[off + 1];
      if (a > b) {
        const unsigned int t = a;
        a = b;
        b = t;
      }
      const int ta = e_tgt[a], da = (int)e_tdir[a];
      lent[off] = make_int2(ta, da);
      lent[off + 1] = make_int2(e_tgt[b], (int)e_tdir[b]);
      lrows[key] = make_int4(off, 2, ta, da);
      mine = false;
    }
  }
  wave_rows_in_order(mine, key, (long long)off, cnt, tmp, [&](unsigned int row, long long o, int n, int rank, unsigned int x) {
    const int t = e_tgt[x], d = (int)e_tdir[x];
    lent[o + rank] = make_int2(t, d);
    if (rank == 0) lrows[row] = make_int4((int)o, n, t, d);
  });
}

// a workgroup per long row: every element finds its rank among the row's (distinct) edge ids; rows beyond HUGE_ROW are
// left to the first LR_HUB_BLOCKS workgroups, which put them in order through a bitmap (huge_row_in_order, amg_device.h)
#define LR_HUB_BLOCKS 8
__global__ __launch_bounds__(256) void k_lr_long(const unsigned int* __restrict__ long_rows,
                                                 const unsigned long long* __restrict__ n_long,
                                                 const unsigned int* __restrict__ tmp, const int* __restrict__ e_tgt,
                                                 const signed char* __restrict__ e_tdir, int4* __restrict__ lrows,
                                                 int2* __restrict__ lent, unsigned int* hub_bits, long long hub_words) {
  __shared__ unsigned int s_wave[4];
  const unsigned long long n = *n_long;
  for (unsigned long long r = blockIdx.x; r < n; r += gridDim.x) {
    const unsigned int key = long_rows[r];
    const int off = lrows[key].x, cnt = lrows[key].y;
    __syncthreads();  // (the row record is rewritten below: everybody has read it)
    if (cnt > HUGE_ROW) continue;
    for (int j = threadIdx.x; j < cnt; j += 256) {
      const unsigned int x = tmp[off + j];
      int rank = 0;
      for (int q = 0; q < cnt; ++q) rank += tmp[off + q] < x ? 1 : 0;
      lent[off + rank] = make_int2(e_tgt[x], (int)e_tdir[x]);
      if (rank == 0) lrows[key] = make_int4(off, cnt, e_tgt[x], (int)e_tdir[x]);
    }
  }
  if (blockIdx.x >= LR_HUB_BLOCKS) return;
  for (unsigned long long r = blockIdx.x; r < n; r += LR_HUB_BLOCKS) {  // (block-uniform)
    const unsigned int key = long_rows[r];
    const int off = lrows[key].x, cnt = lrows[key].y;
    if (cnt <= HUGE_ROW) continue;  // (huge_row_in_order starts with a barrier: the record has been read by then)
    huge_row_in_order(tmp + off, (long long)cnt, hub_bits + (long long)blockIdx.x * hub_words, hub_words, s_wave,
                      [&](long long rank, unsigned int x) {
                        lent[off + rank] = make_int2(e_tgt[x], (int)e_tdir[x]);
                        if (rank == 0) lrows[key] = make_int4(off, cnt, e_tgt[x], (int)e_tdir[x]);
                      });
  }
}

// forward/backward edge lists with the removed edges squeezed out: the walkers below then
// never touch a dead edge (a hub node of an uncorrected graph lists hundreds of them), and the
// lists of the removed edges are never made at all
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
  if (c->ladj_valid) return AMG_OK;
  hipStream_t st = c->stream;
  if (c->ladj_stale) {
    hipLaunchKernelGGL(k_lr_patch, dim3(nblk(2 * c->n_nodes, 256)), dim3(256), 0, st, c->ladj_rows.as<int4>(),
                       c->ladj.as<int2>(), 2 * c->n_nodes, c->node_alive.as<unsigned char>());
    c->ladj_stale = false;
    c->ladj_valid = true;
    return AMG_OK;
  }
  const long long rows = 2 * c->n_nodes, E = c->n_edges;
  AMGCHK(c->ladj_rows.ensure((size_t)(rows + 2) * sizeof(int4)));
  AMGCHK(c->ladj_pos.ensure((size_t)(E + 2) * sizeof(long long)));
  unsigned long long* ctr = c->status.as<unsigned long long>() + ST_COMPACT_A;  // [0] entries handed out, [1] long rows
  {  // the rows and counters are zeroed by the scan's workgroups
    ClearList cl;
    cl.add(c->ladj_rows.p, (size_t)(rows + 2) * sizeof(int4));
    cl.add(ctr, 2 * sizeof(unsigned long long));
    AMGCHK(prim_exscan_bytes_set(c, c->edge_alive.as<unsigned char>(), c->ladj_pos.as<long long>(), (size_t)E, &cl));
  }
  long long total = 0;
  {
    FetchList l;
    l.add(c->ladj_pos.as<long long>() + E);
    AMGCHK(fetch(c, l, reinterpret_cast<unsigned long long*>(&total)));
  }
  AMGCHK(c->ladj.ensure((size_t)(total + 1) * sizeof(int2)));
  AMGCHK(c->ladj_keys.ensure(5 * (size_t)(total + 2) * sizeof(unsigned int)));
  unsigned int* keys = c->ladj_keys.as<unsigned int>();
  unsigned int* edge_of = keys + (total + 2);
  unsigned int* tick = edge_of + (total + 2);
  unsigned int* tmp = tick + (total + 2);
  unsigned int* long_rows = tmp + (total + 2);
  if (total > 0) {
    hipLaunchKernelGGL(k_live_keys, dim3(nblk(E, 256)), dim3(256), 0, st, c->edge_alive.as<unsigned char>(),
                       c->edge_src.as<int>(), c->edge_sdir.as<signed char>(), c->ladj_pos.as<long long>(), E, keys,
                       edge_of);
    hipLaunchKernelGGL(k_lr_count, dim3(nblk(total, 256)), dim3(256), 0, st, keys, total, c->ladj_rows.as<int4>());
    hipLaunchKernelGGL(k_lr_alloc, dim3(nblk(total, 256 * LR_PER)), dim3(256), 0, st, keys, total, c->ladj_rows.as<int4>(),
                       tick, ctr);
    hipLaunchKernelGGL(k_lr_fill, dim3(nblk(total, 256)), dim3(256), 0, st, keys, edge_of, tick, total,
                       c->ladj_rows.as<int4>(), c->edge_tgt.as<int>(), c->edge_tdir.as<signed char>(), tmp, c->ladj.as<int2>());
    hipLaunchKernelGGL(k_lr_finish, dim3(nblk(total, 256)), dim3(256), 0, st, keys, tick, total, tmp, c->edge_tgt.as<int>(),
                       c->edge_tdir.as<signed char>(), c->ladj_rows.as<int4>(), c->ladj.as<int2>(), long_rows, ctr + 1);
    const long long hub_words = (E + 31) / 32 + 1;  // (scratch of the hub rows: LR_HUB_BLOCKS bitmaps over the edge ids)
    AMGCHK(c->hub_bits.ensure((size_t)LR_HUB_BLOCKS * (size_t)hub_words * sizeof(unsigned int)));
    hipLaunchKernelGGL(k_lr_long, dim3(64), dim3(256), 0, st, long_rows, ctr + 1, tmp, c->edge_tgt.as<int>(),
                       c->edge_tdir.as<signed char>(), c->ladj_rows.as<int4>(), c->ladj.as<int2>(),
                       c->hub_bits.as<unsigned int>(), hub_words);
  }
  c->ladj_valid = true;
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
// the order of the atomics; the walk never looks (RView below).
__global__ void k_row_tickets(const unsigned char* __restrict__ e_alive, const int* __restrict__ e_src,
                              const signed char* __restrict__ e_sdir, long long n_edges, int4* __restrict__ rows) {
  long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_edges || !e_alive[e]) return;
  int* r = reinterpret_cast<int*>(rows + (2ll * e_src[e] + (e_sdir[e] > 0 ? 0 : 1)));  // (the row of k_live_keys)
  const int t = atomicAdd(r, 1);
  if (t < 2) r[1 + t] = (int)e;
}

// The walker's view of those rows.  INVARIANT the walk keeps and this view relies on: an ENTRY is only taken from a
// row of a node with at most two live edges in all (the walk starts at a node of degree 1 and only moves on to nodes
// of degree 1 or 2; the closed test looks at path nodes alone), so both edges of every row it reads are in the slots.
// Of rows with more than two live edges only the count is read (a neighbour's degree).
struct RView {
  const int4* rows;  // {live count, edge id of ticket 0, of ticket 1, unused}
  const int* e_tgt;
  const signed char* e_tdir;
  const unsigned char* n_alive;
  const unsigned int* n_cov;
  const long long* n_first;
  const int* n_comp;
};

// what the walk asks of a view: a row's live count, its first entry in list order, the target of its q-th entry
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

// ------------------------------------------------------------------ remove_edge (:409-428)
// one DIRECTED edge per listed id leaves the graph (and its source node's forward / backward list); its reverse
// twin stays, as in the reference, until it is removed by its own call
extern "C" int amg_remove_edges(amg_ctx* c, const int32_t* edge_ids, int64_t n) {
  NEED_BUILT(c);
  if (n < 0 || (n > 0 && !edge_ids)) return amg_fail(AMG_E_ARG, "bad edge list");
  if (n == 0) return AMG_OK;
  AMGCHK(c->s0.ensure((size_t)n * sizeof(int)));
  HIPCHK(hipMemcpyAsync(c->s0.p, edge_ids, (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_kill_listed, dim3(nblk(n, 256)), dim3(256), 0, c->stream, c->s0.as<int>(), (long long)n,
                     c->n_edges, c->edge_alive.as<unsigned char>());
  c->ladj_valid = false;
  c->pristine = false;
  c->edge_own_deaths = true;
  c->ladj_stale = false;  // (an edge left with both ends alive: the lists are made again)
  c->match_valid = false;
  HIPCHK(hipStreamSynchronize(c->stream));
  c->have_corrected = false;
  return AMG_OK;
}

// ------------------------------------------------------------------ remove_short_linear_paths (:679-720)
#define CLIP_MAX 64
// acc = {sum of the live nodes' coverages, number of live nodes} (k_comp_hist): the threshold is 1.5 x their mean
// (:868-871, statistics.mean over live nodes) — the quotient of the two integers as doubles is correctly rounded,
// == float(Fraction(sum, n)), on the device as on the host
// View: the live lists (GView) or the row summary (RView) — one walk, two ways to read a row
template <class View>
__global__ void k_clip_mark(View g, long long n_nodes, int min_length, const unsigned long long* __restrict__ acc,
                            const unsigned int* __restrict__ comp_live,
                            const unsigned char* __restrict__ protect,
                            unsigned char* __restrict__ kill) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_nodes || !g.n_alive[i]) return;
  int n = (int)i;
  if (node_degree(g, n) != 1) return;
  int d0 = (g.n_first[n] & 1ll) ? -1 : 1;  // direction of the node's first occurrence (:852-858)
  int path[CLIP_MAX];
  int len = 0;
  path[len++] = n;
  // backward walk, started with -d0 (get_backward_path_from_node, :804-847)
  int tgt = -1, td = 0;
  int r = lin_step(g, n, d0 == -1, &tgt, &td);
  while (r == 2 && tgt != n) {
    if (len >= min_length) return;  // already too long to be clipped
    path[len++] = tgt;
    r = lin_step(g, tgt, td == 1, &tgt, &td);
  }
  // forward walk, started with d0 (get_forward_path_from_node, :743-779)
  r = lin_step(g, n, d0 == 1, &tgt, &td);
  while (r == 2 && tgt != n) {
    if (len >= min_length) return;
    path[len++] = tgt;
    r = lin_step(g, tgt, td == 1, &tgt, &td);
  }
  if (!(len > 0 && len < min_length)) return;
  const double thr = ((double)acc[0] / (double)acc[1]) * 1.5;
  bool all_high = true;
  for (int j = 0; j < len; ++j) all_high = all_high && ((double)g.n_cov[path[j]] > thr);
  if (all_high) return;
  // a tip that IS its whole component is kept (:710-713)
  if (comp_live) {
    int distinct = 0;
    for (int j = 0; j < len; ++j) {
      bool dup = false;
      for (int q = 0; q < j; ++q) dup = dup || (path[q] == path[j]);
      distinct += dup ? 0 : 1;
    }
    if ((unsigned int)distinct == comp_live[g.n_comp[n]]) return;
  } else {
    // nothing has been removed since the build: the component of the path's nodes is the path exactly when no live
    // edge leaves it (its nodes have at most two edges each: the walk only enters nodes of degree one or two)
    bool closed = true;
    for (int j = 0; j < len && closed; ++j)
      for (int side = 0; side < 2 && closed; ++side) {
        const long long row = 2ll * path[j] + side;
        const int cnt = row_count(g, row);  // (at most 2: a path node)
        for (int q = 0; q < cnt && closed; ++q) {
          const int t = row_target(g, row, q);
          bool in = false;
          for (int m = 0; m < len; ++m) in = in || (path[m] == t);
          closed = in;
        }
      }
    if (closed) return;
  }
  for (int j = 0; j < len; ++j)
    if (!protect || !protect[path[j]]) kill[path[j]] = 1;
}

// (grid-stride: a thread first sums up runs of equal ids along its own nodes, so that the giant
// component costs one atomic per WAVE of a small grid — one per wave of a node-sized grid still put
// thousands of atomics on one address, ~90 per microsecond)
__global__ void k_comp_hist(const int* __restrict__ comp, const unsigned char* __restrict__ alive,
                            const unsigned int* __restrict__ cov, long long n, unsigned int min_cov,
                            unsigned int* __restrict__ live_cnt, unsigned int* __restrict__ high_cnt,
                            unsigned long long* __restrict__ acc /* or null: {sum of live coverages, live nodes} */) {
  int cid = -1;
  unsigned int n_live = 0, n_high = 0;
  unsigned long long s_cov = 0, s_n = 0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    if (!alive[i]) continue;
    if (acc) {
      s_cov += cov[i];
      s_n += 1;
    }
    const int id = comp[i];
    if (id != cid) {
      if (cid >= 0) {
        atomicAdd(&live_cnt[cid], n_live);
        if (high_cnt && n_high) atomicAdd(&high_cnt[cid], n_high);
      }
      cid = id;
      n_live = n_high = 0;
    }
    ++n_live;
    n_high += (high_cnt && cov[i] >= min_cov) ? 1u : 0u;
  }
  const int lane = threadIdx.x & 63;
  if (acc) {  // one pair of atomics per WORKGROUP (a pair per wave: two thousand atomics on one line, ~15 us)
    __shared__ unsigned long long s_part[2][4];
    for (int d = 32; d > 0; d >>= 1) {
      s_cov += __shfl_xor(s_cov, d, 64);
      s_n += __shfl_xor(s_n, d, 64);
    }
    if (lane == 0) {
      s_part[0][threadIdx.x >> 6] = s_cov;
      s_part[1][threadIdx.x >> 6] = s_n;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      const unsigned long long n_all = s_part[1][0] + s_part[1][1] + s_part[1][2] + s_part[1][3];
      if (n_all) {
        atomicAdd(&acc[0], s_part[0][0] + s_part[0][1] + s_part[0][2] + s_part[0][3]);
        atomicAdd(&acc[1], n_all);
      }
    }
  }
  bool active = cid >= 0;
  // most nodes share one giant component: aggregate equal ids inside the wave so that a
  // wave issues one atomic per distinct component instead of one per node
  unsigned long long todo = __ballot(active);
  while (todo) {
    const int leader = __ffsll((long long)todo) - 1;
    const int lc = __shfl(cid, leader, 64);
    const bool same = active && cid == lc;
    const unsigned long long m = __ballot(same);
    unsigned int sl = same ? n_live : 0u, sh = same ? n_high : 0u;
    for (int d = 32; d > 0; d >>= 1) {
      sl += __shfl_xor(sl, d, 64);
      sh += __shfl_xor(sh, d, 64);
    }
    if (lane == leader) {
      atomicAdd(&live_cnt[lc], sl);
      if (high_cnt && sh) atomicAdd(&high_cnt[lc], sh);
    }
    active = active && !same;
    todo &= ~m;
  }
}

// {sum of the live nodes' coverages, number of live nodes} alone (a clip that needs no component labels)
__global__ __launch_bounds__(256) void k_cov_acc(const unsigned char* __restrict__ alive, const unsigned int* __restrict__ cov,
                                                 long long n, unsigned long long* __restrict__ acc) {
  __shared__ unsigned long long s_part[2][4];
  unsigned long long s_cov = 0, s_n = 0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    if (alive[i]) {
      s_cov += cov[i];
      s_n += 1;
    }
  for (int d = 32; d > 0; d >>= 1) {
    s_cov += __shfl_xor(s_cov, d, 64);
    s_n += __shfl_xor(s_n, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    s_part[0][threadIdx.x >> 6] = s_cov;
    s_part[1][threadIdx.x >> 6] = s_n;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long n_all = s_part[1][0] + s_part[1][1] + s_part[1][2] + s_part[1][3];
    if (n_all) {
      atomicAdd(&acc[0], s_part[0][0] + s_part[0][1] + s_part[0][2] + s_part[0][3]);
      atomicAdd(&acc[1], n_all);
    }
  }
}

__global__ void k_scatter_ids(const unsigned char* __restrict__ killed, const long long* __restrict__ pos,
                              long long n, int* __restrict__ out) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && killed[i]) out[pos[i]] = (int)i;
}

// kill[] (s0) -> node_alive, removal side effects, ascending list of removed ids
static int finish_kill(amg_ctx* c, int64_t* n_removed, int32_t* removed_ids) {
  hipStream_t st = c->stream;
  const long long D = c->n_nodes;
  AMGCHK(c->s2.ensure((size_t)(D + 2) * sizeof(long long)));
  // the scan applies what it counts: a marked live node dies, kill[] is left as "removed by this call"
  AMGCHK(prim_exscan_apply_kill(c, c->s0.as<unsigned char>(), c->node_alive.as<unsigned char>(), c->s2.as<long long>(),
                                (size_t)D));
  long long total = 0;
  {
    FetchList l;
    l.add(c->s2.as<long long>() + D);
    AMGCHK(fetch(c, l, reinterpret_cast<unsigned long long*>(&total)));
  }
  if (n_removed) *n_removed = total;
  if (removed_ids && total > 0) {
    AMGCHK(c->s3.ensure((size_t)total * sizeof(int)));
    hipLaunchKernelGGL(k_scatter_ids, dim3(nblk(D, 256)), dim3(256), 0, st, c->s0.as<unsigned char>(),
                       c->s2.as<long long>(), D, c->s3.as<int>());
    HIPCHK(hipMemcpyAsync(removed_ids, c->s3.p, (size_t)total * sizeof(int), hipMemcpyDeviceToHost, st));
  }
  if (total > 0) AMGCHK(apply_removals(c, 0));
  if (removed_ids && total > 0) HIPCHK(hipStreamSynchronize(st));  // (nothing else here is read by the host)
  return AMG_OK;
}

extern "C" int amg_remove_short_linear_paths(amg_ctx* c, int32_t min_length, const uint8_t* protect,
                                             int64_t* n_removed, int32_t* removed_ids) {
  NEED_BUILT(c);
  if (min_length < 1 || min_length > CLIP_MAX)
    return amg_fail(AMG_E_ARG, "min_length must be in [1, %d]", CLIP_MAX);
  hipStream_t st = c->stream;
  const long long D = c->n_nodes;
  if (n_removed) *n_removed = 0;
  if (D == 0) return AMG_OK;
  stages_reset(c);
  // "a tip that is its whole component is kept" (:710-713) compares the path with the LIVE nodes of its component as
  // labelled at build time.  While nothing has been removed since the build that is the question whether a live edge
  // leaves the path, which the walk's own rows answer: no labels are made for the clip of a freshly built graph
  // (the cleaning sweep's case; AMG_CLIP_COMPONENTS=1: A/B + test switch)
  const bool by_labels = !c->pristine || getenv("AMG_CLIP_COMPONENTS");
  if (by_labels) AMGCHK(ensure_components(c));
  // Live lists that exist, or that k_lr_patch brings up to date (inside bubble popping, after a re-threading
  // correction), are walked as they are.  Where there are none — the cleaning sweep's clip of a graph just built,
  // followed by a correction that re-threads nothing and reads no lists either — the walk goes over the row summary
  // of one pass over the edges (k_row_tickets; AMG_CLIP_LISTS=1 makes the lists as before: A/B + test switch).  The
  // summary lives in ladj_rows while the lists are neither valid nor stale, and leaves both flags as they are:
  // whoever needs lists next makes them from the edges, never by patching rows that are not lists.
  const bool light = !c->ladj_valid && !c->ladj_stale && !getenv("AMG_CLIP_LISTS");
  const long long rows = 2 * D;
  if (light) AMGCHK(c->ladj_rows.ensure((size_t)(rows + 2) * sizeof(int4)));
  stage_begin(c, "clip");
  // live nodes per component, and the mean node coverage's two integers (:868-871), in one pass
  unsigned long long* acc = c->status.as<unsigned long long>() + ST_COV_SUM;  // (the live adjacency below uses ST_COMPACT_*)
  AMGCHK(c->s0.ensure((size_t)D + 8));
  if (by_labels) AMGCHK(c->s4.ensure((size_t)(c->n_components + 2) * sizeof(unsigned int)));
  {
    ClearList cl;
    cl.add(acc, 2 * sizeof(unsigned long long));
    cl.add(c->s0.p, (size_t)D + 8);
    if (by_labels) cl.add(c->s4.p, (size_t)(c->n_components + 2) * sizeof(unsigned int));
    if (light) cl.add(c->ladj_rows.p, (size_t)(rows + 2) * sizeof(int4));
    AMGCHK(clear_many(c, cl));
  }
  if (light && c->n_edges > 0)
    hipLaunchKernelGGL(k_row_tickets, dim3(nblk(c->n_edges, 256)), dim3(256), 0, st, c->edge_alive.as<unsigned char>(),
                       c->edge_src.as<int>(), c->edge_sdir.as<signed char>(), c->n_edges, c->ladj_rows.as<int4>());
  if (by_labels)
    hipLaunchKernelGGL(k_comp_hist, dim3(nblk(D, 256) < 256u ? nblk(D, 256) : 256u), dim3(256), 0, st, c->node_comp.as<int>(),
                       c->node_alive.as<unsigned char>(), c->node_cov.as<unsigned int>(), D, 0u,
                       c->s4.as<unsigned int>(), (unsigned int*)nullptr, acc);
  else
    hipLaunchKernelGGL(k_cov_acc, dim3(nblk(D, 2048) < 256u ? nblk(D, 2048) : 256u), dim3(256), 0, st,
                       c->node_alive.as<unsigned char>(), c->node_cov.as<unsigned int>(), D, acc);
  unsigned char* d_protect = nullptr;
  if (protect) {
    AMGCHK(c->s5.ensure((size_t)D + 8));
    HIPCHK(hipMemcpyAsync(c->s5.p, protect, (size_t)D, hipMemcpyHostToDevice, st));
    d_protect = c->s5.as<unsigned char>();
  }
  const unsigned int* comp_live = by_labels ? c->s4.as<unsigned int>() : nullptr;
  if (light) {
    RView v;
    v.rows = c->ladj_rows.as<int4>();
    v.e_tgt = c->edge_tgt.as<int>();
    v.e_tdir = c->edge_tdir.as<signed char>();
    v.n_alive = c->node_alive.as<unsigned char>();
    v.n_cov = c->node_cov.as<unsigned int>();
    v.n_first = c->node_first.as<long long>();
    v.n_comp = c->node_comp.as<int>();
    hipLaunchKernelGGL(k_clip_mark<RView>, dim3(nblk(D, 128)), dim3(128), 0, st, v, D, (int)min_length, acc, comp_live,
                       d_protect, c->s0.as<unsigned char>());
  } else {
    AMGCHK(ensure_live_adj(c));
    hipLaunchKernelGGL(k_clip_mark<GView>, dim3(nblk(D, 128)), dim3(128), 0, st, make_view(c), D, (int)min_length, acc,
                       comp_live, d_protect, c->s0.as<unsigned char>());
  }
  int r = finish_kill(c, n_removed, removed_ids);
  stage_end(c);
  c->have_corrected = false;
  return r;
}

// ------------------------------------------------------------------ remove_low_coverage_components (:950-958)
__global__ void k_kill_low_components(const int* __restrict__ comp, const unsigned char* __restrict__ alive,
                                      const unsigned int* __restrict__ high_cnt, long long n,
                                      unsigned char* __restrict__ kill) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && alive[i] && high_cnt[comp[i]] == 0) kill[i] = 1;
}

extern "C" int amg_remove_low_coverage_components(amg_ctx* c, uint32_t min_cov) {
  NEED_BUILT(c);
  hipStream_t st = c->stream;
  const long long D = c->n_nodes;
  if (D == 0) return AMG_OK;
  AMGCHK(ensure_components(c));
  size_t nc = (size_t)(c->n_components + 2);
  AMGCHK(c->s0.ensure((size_t)D + 8));
  AMGCHK(c->s4.ensure(2 * nc * sizeof(unsigned int)));
  {
    ClearList cl;
    cl.add(c->s0.p, (size_t)D + 8);
    cl.add(c->s4.p, 2 * nc * sizeof(unsigned int));
    AMGCHK(clear_many(c, cl));
  }
  unsigned int* live = c->s4.as<unsigned int>();
  unsigned int* high = live + nc;
  hipLaunchKernelGGL(k_comp_hist, dim3(nblk(D, 256) < 256u ? nblk(D, 256) : 256u), dim3(256), 0, st, c->node_comp.as<int>(),
                     c->node_alive.as<unsigned char>(), c->node_cov.as<unsigned int>(), D, min_cov, live, high,
                     (unsigned long long*)nullptr);
  hipLaunchKernelGGL(k_kill_low_components, dim3(nblk(D, 256)), dim3(256), 0, st, c->node_comp.as<int>(),
                     c->node_alive.as<unsigned char>(), high, D, c->s0.as<unsigned char>());
  c->have_corrected = false;
  return finish_kill(c, nullptr, nullptr);
}
