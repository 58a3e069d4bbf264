// amg_filter.hip — what removes nodes and edges from a built graph, on the device: the coverage filter, listed node /
// edge removals, tip clipping and the component filter (reference construct_graph.py:402-540, 679-861, 950-958).  The
// live adjacency the tip walk reads, its state and the walk's row summary are amg_live_rows.hip's.
#include "amg_rows.h"

// ------------------------------------------------------------------ filter_graph (:523-540)
// list_nodes_to_remove (:496-503): coverage < minNodeCoverage
// Four nodes a thread, k_filter_edges' form below (the node arrays are allocations of their own): the alive bytes arrive
// as one word, the coverages as 16 bytes, the four bytes leave as one word where one of them changed; a quad with
// nothing alive returns after the first load, the last n mod 4 nodes take the scalar form.
__global__ __launch_bounds__(256) void k_filter_nodes(const unsigned int* __restrict__ cov, unsigned char* __restrict__ alive,
                                                      long long n, unsigned int min_cov) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long i0 = 4 * q;
  if (i0 >= n) return;
  if (i0 + 4 > n) {
    for (long long i = i0; i < n; ++i)
      if (alive[i] && cov[i] < min_cov) alive[i] = 0;
    return;
  }
  const unsigned int a = reinterpret_cast<const unsigned int*>(alive)[q];
  if (a == 0u) return;
  const uint4 c = reinterpret_cast<const uint4*>(cov)[q];
  unsigned int keep = 0u;
  if (c.x >= min_cov) keep |= 0x000000ffu;
  if (c.y >= min_cov) keep |= 0x0000ff00u;
  if (c.z >= min_cov) keep |= 0x00ff0000u;
  if (c.w >= min_cov) keep |= 0xff000000u;
  if ((a & keep) != a) reinterpret_cast<unsigned int*>(alive)[q] = a & keep;
}

// list_edges_to_remove (:505-521): coverage < minEdgeCoverage or a doomed endpoint
// (an edge's coverage is at least 1: with the usual threshold of 1 the coverage array is not read at all)
__device__ __forceinline__ void filter_edge(const int* __restrict__ src, const int* __restrict__ tgt,
                                            const unsigned int* __restrict__ cov,
                                            const unsigned char* __restrict__ node_alive,
                                            unsigned char* __restrict__ alive, long long e, unsigned int min_cov) {
  if (!alive[e]) return;
  if ((min_cov > 1 && cov[e] < min_cov) || !node_alive[src[e]] || !node_alive[tgt[e]]) alive[e] = 0;
}

// Four edges a thread (the edge arrays are allocations of their own, so edge 4 q is aligned for the wide loads): the
// alive bytes arrive as one word, src and tgt as 16 bytes each, the eight node bytes are asked for together and the four
// alive bytes leave as one word (a byte that was 0 stays 0).  The last n mod 4 edges take the scalar form.  One edge per
// thread waited through alive -> src, tgt -> two node bytes -> store four times as often per byte moved.
__global__ __launch_bounds__(256) void k_filter_edges(const int* __restrict__ src, const int* __restrict__ tgt,
                                                      const unsigned int* __restrict__ cov,
                                                      const unsigned char* __restrict__ node_alive,
                                                      unsigned char* __restrict__ alive, long long n, unsigned int min_cov) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long e0 = 4 * q;
  if (e0 >= n) return;
  if (e0 + 4 > n) {
    for (long long e = e0; e < n; ++e) filter_edge(src, tgt, cov, node_alive, alive, e, min_cov);
    return;
  }
  const unsigned int a = reinterpret_cast<const unsigned int*>(alive)[q];
  if (a == 0u) return;  // (nothing of the four is left to remove)
  const int4 s = reinterpret_cast<const int4*>(src)[q];
  const int4 t = reinterpret_cast<const int4*>(tgt)[q];
  uint4 c = make_uint4(min_cov, min_cov, min_cov, min_cov);
  if (min_cov > 1) c = reinterpret_cast<const uint4*>(cov)[q];
  // (no load is under a test of its own: the ends of an edge that is dead already are not looked at, node 0 stands in)
  const bool l0 = a & 0x000000ffu, l1 = a & 0x0000ff00u, l2 = a & 0x00ff0000u, l3 = a & 0xff000000u;
  const unsigned int ns0 = node_alive[l0 ? s.x : 0], ns1 = node_alive[l1 ? s.y : 0], ns2 = node_alive[l2 ? s.z : 0],
                     ns3 = node_alive[l3 ? s.w : 0];
  const unsigned int nt0 = node_alive[l0 ? t.x : 0], nt1 = node_alive[l1 ? t.y : 0], nt2 = node_alive[l2 ? t.z : 0],
                     nt3 = node_alive[l3 ? t.w : 0];
  unsigned int keep = 0u;
  if (ns0 && nt0 && c.x >= min_cov) keep |= 0x000000ffu;
  if (ns1 && nt1 && c.y >= min_cov) keep |= 0x0000ff00u;
  if (ns2 && nt2 && c.z >= min_cov) keep |= 0x00ff0000u;
  if (ns3 && nt3 && c.w >= min_cov) keep |= 0xff000000u;
  if ((a & keep) != a) reinterpret_cast<unsigned int*>(alive)[q] = a & keep;
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
                                                    unsigned char* __restrict__ read_fix,
                                                    unsigned long long* __restrict__ win_mask) {
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
  // The live windows 0..63 of every read walked, flagged now or by an earlier removal or not at all, as tok_node reads
  // once this kernel is through (WindowMasks: k_corr_classify takes them instead of loading the windows again); tokens
  // past a read's last window hold -1.  Lane j keeps read j's mask: one 64-byte store per wave.
  unsigned long long mine = 0;
#pragma unroll
  for (int j = 0; j < READS_PER_WAVE; ++j) {
    const unsigned long long m = __ballot(v[j] >= 0 && !dead[j]);
    if (lane == j) mine = m;
  }
  if (lane < READS_PER_WAVE && rbase + lane < n_reads) win_mask[rbase + lane] = mine;
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
  if (min_edge_cov > 1) live_lists_after_edge_deaths(c);  // (an edge may fall to its own coverage)
  else live_lists_after_node_deaths(c);
  if (c->n_edges > 0)
    hipLaunchKernelGGL(k_filter_edges, dim3(nblk(c->n_edges, 4 * 256)), dim3(256), 0, st,
                       c->edge_src.as<int>(), c->edge_tgt.as<int>(), c->edge_cov.as<unsigned int>(),
                       c->node_alive.as<unsigned char>(), c->edge_alive.as<unsigned char>(),
                       c->n_edges, min_edge_cov);
  AMGCHK(c->win_mask.ensure((size_t)(c->n_reads + 2) * sizeof(unsigned long long)));
  if (c->n_reads > 0)
    hipLaunchKernelGGL(k_mask_reads, dim3(nblk(c->n_reads, 4 * READS_PER_WAVE)), dim3(256), 0, st,
                       c->tok_node.as<int>(), c->read_off.as<long long>(), c->n_reads,
                       c->node_alive.as<unsigned char>(), c->read_fix.as<unsigned char>(),
                       c->win_mask.as<unsigned long long>());
  window_masks_made(c);  // (every read was walked: a read flagged by an earlier removal has its mask of now)
  return AMG_OK;
}

extern "C" int amg_filter(amg_ctx* c, uint32_t min_node_cov, uint32_t min_edge_cov) {
  NEED_BUILT(c);
  ctx_removal_begins(c);
  stages_reset(c);
  stage_begin(c, "filter");
  if (c->n_nodes > 0)
    hipLaunchKernelGGL(k_filter_nodes, dim3(nblk(c->n_nodes, 4 * 256)), dim3(256), 0, c->stream,
                       c->node_cov.as<unsigned int>(), c->node_alive.as<unsigned char>(),
                       c->n_nodes, min_node_cov);
  AMGCHK(apply_removals(c, min_edge_cov));
  stage_end(c);
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
  ctx_removal_begins(c);
  AMGCHK(c->s0.ensure((size_t)n * sizeof(int)));
  HIPCHK(hipMemcpyAsync(c->s0.p, node_ids, (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_kill_listed, dim3(nblk(n, 256)), dim3(256), 0, c->stream, c->s0.as<int>(),
                     (long long)n, c->n_nodes, c->node_alive.as<unsigned char>());
  AMGCHK(apply_removals(c, 0));
  HIPCHK(hipStreamSynchronize(c->stream));
  return AMG_OK;
}

// ------------------------------------------------------------------ remove_edge (:409-428)
// one DIRECTED edge per listed id leaves the graph (and its source node's forward / backward list); its reverse
// twin stays, as in the reference, until it is removed by its own call
extern "C" int amg_remove_edges(amg_ctx* c, const int32_t* edge_ids, int64_t n) {
  NEED_BUILT(c);
  if (n < 0 || (n > 0 && !edge_ids)) return amg_fail(AMG_E_ARG, "bad edge list");
  if (n == 0) return AMG_OK;
  ctx_removal_begins(c);
  AMGCHK(c->s0.ensure((size_t)n * sizeof(int)));
  HIPCHK(hipMemcpyAsync(c->s0.p, edge_ids, (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_kill_listed, dim3(nblk(n, 256)), dim3(256), 0, c->stream, c->s0.as<int>(), (long long)n,
                     c->n_edges, c->edge_alive.as<unsigned char>());
  live_lists_after_edge_deaths(c);
  HIPCHK(hipStreamSynchronize(c->stream));
  return AMG_OK;
}

// ------------------------------------------------------------------ remove_short_linear_paths (:679-720)
#define CLIP_MAX 64
// acc = {sum of the live nodes' coverages, number of live nodes} (k_comp_hist): the threshold is 1.5 x their mean
// (:868-871, statistics.mean over live nodes) — the quotient of the two integers as doubles is correctly rounded,
// == float(Fraction(sum, n)), on the device as on the host
// View: the live lists (GView) or the row summary (RView) — one walk, two ways to read a row (amg_rows.h)
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

// acc += {sum, n} over a workgroup of 256 (every thread calls): one pair of atomics per WORKGROUP (a pair per wave: two
// thousand atomics on one line, ~15 us), none from a workgroup without a live node
__device__ __forceinline__ void block_add_cov(unsigned long long sum, unsigned long long n, unsigned long long* __restrict__ acc) {
  __shared__ unsigned long long s_part[2][4];
  for (int d = 32; d > 0; d >>= 1) {
    sum += __shfl_xor(sum, d, 64);
    n += __shfl_xor(n, d, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    s_part[0][threadIdx.x >> 6] = sum;
    s_part[1][threadIdx.x >> 6] = n;
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
  if (acc) block_add_cov(s_cov, s_n, acc);  // (block-uniform)
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
  unsigned long long s_cov = 0, s_n = 0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    if (alive[i]) {
      s_cov += cov[i];
      s_n += 1;
    }
  block_add_cov(s_cov, s_n, acc);
}

__global__ void k_scatter_ids(const unsigned char* __restrict__ killed, const long long* __restrict__ pos,
                              long long n, int* __restrict__ out) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && killed[i]) out[pos[i]] = (int)i;
}

int kill_marks_reserve(amg_ctx* c, ClearList* cl, KillMarks* marks) {
  const long long D = c->n_nodes;
  AMGCHK(c->s0.ensure((size_t)D + 8));
  cl->add(c->s0.p, (size_t)D + 8);
  *marks = KillMarks{c->s0.as<unsigned char>(), D};
  return AMG_OK;
}

int kill_marks_check(const amg_ctx* c, const KillMarks& marks) {
  if (!marks.bytes || marks.bytes != c->s0.p || marks.n != c->n_nodes)
    return amg_fail(AMG_E_STATE, "the kill marks (%lld nodes) are not the ctx's current ones (%lld nodes): something else "
                                 "ran on the ctx between their reservation and their use",
                    marks.n, (long long)c->n_nodes);
  return AMG_OK;
}

// marks -> node_alive, removal side effects, ascending list of removed ids
int finish_kill(amg_ctx* c, const KillMarks& marks, int64_t* n_removed, int32_t* removed_ids) {
  hipStream_t st = c->stream;
  const long long D = c->n_nodes;
  AMGCHK(kill_marks_check(c, marks));
  AMGCHK(c->s2.ensure((size_t)(D + 2) * sizeof(long long)));
  // the scan applies what it counts: a marked live node dies, the marks are left as "removed by this call"
  AMGCHK(prim_exscan_apply_kill(c, marks.bytes, c->node_alive.as<unsigned char>(), c->s2.as<long long>(), (size_t)D));
  long long total = 0;
  {
    FetchList l;
    l.add(c->s2.as<long long>() + D);
    AMGCHK(fetch(c, l, reinterpret_cast<unsigned long long*>(&total)));
  }
  if (n_removed) *n_removed = total;
  if (removed_ids && total > 0) {
    AMGCHK(c->s3.ensure((size_t)total * sizeof(int)));
    hipLaunchKernelGGL(k_scatter_ids, dim3(nblk(D, 256)), dim3(256), 0, st, marks.bytes, c->s2.as<long long>(), D,
                       c->s3.as<int>());
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
  ctx_removal_begins(c);
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
  // of one pass over the edges (row_summary, amg_live_rows.hip; AMG_CLIP_LISTS=1 makes the lists as before: A/B + test
  // switch).
  const bool light = c->live_lists == LiveLists::Absent && !getenv("AMG_CLIP_LISTS");
  stage_begin(c, "clip");
  // live nodes per component, and the mean node coverage's two integers (:868-871), in one pass
  unsigned long long* acc = c->status.as<unsigned long long>() + ST_COV_SUM;  // (the live adjacency below uses ST_COMPACT_*)
  KillMarks marks;
  {
    ClearList cl;
    cl.add(acc, 2 * sizeof(unsigned long long));
    AMGCHK(kill_marks_reserve(c, &cl, &marks));
    if (by_labels) {
      AMGCHK(c->s4.ensure((size_t)(c->n_components + 2) * sizeof(unsigned int)));
      cl.add(c->s4.p, (size_t)(c->n_components + 2) * sizeof(unsigned int));
    }
    if (light) AMGCHK(row_summary_reserve(c, &cl));  // (its rows are zeroed with the rest)
    AMGCHK(clear_many(c, cl));
  }
  RView summary;
  if (light) summary = row_summary(c);
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
    hipLaunchKernelGGL(k_clip_mark<RView>, dim3(nblk(D, 128)), dim3(128), 0, st, summary, D, (int)min_length, acc, comp_live,
                       d_protect, marks.bytes);
  } else {
    AMGCHK(ensure_live_adj(c));
    hipLaunchKernelGGL(k_clip_mark<GView>, dim3(nblk(D, 128)), dim3(128), 0, st, make_view(c), D, (int)min_length, acc,
                       comp_live, d_protect, marks.bytes);
  }
  int r = finish_kill(c, marks, n_removed, removed_ids);
  stage_end(c);
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
  ctx_removal_begins(c);
  AMGCHK(ensure_components(c));
  size_t nc = (size_t)(c->n_components + 2);
  KillMarks marks;
  {
    ClearList cl;
    AMGCHK(kill_marks_reserve(c, &cl, &marks));
    AMGCHK(c->s4.ensure(2 * nc * sizeof(unsigned int)));
    cl.add(c->s4.p, 2 * nc * sizeof(unsigned int));
    AMGCHK(clear_many(c, cl));
  }
  unsigned int* live = c->s4.as<unsigned int>();
  unsigned int* high = live + nc;
  hipLaunchKernelGGL(k_comp_hist, dim3(nblk(D, 256) < 256u ? nblk(D, 256) : 256u), dim3(256), 0, st, c->node_comp.as<int>(),
                     c->node_alive.as<unsigned char>(), c->node_cov.as<unsigned int>(), D, min_cov, live, high,
                     (unsigned long long*)nullptr);
  hipLaunchKernelGGL(k_kill_low_components, dim3(nblk(D, 256)), dim3(256), 0, st, c->node_comp.as<int>(),
                     c->node_alive.as<unsigned char>(), high, D, marks.bytes);
  return finish_kill(c, marks, nullptr, nullptr);
}
