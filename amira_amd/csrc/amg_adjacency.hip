// amg_adjacency.hip — the two views of a built graph that are made on first use, whichever key scheme built it: the full
// forward / backward edge lists of every node (ensure_adjacency) and the component ids (ensure_components).  amg_finalize
// asks for both; a cleaning sweep asks for what it needs.  The lists of the LIVE edges, which the walkers read, are
// amg_live_rows.hip's; both units put a row's ids in order with amg_rows.h.
#include "amg_rows.h"

// ------------------------------------------------------------------ full adjacency lists
// adjacency rows: adj_row_of; edge ids ascending inside a row
__global__ void k_adj_keys(const int* __restrict__ e_src, const signed char* __restrict__ e_sdir,
                           long long n_edges, unsigned int* __restrict__ keys,
                           unsigned int* __restrict__ vals) {
  long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n_edges) return;
  keys[e] = adj_row_of(e_src[e], e_sdir[e]);
  vals[e] = (unsigned int)e;
}

// CSR offsets from the sorted row keys, no atomics: position i opens every row in
// (key[i - 1], key[i]]; the position after the last edge opens the remaining rows and n_rows
__global__ void k_row_offsets(const unsigned int* __restrict__ keys, long long n_edges, long long n_rows,
                              long long* __restrict__ off) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n_edges) return;
  const long long prev = i > 0 ? (long long)keys[i - 1] : -1;
  const long long cur = i < n_edges ? (long long)keys[i] : n_rows;
  for (long long r = prev + 1; r <= cur; ++r) off[r] = i;
}

// The same lists WITHOUT a sort, for graphs of up to a few million edges (every graph of a cleaning sweep after the first
// filter): a library radix sort is a dozen launches of ~5 us whatever it sorts.
//   k_adjc_ticket  every edge draws a ticket of its row (rows zeroed before): row sizes and a place inside the row
//   (scan)         row sizes -> CSR offsets
//   k_adjc_fill    every edge drops its id at offset + ticket (any order within the row)
//   k_adjc_rows    a thread per row puts the row's ids in ascending order (short_rows_in_order, amg_rows.h); rows longer
//                  than a wave are left to k_adjc_long (long_rows_in_order: hub nodes)
__global__ void k_adjc_ticket(const int* __restrict__ e_src, const signed char* __restrict__ e_sdir, long long n_edges,
                              unsigned int* __restrict__ cnt, unsigned int* __restrict__ tick) {
  long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n_edges) tick[e] = atomicAdd(&cnt[adj_row_of(e_src[e], e_sdir[e])], 1u);
}

__global__ void k_adjc_fill(const int* __restrict__ e_src, const signed char* __restrict__ e_sdir, long long n_edges,
                            const long long* __restrict__ off, const unsigned int* __restrict__ tick,
                            unsigned int* __restrict__ tmp) {
  long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n_edges) tmp[off[adj_row_of(e_src[e], e_sdir[e])] + tick[e]] = (unsigned int)e;
}

__global__ __launch_bounds__(256) void k_adjc_rows(const long long* __restrict__ off, long long n_rows,
                                                   const unsigned int* __restrict__ tmp, int* __restrict__ adj_edge,
                                                   unsigned int* __restrict__ long_rows, unsigned long long* n_long) {
  long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  long long o = 0;
  int cnt = 0;
  if (r < n_rows) {
    o = off[r];
    cnt = (int)(off[r + 1] - o);
  }
  short_rows_in_order(cnt > 0, (unsigned int)r, o, cnt, tmp, long_rows, n_long,
                      [&](unsigned int, long long ro, int, long long rank, unsigned int x) { adj_edge[ro + rank] = (int)x; });
}

__global__ __launch_bounds__(256) void k_adjc_long(const unsigned int* __restrict__ long_rows,
                                                   const unsigned long long* __restrict__ n_long,
                                                   const long long* __restrict__ off, const unsigned int* __restrict__ tmp,
                                                   int* __restrict__ adj_edge, unsigned int* hub_bits, long long hub_words) {
  __shared__ unsigned int s_wave[4];
  long_rows_in_order(
      long_rows, *n_long, [&](unsigned int r) { return RowSpan{off[r], (int)(off[r + 1] - off[r])}; }, tmp, hub_bits,
      hub_words, s_wave, [&](unsigned int, long long ro, int, long long rank, unsigned int x) { adj_edge[ro + rank] = (int)x; });
}

// ------------------------------------------------------------------ components
// Union-find with parent[x] <= x.  Only the hook (a root gets a smaller parent) is an atomic;
// every other access is a PLAIN load or store that the issuing XCD's L2 may serve stale.  That
// is safe: a node's parent only ever moves to another member of its set with a smaller id, a
// stale value is an older such ancestor, and a node that has been hooked never becomes a root
// again — so a walk over stale parents still ends at a member of the set, a hook attempted on a
// node that only LOOKED like a root fails and returns the truth, and a path-halving store can
// at worst undo some compression.  (With agent-scope loads and atomicMin halving every step was
// a fabric transaction: 0.8 ms for 6.3 M pairs.)
__global__ void k_uf_init(int* parent, long long n) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) parent[i] = (int)i;
}

// Node ids are first-seen ranks: nine edge classes in ten join ids n and n + 1, so a component is mostly a few long
// RUNS of consecutive ids.  The runs are linked before any union: starts[n] = 0 where a class (n - 1, n) exists, a
// prefix sum numbers the runs, every node's parent is its run's first node (a flat forest, parent <= self), and the
// union-find proper only sees the classes that do NOT join consecutive ids.  (One pass of hooks over all classes built
// long chains along those runs first and then halved them: 0.11 ms per call for 0.5 M classes, twice per cleaning sweep,
// and at W emulated ranks the merged graph's 0.5 M x W classes on every rank.)
__global__ void k_uf_links(const unsigned long long* __restrict__ pkey, long long n_pairs, unsigned int* __restrict__ starts) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_pairs) return;
  const unsigned long long key = pkey[i];
  const unsigned int a = (unsigned int)((key >> 32) & 0x7fffffffull), b = (unsigned int)(key & 0xffffffffull) - 1u;
  if (b == a + 1u) starts[b] = 0u;  // (both classes of such a pair, the two signs, store the same word)
}

__global__ void k_uf_run_starts(const unsigned int* __restrict__ starts, const long long* __restrict__ run_of, long long n,
                                int* __restrict__ run_start) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && starts[i]) run_start[run_of[i]] = (int)i;
}

__global__ void k_uf_init_runs(const unsigned int* __restrict__ starts, const long long* __restrict__ run_of,
                               const int* __restrict__ run_start, long long n, int* __restrict__ parent) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) parent[i] = run_start[run_of[i] + (long long)starts[i] - 1];  // (run_of = runs started BEFORE i)
}

__global__ void k_uf_union(const unsigned long long* __restrict__ pkey, long long n_pairs, int* parent) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_pairs) return;
  unsigned long long key = pkey[i];
  int a = (int)((key >> 32) & 0x7fffffffull);
  int b = (int)((key & 0xffffffffull) - 1ull);
  if (b == a + 1) return;  // linked as a run already (k_uf_links)
  while (true) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) break;
    if (a > b) { int t = a; a = b; b = t; }
    int old = atomicCAS(parent + b, b, a);  // hook the larger root under the smaller
    if (old == b) break;
    b = old;
  }
}

// root_copy: the roots once more, for the labelling that overwrites parent[] (was a copy launch of its own);
// is_root[n] = 0 closes the array for the scan
__global__ void k_uf_roots(int* parent, long long n, unsigned int* __restrict__ is_root, int* __restrict__ root_copy) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) is_root[n] = 0u;
  if (i >= n) return;
  int r = uf_find(parent, (int)i);
  parent[i] = r;  // only thread i writes entry i with its final root; roots keep parent==self
  root_copy[i] = r;
  is_root[i] = (r == (int)i) ? 1u : 0u;
}

// component id = 1 + rank of the component's smallest node id == DFS discovery order
__global__ void k_uf_label(const int* __restrict__ root, const long long* __restrict__ root_rank,
                           long long n, int* __restrict__ comp) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int r = root[i];
  // root[] entries of non-roots may still point at an intermediate ancestor written by
  // another thread's k_uf_roots; chase to the fixed point (roots satisfy root[r] == r)
  while (root[r] != r) r = root[r];
  comp[i] = (int)(root_rank[r] + 1);
}

// assign_component_ids (construct_graph.py:920-927) of the graph AS BUILT (all edge classes, whatever was
// removed since: the reference labels once, in __init__)
int ensure_components(amg_ctx* c) {
  if (c->comp_valid) return AMG_OK;
  if (c->comp_from_claims) return bx_components_from_claims(c);  // a filtered build: the UNFILTERED graph's labels
  hipStream_t st = c->stream;
  const long long P = c->n_pairs, D = c->n_nodes;
  stage_begin(c, "components");
  AMGCHK(c->node_comp.ensure((size_t)(D + 1) * sizeof(int)));
  int* parent = c->node_comp.as<int>();  // holds roots until k_uf_label rewrites it
  AMGCHK(c->s1.ensure((size_t)(D + 2) * sizeof(long long)));  // root ranks
  AMGCHK(c->s2.ensure((size_t)(D + 2) * sizeof(unsigned int) + (size_t)(D + 2) * sizeof(int)));
  unsigned int* is_root = c->s2.as<unsigned int>();
  int* root_copy = reinterpret_cast<int*>(is_root + (D + 2));
  long long ncomp = 0;
  if (D > 0) {
    if (P > 0) {
      // runs of consecutive ids first (k_uf_links), the other classes through the union-find
      AMGCHK(c->s3.ensure((size_t)(D + 2) * sizeof(unsigned int)));
      AMGCHK(c->s4.ensure((size_t)(D + 2) * sizeof(int)));
      AMGCHK(c->s5.ensure((size_t)(D + 2) * sizeof(long long)));
      unsigned int* starts = c->s3.as<unsigned int>();
      int* run_start = c->s4.as<int>();
      long long* run_of = c->s5.as<long long>();
      ClearList cl;
      cl.add(starts, (size_t)D * sizeof(unsigned int), 1u);
      AMGCHK(clear_many(c, cl));
      hipLaunchKernelGGL(k_uf_links, dim3(nblk(P, 256)), dim3(256), 0, st, c->pair_key.as<unsigned long long>(), P, starts);
      AMGCHK(prim_exscan_u32_to_i64(c, starts, run_of, (size_t)D));
      hipLaunchKernelGGL(k_uf_run_starts, dim3(nblk(D, 256)), dim3(256), 0, st, starts, run_of, D, run_start);
      hipLaunchKernelGGL(k_uf_init_runs, dim3(nblk(D, 256)), dim3(256), 0, st, starts, run_of, run_start, D, parent);
      hipLaunchKernelGGL(k_uf_union, dim3(nblk(P, 256)), dim3(256), 0, st,
                         c->pair_key.as<unsigned long long>(), P, parent);
    } else {
      hipLaunchKernelGGL(k_uf_init, dim3(nblk(D, 256)), dim3(256), 0, st, parent, D);
    }
    hipLaunchKernelGGL(k_uf_roots, dim3(nblk(D, 256)), dim3(256), 0, st, parent, D, is_root, root_copy);
    AMGCHK(prim_exscan_u32_to_i64(c, is_root, c->s1.as<long long>(), (size_t)D + 1));
    hipLaunchKernelGGL(k_uf_label, dim3(nblk(D, 256)), dim3(256), 0, st, root_copy,
                       c->s1.as<long long>(), D, parent);
    FetchList l;
    l.add(c->s1.as<long long>() + D);
    AMGCHK(fetch(c, l, reinterpret_cast<unsigned long long*>(&ncomp)));
  }
  stage_end(c);
  c->n_components = ncomp;
  c->comp_valid = true;
  return AMG_OK;
}

// forwardEdgeHashes / backwardEdgeHashes of every node (construct_node.py:79-101): all edges ever
// inserted, in list order; removed edges stay listed (test `alive`)
int ensure_adjacency(amg_ctx* c) {
  if (c->adj_valid) return AMG_OK;
  hipStream_t st = c->stream;
  const long long D = c->n_nodes, E = c->n_edges;
  stage_begin(c, "adjacency");
  AMGCHK(c->adj_off.ensure((size_t)(2 * D + 2) * sizeof(long long)));
  AMGCHK(c->adj_edge.ensure((size_t)(E + 2) * sizeof(int)));
  AMGCHK(c->s1.ensure((size_t)(E + 2) * sizeof(unsigned int)));
  AMGCHK(c->s2.ensure((size_t)(E + 2) * sizeof(unsigned int)));
  AMGCHK(c->s3.ensure((size_t)(E + 2) * sizeof(unsigned int)));
  const char* force_sort = getenv("AMG_ADJ_SORT");  // A/B switch and test hook: the sorted route for every graph
  if (E > 0 && E <= (4ll << 20) && !(force_sort && force_sort[0] == '1')) {
    AMGCHK(c->s1.ensure((size_t)(2 * D + 2 > E + 2 ? 2 * D + 2 : E + 2) * sizeof(unsigned int)));
    unsigned int* cnt = c->s1.as<unsigned int>();
    unsigned int* tick = c->s2.as<unsigned int>();
    unsigned int* tmp = c->s3.as<unsigned int>();
    AMGCHK(c->s4.ensure((size_t)(E / WAVE_ROW_MAX + 2) * sizeof(unsigned int)));
    unsigned int* long_rows = c->s4.as<unsigned int>();
    unsigned long long* n_long = c->status.as<unsigned long long>() + ST_COMPACT_B;
    {
      ClearList cl;
      cl.add(cnt, (size_t)(2 * D + 2) * sizeof(unsigned int));
      cl.add(n_long, sizeof(unsigned long long));
      AMGCHK(clear_many(c, cl));
    }
    hipLaunchKernelGGL(k_adjc_ticket, dim3(nblk(E, 256)), dim3(256), 0, st, c->edge_src.as<int>(),
                       c->edge_sdir.as<signed char>(), E, cnt, tick);
    AMGCHK(prim_exscan_u32_to_i64(c, cnt, c->adj_off.as<long long>(), (size_t)(2 * D + 1)));
    hipLaunchKernelGGL(k_adjc_fill, dim3(nblk(E, 256)), dim3(256), 0, st, c->edge_src.as<int>(),
                       c->edge_sdir.as<signed char>(), E, c->adj_off.as<long long>(), tick, tmp);
    hipLaunchKernelGGL(k_adjc_rows, dim3(nblk(2 * D, 256)), dim3(256), 0, st, c->adj_off.as<long long>(), 2 * D, tmp,
                       c->adj_edge.as<int>(), long_rows, n_long);
    const long long hub_words = (E + 31) / 32 + 1;  // (scratch of the hub rows: HUB_BLOCKS bitmaps over the edge ids)
    AMGCHK(c->hub_bits.ensure((size_t)HUB_BLOCKS * (size_t)hub_words * sizeof(unsigned int)));
    hipLaunchKernelGGL(k_adjc_long, dim3(256), dim3(256), 0, st, long_rows, n_long, c->adj_off.as<long long>(), tmp,
                       c->adj_edge.as<int>(), c->hub_bits.as<unsigned int>(), hub_words);
    stage_end(c);
    c->adj_valid = true;
    return AMG_OK;
  }
  if (E > 0) {
    hipLaunchKernelGGL(k_adj_keys, dim3(nblk(E, 256)), dim3(256), 0, st,
                       c->edge_src.as<int>(), c->edge_sdir.as<signed char>(), E,
                       c->s1.as<unsigned int>(), c->s2.as<unsigned int>());
    AMGCHK(prim_sort_u32_u32(c, c->s1.as<unsigned int>(), c->s3.as<unsigned int>(),
                             c->s2.as<unsigned int>(),
                             reinterpret_cast<unsigned int*>(c->adj_edge.p), (size_t)E,
                             ilog2_ceil((uint64_t)2 * D + 2) + 1));
  }
  hipLaunchKernelGGL(k_row_offsets, dim3(nblk(E + 1, 256)), dim3(256), 0, st,
                     c->s3.as<unsigned int>(), E, 2 * D, c->adj_off.as<long long>());
  stage_end(c);
  c->adj_valid = true;
  return AMG_OK;
}
