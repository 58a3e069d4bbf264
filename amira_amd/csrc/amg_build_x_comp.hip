// amg_build_x_comp.hip — what only a build with the coverage filter applied on the way needs after its per-claim stage
// (amg_build_x_claims.hip): the component ids of the UNFILTERED graph, made from the claims, and the reads the filter
// touched.
#include "amg_slot16.h"

// ------------------------------------------------------------------ components of a filtered build
// The reference labels components once, in __init__, on the graph of ALL nodes (construct_graph.py:101-102,
// :911-927) and keeps the labels through filter_graph.  A filtered build never makes the nodes and edges
// below the threshold, so the labels are made in CLAIM space instead, from what the node pass left behind:
// every window's claim (tok_slot) — two consecutive windows of a read are an edge of the unfiltered graph —
// and every claim's first-seen value (saved by k_x_drop_claims).  Union-find over the claims; component id =
// 1 + rank of the component's earliest first-seen among the components (= DFS discovery order over _nodes).
__global__ void k_xc_init(int* parent, long long n) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) parent[i] = (int)i;
}

__global__ void k_xc_union(const int* __restrict__ tok_claim, long long n_tokens, int* parent) {
  long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t + 1 >= n_tokens) return;
  const int raw = tok_claim[t];
  if (raw == -1 || ((unsigned int)raw & AMG_LAST_FLAG)) return;
  const int nxt = tok_claim[t + 1];
  if (nxt == -1) return;
  int a = (int)((unsigned int)raw & ~AMG_FLAG_MASK), b = (int)((unsigned int)nxt & ~AMG_FLAG_MASK);
  while (true) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) break;
    if (a > b) { int x = a; a = b; b = x; }
    const int old = atomicCAS(parent + b, b, a);  // hook the larger root under the smaller
    if (old == b) break;
    b = old;
  }
}

__global__ void k_xc_flatten(int* parent, long long n) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) parent[i] = uf_find(parent, (int)i);  // only thread i writes entry i; roots keep parent == self
}

__device__ __forceinline__ int xc_root(const int* __restrict__ parent, long long c) {
  int r = parent[c];
  while (parent[r] != r) r = parent[r];  // entries of non-roots may still name an intermediate ancestor
  return r;
}

// best2[2 r] = the largest complemented first-seen (= the earliest) among the claims of root r; roots counted
__global__ void k_xc_best(const int* __restrict__ parent, const unsigned int* __restrict__ first_all, long long n,
                          unsigned int* __restrict__ best2, unsigned long long* __restrict__ n_roots) {
  long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  bool root = false;
  if (c < n && first_all[c] != 0u) {
    const int r = xc_root(parent, c);
    root = r == (int)c;
    atomicMax(best2 + 2ll * r, first_all[c]);
  }
  const unsigned long long m = __ballot(root);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(n_roots, (unsigned long long)__popcll(m));
}

__global__ void k_xc_label(const int* __restrict__ parent, const unsigned int* __restrict__ first_all, long long n,
                           const unsigned int* __restrict__ best2, const unsigned int* __restrict__ bits,
                           const long long* __restrict__ prefix, const int* __restrict__ final_of_claim,
                           int* __restrict__ node_comp) {
  long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n || first_all[c] == 0u) return;
  const int node = final_of_claim[c];
  if (node < 0) return;  // the filter dropped this node
  const unsigned int first = ~best2[2ll * xc_root(parent, c)];
  node_comp[node] = (int)x_rank_of(first >> 1, bits, prefix) + 1;
}

// component ids of a filtered build (see k_xc_*)
int bx_components_from_claims(amg_ctx* c) {
  hipStream_t st = c->stream;
  const long long S = c->x_nspace, T = c->n_tokens, D = c->n_nodes;
  stage_begin(c, "components");
  AMGCHK(c->node_comp.ensure((size_t)(D + 1) * sizeof(int)));
  AMGCHK(c->s3.ensure((size_t)(S + 2) * sizeof(int)));
  AMGCHK(c->s4.ensure((size_t)(2 * S + 4) * sizeof(unsigned int)));
  int* parent = c->s3.as<int>();
  unsigned int* best2 = c->s4.as<unsigned int>();
  unsigned long long* n_roots = c->status.as<unsigned long long>() + ST_COMPACT_A;
  long long ncomp = 0;
  if (S > 0) {
    ClearList cl;
    cl.add(best2, (size_t)(2 * S + 2) * sizeof(unsigned int));
    cl.add(n_roots, sizeof(unsigned long long));
    AMGCHK(clear_many(c, cl));
    hipLaunchKernelGGL(k_xc_init, dim3(nblk(S, 256)), dim3(256), 0, st, parent, S);
    if (T > 1)
      hipLaunchKernelGGL(k_xc_union, dim3(nblk(T, 256)), dim3(256), 0, st, c->tok_slot.as<int>(), T, parent);
    hipLaunchKernelGGL(k_xc_flatten, dim3(nblk(S, 256)), dim3(256), 0, st, parent, S);
    hipLaunchKernelGGL(k_xc_best, dim3(nblk(S, 256)), dim3(256), 0, st, parent, c->x_first_all.as<unsigned int>(), S,
                       best2, n_roots);
    RankBitmap r;
    AMGCHK(rank_first_seen(c, best2, S, 1, RankFlagsZeroed{}, &r));  // non-roots keep {0, 0}: skipped like unclaimed ids
    hipLaunchKernelGGL(k_xc_label, dim3(nblk(S, 256)), dim3(256), 0, st, parent, c->x_first_all.as<unsigned int>(), S,
                       best2, r.bits, r.prefix, c->x_final.as<int>(), c->node_comp.as<int>());
    FetchList l;
    l.add(n_roots);
    AMGCHK(fetch(c, l, reinterpret_cast<unsigned long long*>(&ncomp)));
  }
  stage_end(c);
  c->n_components = ncomp;
  c->comp_valid = true;
  return AMG_OK;
}

// ------------------------------------------------------------------ reads the filter touched
// reads that lost a window to the filter join _readsToCorrect (remove_node_from_reads :442-461).  Sixteen lanes per
// read, four loads per lane in flight: a wave per read kept ONE 240-byte load in flight and ran at 1.2 TB/s.
#define FD_READS 16  // reads per 256-thread workgroup
__global__ __launch_bounds__(256) void k_x_flag_dead_reads(const int* __restrict__ tok_node,
                                                            const long long* __restrict__ read_off, long long n_reads,
                                                            unsigned char* __restrict__ read_fix) {
  const int lane = threadIdx.x & 63, sub = lane & 15, grp = lane >> 4;
  const long long r = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 4 + grp;
  const bool have = r < n_reads;
  const long long a = have ? read_off[r] : 0, b = have ? read_off[r + 1] : 0;
  int v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = a + sub + 16 * j < b ? tok_node[a + sub + 16 * j] : 0;
  bool hit = v[0] == -2 || v[1] == -2 || v[2] == -2 || v[3] == -2;
  for (long long t = a + 64 + sub; t < b; t += 16) hit = hit || (tok_node[t] == -2);  // reads longer than 64 genes
  const unsigned long long m = __ballot(hit);
  if (have && sub == 0 && ((m >> (grp * 16)) & 0xffffull)) read_fix[r] = 1;
}

// after bs_finish_from_pairs of a filtered build (single GPU or merged): the reads the filter touched
int bx_flag_dead_reads(amg_ctx* c) {
  if (c->n_reads > 0)
    hipLaunchKernelGGL(k_x_flag_dead_reads, dim3(nblk(c->n_reads, FD_READS)), dim3(256), 0, c->stream,
                       c->tok_node.as<int>(), c->read_off.as<long long>(), c->n_reads, c->read_fix.as<unsigned char>());
  return AMG_OK;
}
