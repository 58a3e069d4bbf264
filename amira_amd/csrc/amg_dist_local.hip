// amg_dist_local.hip — key-owner merge (amg_dist.hip), phase local: the shard's tables -> records by destination.
#include "amg_dist.h"

// destination of every local node (compaction list: first / slot) — fingerprint path
__global__ void k_dist_dest(const unsigned int* __restrict__ slots, long long n, const Slot* __restrict__ tab,
                            unsigned int world, unsigned int* __restrict__ dest, unsigned int* __restrict__ idx) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  dest[i] = owner_of(tab[slots[i]].key, world);
  idx[i] = (unsigned int)i;
}

// counts[d] = number of entries equal to d in the ascending array dest_sorted[0..n)
__global__ void k_dest_counts(const unsigned int* __restrict__ dest_sorted, long long n, unsigned int world,
                              unsigned long long* __restrict__ counts) {
  unsigned int d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= world) return;
  auto lower = [&](unsigned int v) {
    long long lo = 0, hi = n;
    while (lo < hi) {
      long long mid = (lo + hi) >> 1;
      if (dest_sorted[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
  };
  counts[d] = (unsigned long long)(lower(d + 1) - lower(d));
}

// the count message of a phase, one CNT_WORDS block per peer.  code != 0: this rank's phase failed on the host;
// otherwise the device's own status words are looked at (a reply nobody answers, a tuple that is not its key's)
__global__ void k_cnt_msg(const unsigned long long* __restrict__ counts, long long single_count, int world,
                          long long n_tokens, int attempt, int kind, long long code,
                          const unsigned long long* __restrict__ status, long long* __restrict__ msg) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= world) return;
  if (code == 0 && status[ST_DIST_BAD]) code = CODE_ERROR;
  if (code == 0 && status[ST_COLLISION]) code = CODE_COLLISION;
  long long* m = msg + (size_t)p * CNT_WORDS;
  m[0] = code ? code : (counts ? (long long)counts[p] : single_count);
  m[1] = n_tokens;
  m[2] = attempt;
  m[3] = kind;
}

void count_message(amg_ctx* c, DistState* d, int is_edge) {
  const int W = d->world;
  const long long code = !d->fail_ret ? 0 : (d->fail_ret == AMG_E_COLLISION ? CODE_COLLISION : CODE_ERROR);
  hipLaunchKernelGGL(k_cnt_msg, dim3(nblk(W, 64)), dim3(64), 0, c->stream,
                     (W > 1 && !d->fail_ret) ? d->loc_dest_cnt.as<unsigned long long>() : (const unsigned long long*)nullptr,
                     (long long)d->n_send, W, (long long)c->n_tokens, d->attempt, is_edge, code,
                     c->status.as<unsigned long long>(), d->cnt_send.as<long long>());
}

// fingerprint of a canonical tuple given as tokens: same value as canon_fingerprint()
__device__ __forceinline__ unsigned long long tuple_fingerprint(const int* tok, int k, unsigned long long seed) {
  unsigned long long h = seed;
  for (int j = 0; j < k; ++j) {
    h = (h ^ (unsigned long long)(unsigned int)tok[j]) * 0x9E3779B97F4A7C15ull;
    h ^= h >> 29;
  }
  h = mix64(h);
  return h ? h : 1ull;
}

// exact-key shards: merge key and destination per claim
// (claim ids nobody took — shard counters leave holes — have first-seen 0: they get destination `world`, which sorts
// behind every rank and is never sent; `bucket`: destinations are wanted, i.e. world > 1 or there are holes)
__global__ void k_xd_node_keys(const Slot16* __restrict__ tab, const unsigned int* __restrict__ slot_by_claim,
                               const unsigned int* __restrict__ first2,
                               long long n, int k, int bits, int two, unsigned long long seed, unsigned long long key_mask,
                               unsigned int world, int bucket,
                               unsigned long long* __restrict__ keys, unsigned int* __restrict__ dest,
                               unsigned int* __restrict__ idx) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (x_first_inv(first2, i) == 0u) {
    keys[i] = 0ull;
    if (bucket) {
      dest[i] = world;
      idx[i] = (unsigned int)i;
    }
    return;
  }
  const Slot16 s = tab[slot_by_claim[i]];
  const unsigned int tag = x_tag_of(s, two);
  int tok[AMG_MAX_K];
  for (int j = 0; j < k; ++j) tok[j] = x_unpack(s.w1, tag, bits, j);
  unsigned long long key = tuple_fingerprint(tok, k, seed);  // (the same value as the fingerprint shards' slot keys)
  if (key_mask != ~0ull) key = (key & key_mask) | 1ull;      // test hook, see nodes_local
  keys[i] = key;
  if (bucket) {
    dest[i] = world > 1 ? owner_of(key, world) : 0u;
    idx[i] = (unsigned int)i;
  }
}

__global__ void k_xd_edge_dest(const Slot16* __restrict__ etab, const unsigned int* __restrict__ slot_by_claim,
                               const unsigned int* __restrict__ first2, long long n, unsigned int world,
                               unsigned int* __restrict__ dest, unsigned int* __restrict__ idx) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  dest[i] = x_first_inv(first2, i) == 0u ? world : (world > 1 ? owner_of(etab[slot_by_claim[i]].w1, world) : 0u);
  idx[i] = (unsigned int)i;
}

// records in destination order.  order == nullptr: local order (one destination and no unclaimed ids in between)
// exact-key shards: key per claim from `keys` (nodes) or the class slot (edges), first-seen = base + local value
__global__ void k_xd_pack(const unsigned int* __restrict__ order, long long n, const unsigned long long* __restrict__ keys,
                          const Slot16* __restrict__ etab, const unsigned int* __restrict__ slot_by_claim,
                          const unsigned int* __restrict__ first2, unsigned long long base,
                          const unsigned int* __restrict__ lcnt, unsigned long long* __restrict__ out) {
  long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const unsigned int c = order ? order[j] : (unsigned int)j;
  unsigned long long* q = out + 3 * j;
  q[0] = keys ? keys[c] : etab[slot_by_claim[c]].w1;
  q[1] = base + (unsigned long long)(unsigned int)~x_first_inv(first2, c);
  q[2] = (unsigned long long)lcnt[c];
}

// fingerprint shards: the compaction list (firsts / slots) in destination order
__global__ void k_fd_pack(const unsigned int* __restrict__ order, long long n, const unsigned int* __restrict__ slots,
                          const unsigned long long* __restrict__ firsts, unsigned long long base,
                          const Slot* __restrict__ tab, const unsigned int* __restrict__ lcnt,
                          unsigned long long* __restrict__ out) {
  long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const unsigned int i = order ? order[j] : (unsigned int)j;
  const Slot* s = tab + slots[i];
  unsigned long long* q = out + 3 * j;
  q[0] = s->key;
  q[1] = firsts[i] + base;
  q[2] = (unsigned long long)lcnt[s->id];  // s->id is still the LOCAL first-seen rank here
}

void pack_records(amg_ctx* c, DistState* d, int is_edge) {
  if (d->n_send <= 0) return;
  const long long n = d->n_send;
  const unsigned int* order = send_order(d);
  const unsigned long long base = (unsigned long long)c->tok_base << (is_edge ? 3 : 1);
  if (c->dist_x)
    hipLaunchKernelGGL(k_xd_pack, dim3(nblk(n, 256)), dim3(256), 0, c->stream, order, n,
                       is_edge ? (const unsigned long long*)nullptr : d->loc_first.as<unsigned long long>(),
                       c->edge_tab.as<Slot16>(), c->x_eslot.as<unsigned int>(),
                       is_edge ? c->x_efirst.as<unsigned int>() : c->x_first.as<unsigned int>(), base,
                       d->loc_cnt.as<unsigned int>(), d->send.as<unsigned long long>());
  else
    hipLaunchKernelGGL(k_fd_pack, dim3(nblk(n, 256)), dim3(256), 0, c->stream, order, n,
                       d->loc_slot.as<unsigned int>(), d->loc_first.as<unsigned long long>(),
                       is_edge ? 0ull : base, is_edge ? c->edge_tab.as<Slot>() : c->node_tab.as<Slot>(),
                       d->loc_cnt.as<unsigned int>(), d->send.as<unsigned long long>());
}

// the four arrays of a bucketing (n + 1 words each) inside d->loc_bucket
struct Bucketing {
  unsigned int *dest, *idx, *dest_sorted, *order;
};
static int bucketing(DistState* d, long long n, Bucketing* b) {
  AMGCHK(d->loc_bucket.ensure((size_t)(n + 1) * sizeof(unsigned int) * 4 + 64));
  b->dest = d->loc_bucket.as<unsigned int>();
  b->idx = b->dest + (n + 1);
  b->dest_sorted = b->idx + (n + 1);
  b->order = b->dest_sorted + (n + 1);
  return AMG_OK;
}

// Records by destination without a sort: a histogram of the destinations (LDS per tile, one atomic per tile and bin), the
// bins' first places, and a scatter in which every tile reserves its stretch of each bin with one atomic.  The order of
// the records INSIDE a destination is whatever the atomics make it — owners sum counts and minimise first-seen values,
// and replies come back in the order the records left.  (A library radix sort of 5.4 M (destination, index) pairs was
// ~0.25 ms of a first build's node phase.)
#define BK_MAX 256
#define BK_PER 8
__global__ __launch_bounds__(256) void k_bucket_hist(const unsigned int* __restrict__ dest, long long n, int bins,
                                                     unsigned long long* __restrict__ counts) {
  __shared__ unsigned int h[BK_MAX];
  for (int b = threadIdx.x; b < bins; b += 256) h[b] = 0u;
  __syncthreads();
  const long long i0 = (long long)blockIdx.x * (256 * BK_PER) + threadIdx.x;
#pragma unroll
  for (int j = 0; j < BK_PER; ++j) {
    const long long i = i0 + (long long)j * 256;
    if (i < n) atomicAdd(&h[dest[i]], 1u);
  }
  __syncthreads();
  for (int b = threadIdx.x; b < bins; b += 256)
    if (h[b]) atomicAdd(&counts[b], (unsigned long long)h[b]);
}
__global__ void k_bucket_starts(const unsigned long long* __restrict__ counts, int bins, unsigned long long* __restrict__ cursor) {
  if (threadIdx.x || blockIdx.x) return;
  unsigned long long s = 0;
  for (int b = 0; b < bins; ++b) {
    cursor[b] = s;
    s += counts[b];
  }
}
__global__ __launch_bounds__(256) void k_bucket_scatter(const unsigned int* __restrict__ dest, long long n, int bins,
                                                        unsigned long long* __restrict__ cursor, unsigned int* __restrict__ order) {
  __shared__ unsigned int h[BK_MAX];
  __shared__ unsigned long long base[BK_MAX];
  for (int b = threadIdx.x; b < bins; b += 256) h[b] = 0u;
  __syncthreads();
  const long long i0 = (long long)blockIdx.x * (256 * BK_PER) + threadIdx.x;
  unsigned int d[BK_PER], rank[BK_PER];
#pragma unroll
  for (int j = 0; j < BK_PER; ++j) {
    const long long i = i0 + (long long)j * 256;
    d[j] = 0u;
    rank[j] = 0u;
    if (i < n) {
      d[j] = dest[i];
      rank[j] = atomicAdd(&h[d[j]], 1u);
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < bins; b += 256)
    if (h[b]) base[b] = atomicAdd(&cursor[b], (unsigned long long)h[b]);
  __syncthreads();
#pragma unroll
  for (int j = 0; j < BK_PER; ++j) {
    const long long i = i0 + (long long)j * 256;
    if (i < n) order[base[d[j]] + rank[j]] = (unsigned int)i;
  }
}

// n ids bucketed (claim ids in use, holes included: destination `world`), n_real records among them: `order` lists the
// ids by destination and the per-destination counts stay in d->loc_dest_cnt ON THE DEVICE (one rank without holes:
// nothing to do)
static int dest_counts(amg_ctx* c, DistState* d, long long n, long long n_real, const Bucketing& b) {
  hipStream_t st = c->stream;
  const int world = d->world;
  d->nspace = n;
  d->sorted = world > 1 || n != n_real;
  if (!d->sorted) return AMG_OK;
  const int bins = world + 1;
  AMGCHK(d->loc_dest_cnt.ensure((size_t)(2 * bins + 2) * sizeof(unsigned long long)));
  unsigned long long* counts = d->loc_dest_cnt.as<unsigned long long>();
  unsigned long long* cursor = counts + bins + 1;
  HIPCHK(hipMemsetAsync(counts, 0, (size_t)(2 * bins + 2) * sizeof(unsigned long long), st));
  if (n <= 0) return AMG_OK;
  if (bins <= BK_MAX) {
    hipLaunchKernelGGL(k_bucket_hist, dim3(nblk(n, 256 * BK_PER)), dim3(256), 0, st, b.dest, n, bins, counts);
    hipLaunchKernelGGL(k_bucket_starts, dim3(1), dim3(1), 0, st, counts, bins, cursor);
    hipLaunchKernelGGL(k_bucket_scatter, dim3(nblk(n, 256 * BK_PER)), dim3(256), 0, st, b.dest, n, bins, cursor, b.order);
    return AMG_OK;
  }
  AMGCHK(prim_sort_u32_u32(c, b.dest, b.dest_sorted, b.idx, b.order, (size_t)n, ilog2_ceil((uint64_t)world + 1) + 1));
  hipLaunchKernelGGL(k_dest_counts, dim3(nblk(world, 64)), dim3(64), 0, st, b.dest_sorted, n, (unsigned int)world, counts);
  return AMG_OK;
}

// a table pass, repeated while the table `grows` names overflows: it is grown, up to 8 times.  Every other outcome is
// the caller's (*which: the cause of an AMG_E_OVERFLOW)
template <class Pass>
static int pass_until_fits(amg_ctx* c, Overflow grows, Overflow* which, Pass pass) {
  for (int attempt = 0;; ++attempt) {
    *which = OV_NONE;
    const int r = pass(which);
    if (r != AMG_E_OVERFLOW || *which != grows || attempt >= 8) return r;
    AMGCHK(grow_after_overflow(c, grows));
  }
}
// an edge pass reports two gene-mers under one merge key as an overflow of its own kind
static int edge_pass_result(int r, Overflow which, const char* what) {
  if (r == AMG_E_OVERFLOW && which == OV_COLLISION)
    return amg_fail(AMG_E_COLLISION, "%s: the merged build is repeated with the next seed", what);
  return r;
}

static int nodes_local_x(amg_ctx* c, DistState* d, unsigned long long key_mask) {
  hipStream_t st = c->stream;
  const int k = d->k, world = d->world;
  Overflow which;
  AMGCHK(pass_until_fits(c, OV_NODE_TABLE, &which,
                         [&](Overflow* w) { return bx_nodes_upsert(c, k, w, PassCaller::MergedLocal, nullptr); }));
  // claim ids in use lie below n (shard counters: with ids nobody took in between, first-seen 0)
  const long long n = c->x_nspace, T = c->n_tokens;
  // local occurrence counts per claim, straight from the per-window claims
  stage_begin(c, "node_count");
  AMGCHK(d->loc_cnt.ensure((size_t)(n + 2) * sizeof(unsigned int)));
  AMGCHK(count_ids(c, CountNodes, IdsClaimsMarked, c->tok_slot.as<int>(), T, n, d->loc_cnt.as<unsigned int>()));
  stage_end(c);
  stage_begin(c, "merge_node_bucket");
  Bucketing b;
  AMGCHK(bucketing(d, n, &b));
  AMGCHK(d->loc_first.ensure((size_t)(n + 1) * sizeof(unsigned long long)));  // keys per claim
  if (n > 0)
    // (x_two: dist_x implies !x_fp — bx_tuple_fits — so here and below it says "the TUPLE spills into the second word")
    hipLaunchKernelGGL(k_xd_node_keys, dim3(nblk(n, 256)), dim3(256), 0, st, c->node_tab.as<Slot16>(),
                       c->x_slot.as<unsigned int>(), c->x_first.as<unsigned int>(), n, k, c->x_bits,
                       c->x_two ? 1 : 0, c->seed, key_mask, (unsigned int)world,
                       (world > 1 || n != c->n_local_nodes) ? 1 : 0, d->loc_first.as<unsigned long long>(), b.dest, b.idx);
  const int r = dest_counts(c, d, n, c->n_local_nodes, b);
  stage_end(c);
  return r;
}

static int edges_local_x(amg_ctx* c, DistState* d) {
  hipStream_t st = c->stream;
  const int world = d->world;
  Overflow which;
  const int fits = pass_until_fits(c, OV_EDGE_TABLE, &which, [&](Overflow* w) {
    return bx_edges_upsert(c, w, false, PassCaller::MergedLocal, nullptr);
  });
  AMGCHK(edge_pass_result(fits, which, "two gene-mers share a merge key"));
  const long long n = c->x_espace, T = c->n_tokens;  // (claim ids in use lie below n: see nodes_local_x)
  stage_begin(c, "edge_count");
  AMGCHK(d->loc_cnt.ensure((size_t)(n + 2) * sizeof(unsigned int)));
  AMGCHK(count_ids(c, CountEdgeClasses, IdsClaimsMarked, c->tok_pair.as<int>(), T, n, d->loc_cnt.as<unsigned int>()));
  stage_end(c);
  stage_begin(c, "merge_edge_bucket");
  Bucketing b;
  AMGCHK(bucketing(d, n, &b));
  if (n > 0 && (world > 1 || n != c->n_local_pairs))
    hipLaunchKernelGGL(k_xd_edge_dest, dim3(nblk(n, 256)), dim3(256), 0, st, c->edge_tab.as<Slot16>(),
                       c->x_eslot.as<unsigned int>(), c->x_efirst.as<unsigned int>(), n, (unsigned int)world, b.dest, b.idx);
  const int r = dest_counts(c, d, n, c->n_local_pairs, b);
  stage_end(c);
  return r;
}

// fingerprint shards, after the table pass of a kind (0 nodes, 1 edge classes) left its key list (c->fp_keys): local
// occurrence counts, the list in first-seen order, destinations
static int fp_records_local(amg_ctx* c, DistState* d, int kind) {
  hipStream_t st = c->stream;
  const int world = d->world;
  const long long n = kind ? c->n_local_pairs : c->n_local_nodes;
  Slot* tab = kind ? c->edge_tab.as<Slot>() : c->node_tab.as<Slot>();
  // local occurrence counts: rank the local keys by first-seen (hot ones get low ids), count through LDS
  // (first-seen: token index << 1 | direction of a node, local so far; << 3 | orientation of a class, global already.
  // Nodes: tok_node is free scratch until the edge pass writes it)
  const uint64_t first_top = kind ? (uint64_t)(c->tok_total > 0 ? c->tok_total : 1) * 8 + 8
                                  : (uint64_t)(c->n_tokens > 0 ? c->n_tokens : 1) * 2 + 2;
  const FpKeyList& keys = c->fp_keys;
  AMGCHK(fp_list_sort(c, keys, ilog2_ceil(first_top) + 1));
  AMGCHK(d->loc_cnt.ensure((size_t)(n + 2) * sizeof(unsigned int)));
  AMGCHK(bs_count_by_slot(c, kind ? CountEdgeClasses : CountNodes, kind ? c->tok_pair.as<int>() : c->tok_slot.as<int>(),
                          kind ? c->tok_pair.as<int>() : c->tok_node.as<int>(), c->n_tokens, tab,
                          keys.slot_sorted, n, d->loc_cnt.as<unsigned int>()));
  Bucketing b;
  AMGCHK(bucketing(d, n, &b));
  // keep the sorted list in buffers of the merge's own: the later sorts use the generic scratch
  AMGCHK(d->loc_first.ensure((size_t)(n + 1) * sizeof(unsigned long long)));
  AMGCHK(d->loc_slot.ensure((size_t)(n + 1) * sizeof(unsigned int)));
  HIPCHK(hipMemcpyAsync(d->loc_first.p, keys.first_sorted, (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpyAsync(d->loc_slot.p, keys.slot_sorted, (size_t)n * sizeof(unsigned int), hipMemcpyDeviceToDevice, st));
  if (n > 0 && world > 1)
    hipLaunchKernelGGL(k_dist_dest, dim3(nblk(n, 256)), dim3(256), 0, st, d->loc_slot.as<unsigned int>(), n, tab,
                       (unsigned int)world, b.dest, b.idx);
  return dest_counts(c, d, n, n, b);
}

// the node pass of the shard; first-seen values stay LOCAL here (the shard's token base is learnt in the count
// exchange that follows) and become global when the records are packed
int nodes_local(amg_ctx* c, DistState* d) {
  const int k = d->k, world = d->world;
  stages_reset(c);
  c->sw = read_build_switches();  // (a merged build starts here)
  (void)ctx_build_begins(c);  // (the offer of a derived rebuild was taken or declined before: amg_dist.hip)
  ctx_build_from_reads(c, k, true);
  c->world = world;
  c->dist_min_node = d->mn;
  c->dist_min_edge = d->me;
  // merge keys and key owners are fingerprints of this seed: every rank must use the SAME one, whatever collision
  // retries an earlier single-GPU build on this ctx went through; `attempt` is the ranks' common retry counter
  c->seed = kAmgSeed0;
  for (int a = 0; a < d->attempt; ++a) c->seed = c->seed * 6364136223846793005ull + 1442695040888963407ull;
  c->count_inline = false;  // local occurrence counts come from the per-window claims, not per-window atomics
  bs_size_tables(c);
  c->exact_keys = false;
  // test hooks.  AMG_TEST_DIST_FAIL=r: rank r's node phase fails (its peers must be told).  AMG_TEST_DIST_WEAK_KEYS=n:
  // the first n attempts cut the merge keys to 10 bits, so that gene-mers share them and the build has to be repeated
  if (const char* e = getenv("AMG_TEST_DIST_FAIL"))
    if (atoi(e) == d->rank) return amg_fail(AMG_E_STATE, "told to fail (AMG_TEST_DIST_FAIL)");
  bool weak = false;
  if (const char* e = getenv("AMG_TEST_DIST_WEAK_KEYS")) weak = atoi(e) > d->attempt;
  c->weak_fp_builds = 0;
  c->dist_x = bx_tuple_fits(c, k);  // (the held records carry the tuple: the slots must hold it)
  if (c->dist_x) return nodes_local_x(c, d, weak ? 0x3ffull : ~0ull);
  c->weak_fp_builds = weak ? 1 : 0;
  Overflow which;
  AMGCHK(pass_until_fits(c, OV_NODE_TABLE, &which, [&](Overflow* w) { return bs_nodes_pass(c, k, w); }));
  return fp_records_local(c, d, 0);
}

int edges_local(amg_ctx* c, DistState* d) {
  if (c->dist_x) return edges_local_x(c, d);
  Overflow which;
  const int fits = pass_until_fits(c, OV_EDGE_TABLE, &which, [&](Overflow* w) { return bs_edges_pass(c, w); });
  AMGCHK(edge_pass_result(fits, which, "fingerprint collision"));
  return fp_records_local(c, d, 1);
}
