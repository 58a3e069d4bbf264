// amg_build_x_claims.hip — the exact-key build after its table passes (amg_build_x.hip): what is done once per CLAIM.
//
// A table pass leaves dense arrays indexed by claim id (first-seen, slot) and the claim of every window / adjacency.
// From those, per kind (nodes, edge classes):
//   * coverage = occurrences per claim (count_ids, amg_count.hip), stored per node by k_x_cov_from_claims;
//   * a build with the coverage filter applied on the way takes the claims below the threshold out of the claim space
//     before anything is ranked (k_x_drop_claims);
//   * node id / edge-class id = rank of first-seen among the claims that are left (the bitmap ranking below), and the
//     node arrays / edge-class arrays in that order (k_x_assign_nodes_ranked, k_x_gather_pairs_ranked).
// The drivers bx_nodes / bx_nodes_filtered and bx_edges run a table pass and this stage; the component ids and touched
// reads of a filtered build are amg_build_x_comp.hip's.
#include "amg_slot16.h"

// ---- build with the coverage filter applied on the way (amg_build_filtered): claims below the threshold are
// taken out of the claim space (first-seen words zeroed = "unclaimed", which every ranking kernel skips) before
// anything is ranked, so only the survivors get ids, arrays, edges
__global__ void k_x_drop_claims(const unsigned int* __restrict__ cnt, long long n, unsigned int min_cnt,
                                unsigned int* __restrict__ first2, int* __restrict__ final_of_claim,
                                unsigned long long* __restrict__ n_kept, unsigned int* __restrict__ first_all) {
  long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  bool keep = false;
  if (c < n) {
    if (first_all) first_all[c] = x_first_inv(first2, c);  // component labels are those of the UNFILTERED graph
    keep = cnt[c] >= min_cnt && x_first_inv(first2, c) != 0u;
    if (!keep) {
      first2[2 * c] = 0u;
      first2[2 * c + 1] = 0u;
      if (final_of_claim) final_of_claim[c] = -2;  // windows of a dropped node read None (remove_node_from_reads)
    }
  }
  const unsigned long long m = __ballot(keep);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(n_kept, (unsigned long long)__popcll(m));
}

// tagged != nullptr: claim -> node id | AMG_SINGLE_BIT where the node's coverage is 1 (what k_edges_v<.., LONE> reads)
__global__ void k_x_cov_from_claims(const unsigned int* __restrict__ cnt, const unsigned int* __restrict__ first2,
                                    const int* __restrict__ final_of_claim, long long n,
                                    unsigned int* __restrict__ node_cov, int* __restrict__ tagged) {
  long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  const int id = final_of_claim[c];
  const bool used = x_first_inv(first2, c) != 0u;
  if (tagged) tagged[c] = (used && id >= 0 && cnt[c] == 1u) ? (int)((unsigned int)id | AMG_SINGLE_BIT) : id;
  if (used) node_cov[id] = cnt[c];
}

// ---- ranking by first-seen without a sort.  A token
// position opens at most one window / adjacency, so the first-seen token indices of the claims are
// distinct: set one bit per claim in a bitmap over the tokens, prefix-count the bitmap words, and
// the rank of a claim is the number of bits before its own (x_rank_of).  (A radix sort of 0.5 - 1 M pairs
// costs ~10 launches and ~0.2 ms however small the input; this costs ~0.06 ms.  At 5.4 M claims: 0.38 against 0.44 ms.)
// (one BYTE per token first, set with plain stores: 5.4 M scattered atomicOr on bitmap words ran at the
// memory-side atomic rate, 0.2 ms per ranking of the first build; the bytes are folded into the
// bitmap words by the pass that counts them)
__global__ void k_x_rank_setflags(const unsigned int* __restrict__ first2, long long n, int shift,
                                  unsigned char* __restrict__ flags) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned int fi = x_first_inv(first2, i);
  if (fi == 0u) return;  // a claim id nobody took (the chunked shards leave holes: XShard)
  flags[(~fi) >> shift] = 1;
}

// The one owner of the ranking's buffers: flag bytes in s0 (32 per bitmap word), bitmap words in s1, exclusive prefix of
// the word popcounts in s5 with the total behind it.
static long long rank_words(const amg_ctx* c) { return (c->n_tokens >> 5) + 2; }

// the flag bytes are zeroed behind a read-back kernel, while the host waits for it.  The caller ranks next, with nothing
// in between that writes s0, and hands *zeroed to rank_bitmap_begin, which then saves its clear
int rank_flags_zero_behind(amg_ctx* c, ClearList* filler, RankFlagsZeroed* zeroed) {
  const long long words = rank_words(c);
  AMGCHK(c->s0.ensure((size_t)words * 32 + 64));
  filler->add(c->s0.p, (size_t)words * 32);
  *zeroed = RankFlagsZeroed{c->s0.p, words};
  return AMG_OK;
}

int rank_bitmap_begin(amg_ctx* c, const RankFlagsZeroed& zeroed, unsigned char** flags) {
  const long long words = rank_words(c);
  AMGCHK(c->s1.ensure((size_t)words * sizeof(unsigned int)));
  AMGCHK(c->s5.ensure((size_t)(words + 2) * sizeof(long long)));
  AMGCHK(c->s0.ensure((size_t)words * 32 + 64));
  if (zeroed.flags != c->s0.p || zeroed.words != words) {
    ClearList cl;
    cl.add(c->s0.p, (size_t)words * 32);
    AMGCHK(clear_many(c, cl));
  }
  *flags = c->s0.as<unsigned char>();
  return AMG_OK;
}

// the flag bytes are folded into the bitmap words by the scan that counts them (one launch, no count array)
int rank_bitmap_finish(amg_ctx* c, RankBitmap* r) {
  const long long words = rank_words(c);
  *r = RankBitmap{c->s1.as<unsigned int>(), c->s5.as<long long>(), c->s5.as<long long>() + words};
  return prim_exscan_flag_words(c, c->s0.as<unsigned char>(), c->s1.as<unsigned int>(), c->s5.as<long long>(), (size_t)words);
}

// the ranking of the claims 0 .. n - 1 whose first-seen words are not zero (shift: 1 nodes, 3 edge classes)
int rank_first_seen(amg_ctx* c, const unsigned int* first2, long long n, int shift, const RankFlagsZeroed& zeroed,
                    RankBitmap* r) {
  unsigned char* flags;
  AMGCHK(rank_bitmap_begin(c, zeroed, &flags));
  hipLaunchKernelGGL(k_x_rank_setflags, dim3(nblk(n, 256)), dim3(256), 0, c->stream, first2, n, shift, flags);
  return rank_bitmap_finish(c, r);
}

// A node's tuple is the window at its first-seen position, reversed and flipped when the first-seen's direction bit
// (bit 0: ndir of k_nodes_m / k_nodes_v, whatever the key scheme) is set: the canonical tuple, read from the reads
// rather than unpacked from the key's table slot (one random 16-byte read per claim of a table of hundreds of MB; the
// claims of a wave were made by one tile, so their windows lie within the same 1 024 tokens).  A window lies inside its
// read: f + k <= n_tokens.
// The wave writes the 64 k tokens of its 64 nodes with a node's k tokens on neighbouring lanes: lane l of round m takes
// token (l + 64 m) % k of the node of lane (l + 64 m) / k, so the nodes of consecutive ids — a wave's, nearly always —
// leave as contiguous 256-byte stores (a lane writing its own k tokens puts the lanes of one store k ints apart).
// Every lane of the wave calls; node < 0: this lane has none.
__device__ __forceinline__ void node_tuples_from_reads(int* __restrict__ node_tokens, const int* __restrict__ tokens,
                                                       int node, unsigned int first, int k, int flip) {
  const unsigned int lane = threadIdx.x & 63u;
  for (int m = 0; m < k; ++m) {
    const unsigned int e = lane + 64u * (unsigned int)m;
    const unsigned int q = e / (unsigned int)k, j = e - q * (unsigned int)k;  // (q < 64: e < 64 k)
    const int nq = __shfl(node, (int)q, 64);
    const unsigned int fq = __shfl(first, (int)q, 64);
    if (nq < 0) continue;
    const int* w = tokens + (long long)(fq >> 1);
    node_tokens[(long long)nq * k + j] = (fq & 1u) ? flip - w[k - 1 - (int)j] : w[j];
  }
}

__global__ __launch_bounds__(256) void k_x_assign_nodes_ranked(
    const unsigned int* __restrict__ first2, long long n_nodes, const unsigned int* __restrict__ bits,
    const long long* __restrict__ prefix, int k, int* __restrict__ final_of_claim, int* __restrict__ node_tokens,
    long long* __restrict__ node_first, unsigned char* __restrict__ node_alive, const int* __restrict__ tokens, int flip) {
  const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned int fi = c < n_nodes ? x_first_inv(first2, c) : 0u;  // 0: unclaimed (or past the end): no node
  const unsigned int first = ~fi;
  int node = -1;
  if (fi != 0u) {
    const long long i = x_rank_of(first >> 1, bits, prefix);
    node = (int)i;
    final_of_claim[c] = node;
    node_first[i] = (long long)first;
    node_alive[i] = 1;
  }
  node_tuples_from_reads(node_tokens, tokens, node, first, k, flip);
}

// edge classes in first-seen order: key, first, count (counted per claim by k_count_ids)
__global__ void k_x_gather_pairs_ranked(const unsigned int* __restrict__ first2, long long n_pairs,
                                        const unsigned int* __restrict__ bits, const long long* __restrict__ prefix,
                                        const Slot16* __restrict__ etab, const unsigned int* __restrict__ slot_by_claim,
                                        const unsigned int* __restrict__ cnt_by_claim,
                                        unsigned long long* __restrict__ pkey, unsigned long long* __restrict__ pfirst,
                                        unsigned int* __restrict__ pcnt) {
  long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n_pairs) return;
  if (x_first_inv(first2, c) == 0u) return;  // unclaimed
  const unsigned int first = ~x_first_inv(first2, c);
  const long long i = x_rank_of(first >> 3, bits, prefix);
  pkey[i] = etab[slot_by_claim[c]].w1;
  pfirst[i] = (unsigned long long)first;
  pcnt[i] = cnt_by_claim[c];
}

// ------------------------------------------------------------------ host side
// node id = rank of first-seen among the claims; node arrays
static int bx_nodes_rank(amg_ctx* c, const RankFlagsZeroed& zeroed) {
  stage_begin(c, "node_rank");
  const long long D = c->n_nodes;
  const long long S = c->x_nspace;  // claim ids in use (== D unless handed out in interleaved shards, or dropped by the filter)
  AMGCHK(bs_alloc_nodes(c, D));
  if (D > 0) {
    RankBitmap r;
    AMGCHK(rank_first_seen(c, c->x_first.as<unsigned int>(), S, 1, zeroed, &r));
    hipLaunchKernelGGL(k_x_assign_nodes_ranked, dim3(nblk(S, 256)), dim3(256), 0, c->stream,
                       c->x_first.as<unsigned int>(), S, r.bits, r.prefix, c->k, c->x_final.as<int>(),
                       c->node_tokens.as<int>(), c->node_first.as<long long>(), c->node_alive.as<unsigned char>(),
                       c->tokens.as<int>(), c->two_v - 1);
  }
  stage_end(c);
  return AMG_OK;
}

// windows -> node table, claim ids, node ids, node arrays.  AMG_E_OVERFLOW + *which = OV_NODE_TABLE: table full
int bx_nodes(amg_ctx* c, int k, Overflow* which) {
  RankFlagsZeroed zeroed;
  AMGCHK(bx_nodes_upsert(c, k, which, PassCaller::PlainBuild, &zeroed));
  return bx_nodes_rank(c, zeroed);
}

// node table pass, then only the nodes with coverage >= min_cov are kept: ids, arrays and coverages of the
// survivors; x_final = -2 for the others
int bx_nodes_filtered(amg_ctx* c, int k, unsigned int min_cov, Overflow* which) {
  hipStream_t st = c->stream;
  RankFlagsZeroed zeroed;
  AMGCHK(bx_nodes_upsert(c, k, which, PassCaller::FilteredBuild, &zeroed));
  // claim ids in use lie below n (shard counters: with ids nobody took in between — first-seen 0, like the claims
  // dropped here)
  const long long n = c->x_nspace, T = c->n_tokens;
  stage_begin(c, "node_count");  // per claim, straight from the per-window claims (construct_node.py:33-36)
  AMGCHK(c->x_ecnt.ensure((size_t)(n + 2) * sizeof(unsigned int)));
  AMGCHK(count_ids(c, CountNodes, IdsClaimsMarked, c->tok_slot.as<int>(), T, n, c->x_ecnt.as<unsigned int>()));
  stage_end(c);
  stage_begin(c, "node_filter");
  AMGCHK(c->x_first_all.ensure((size_t)(n + 2) * sizeof(unsigned int)));
  c->comp_from_claims = true;
  unsigned long long* kept = c->status.as<unsigned long long>() + ST_COMPACT_A;
  HIPCHK(hipMemsetAsync(kept, 0, sizeof(unsigned long long), st));
  if (n > 0)
    hipLaunchKernelGGL(k_x_drop_claims, dim3(nblk(n, 256)), dim3(256), 0, st, c->x_ecnt.as<unsigned int>(), n,
                       min_cov, c->x_first.as<unsigned int>(), c->x_final.as<int>(), kept,
                       c->x_first_all.as<unsigned int>());
  unsigned long long D = 0;
  {
    FetchList l;
    l.add(kept);
    l.add(c->status.as<unsigned long long>() + ST_COLLISION);
    unsigned long long v[2] = {0, 0};
    AMGCHK(fetch(c, l, v));
    D = v[0];
    if (v[1]) {  // two gene-mers share a fingerprint (k_x_verify_fp): the build is repeated with the next seed
      stage_end(c);
      return overflowed(which, OV_COLLISION);
    }
  }
  stage_end(c);
  c->n_nodes = (int64_t)D;
  AMGCHK(bx_nodes_rank(c, zeroed));
  if (n > 0 && D > 0)
    hipLaunchKernelGGL(k_x_cov_from_claims, dim3(nblk(n, 256)), dim3(256), 0, st, c->x_ecnt.as<unsigned int>(),
                       c->x_first.as<unsigned int>(), c->x_final.as<int>(), n, c->node_cov.as<unsigned int>(), (int*)nullptr);
  return AMG_OK;
}

// node coverage of a plain build (construct_node.py:33-36): occurrences per CLAIM from the node pass's per-window
// claims — the occurrence that created a key is marked there, so the keys seen once (most of an uncorrected graph)
// cost nothing — then one store per claim into the node's counter.  tag: x_ftag = x_final with AMG_SINGLE_BIT
static int bx_node_count(amg_ctx* c, bool tag) {
  const long long T = c->n_tokens, D = c->n_nodes;
  stage_begin(c, "node_count");
  const long long S = c->x_nspace;
  AMGCHK(c->x_ncnt.ensure((size_t)(S + 2) * sizeof(unsigned int)));
  if (tag) AMGCHK(c->x_ftag.ensure((size_t)(S + 2) * sizeof(int)));
  AMGCHK(count_ids(c, CountNodes, IdsClaimsMarked, c->tok_slot.as<int>(), T, S, c->x_ncnt.as<unsigned int>()));
  if (S > 0 && D > 0)
    hipLaunchKernelGGL(k_x_cov_from_claims, dim3(nblk(S, 256)), dim3(256), 0, c->stream,
                       c->x_ncnt.as<unsigned int>(), c->x_first.as<unsigned int>(), c->x_final.as<int>(), S,
                       c->node_cov.as<unsigned int>(), tag ? c->x_ftag.as<int>() : (int*)nullptr);
  stage_end(c);
  return AMG_OK;
}

// coverages, then the edge classes in first-seen order (pair_key / pair_first / pair_cnt) from the claims' arrays.
// min_edge_cov > 1: the build applies the coverage filter on the way and the classes below it are dropped before ranking
static int bx_edges_rank(amg_ctx* c, unsigned int min_edge_cov, const RankFlagsZeroed& zeroed) {
  hipStream_t st = c->stream;
  const long long T = c->n_tokens, S = c->x_espace;  // (claim ids in use lie below S)
  stage_begin(c, "edge_count");  // edge-class coverage per claim
  AMGCHK(c->x_ecnt.ensure((size_t)(S + 2) * sizeof(unsigned int)));
  AMGCHK(count_ids(c, CountEdgeClasses, IdsClaimsMarked, c->tok_pair.as<int>(), T, S, c->x_ecnt.as<unsigned int>()));
  stage_end(c);
  if (min_edge_cov > 1 && S > 0) {  // filter_graph's edge threshold (:531-535)
    unsigned long long* kept = c->status.as<unsigned long long>() + ST_COMPACT_A;
    HIPCHK(hipMemsetAsync(kept, 0, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(k_x_drop_claims, dim3(nblk(S, 256)), dim3(256), 0, st, c->x_ecnt.as<unsigned int>(), S,
                       min_edge_cov, c->x_efirst.as<unsigned int>(), (int*)nullptr, kept, (unsigned int*)nullptr);
    unsigned long long left = 0;
    FetchList l;
    l.add(kept);
    AMGCHK(fetch(c, l, &left));
    c->n_pairs = (int64_t)left;  // x_espace stays: the dropped classes are holes of the claim space
  }
  const long long P = c->n_pairs;
  stage_begin(c, "edge_rank");
  AMGCHK(bs_alloc_pairs(c, P));
  if (P > 0) {
    RankBitmap r;
    AMGCHK(rank_first_seen(c, c->x_efirst.as<unsigned int>(), S, 3, zeroed, &r));
    hipLaunchKernelGGL(k_x_gather_pairs_ranked, dim3(nblk(S, 256)), dim3(256), 0, st, c->x_efirst.as<unsigned int>(), S,
                       r.bits, r.prefix, c->edge_tab.as<Slot16>(), c->x_eslot.as<unsigned int>(),
                       c->x_ecnt.as<unsigned int>(), c->pair_key.as<unsigned long long>(),
                       c->pair_first.as<unsigned long long>(), c->pair_cnt.as<unsigned int>());
  }
  stage_end(c);
  return AMG_OK;
}

// adjacencies -> edge-class table, claims, pair arrays in first-seen order, coverages.
// AMG_E_OVERFLOW + *which = OV_EDGE_TABLE: edge table full
int bx_edges(amg_ctx* c, Overflow* which, PassCaller who, unsigned int min_edge_cov) {
  // a plain build counts its nodes BEFORE the edge pass (a filtered build has counted them to filter them): the nodes
  // of coverage 1 (nine in ten of an uncorrected graph) mark the edge classes that occur once, and those need no
  // table (k_edges_v<.., LONE>)
  bool lone = false;
  if (who == PassCaller::PlainBuild) {
    const bool can = c->sw.edge_home && c->n_nodes > 0;
    // AMG_EDGE_LONE (A/B + test switch): 0 never, 1 whenever the kernel allows it; else where it is
    // worth its extra words per window: where many nodes are single, more than one node per 16 windows
    lone = can && (c->sw.edge_lone >= 0 ? c->sw.edge_lone != 0 : c->n_nodes * 16 > c->n_tokens);
    AMGCHK(bx_node_count(c, lone));
  }
  RankFlagsZeroed zeroed;
  AMGCHK(bx_edges_upsert(c, which, lone, who, &zeroed));
  return bx_edges_rank(c, min_edge_cov, zeroed);
}
