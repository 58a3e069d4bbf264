// amg_build_fp.hip — the node and edge-class stages of a build on 32-byte slots keyed by VERIFIED FINGERPRINTS
// (GeneMerGraph.__init__, reference construct_graph.py:31-102): the path of 2^29 tokens and more, of AMG_KEY_MODE=fp and of
// merged builds whose tuple does not fit a 16-byte slot.  Here: its table passes, the ranking of their slots by
// first-seen, and bs_count_by_slot, the merged build's count over such a table.  The driver that picks this path, and
// what follows the edge classes, is amg_build.hip.
//
// Launch sequence of amg_build on this path, all on ctx->stream (most builds take amg_build_x.hip's: build_impl):
//   k_read_stats      per-read window / short-read counts, read-end bitmap (construct_graph.py:53-55; bs_read_stats,
//                     amg_build.hip)
//   k_node_upsert     K1+K2: LDS-staged sliding windows, canonical orientation
//                     (construct_gene_mer.py:4-56), fingerprint, open-address upsert:
//                     count (+=1, construct_node.py:33-36) and first-seen (atomicMax of ~first)
//   k_compact_slots   wave-ballot / prefix-sum compaction of occupied slots
//   radix sort        by first-seen  -> node id = insertion order of _nodes (:188-190)
//   k_assign_nodes    dense node arrays (canonical tokens, coverage, first direction)
//   k_edges           K3/K4: slot -> node id per window (get_readNodes, :165-178), exact
//                     verification of the fingerprint against the node's canonical tuple,
//                     and upsert of one record per adjacency into the edge-class table
//                     (create_edges / add_edge_to_edges, :246-277; Edge.__hash__ classes,
//                     construct_edge.py:104-124)
//   k_compact_slots + sort + k_gather_pairs
//                     edge classes in first-seen order
//   k_count_ids       node and edge-class coverage, unless AMG_COUNT_INLINE (amg_count.hip)
// then, as on every path (bs_finish_from_pairs, amg_build.hip):
//   the pair-width scan that emits the edges (amg_scan.hip)
//                     directed edges in _edges insertion order, E1 then E2 (:279-285)
// and on first use (amg_adjacency.hip):
//   k_adj_keys + stable radix sort + k_row_offsets, or k_adjc_*
//                     forwardEdgeHashes / backwardEdgeHashes lists (:287-298)
//   k_uf_*            connected components, ids in DFS discovery order (:911-927)
#include "amg_device.h"

#include "amg_tile.h"

// ------------------------------------------------------------------ K1 + K2
__global__ __launch_bounds__(TILE_THREADS) void k_node_upsert(
    const int* __restrict__ tokens, const unsigned int* __restrict__ bnd_bits, long long n_tokens, int k,
    int two_v, unsigned long long seed, Slot* __restrict__ tab, unsigned long long mask,
    unsigned int probe_limit, long long tok_base, int* __restrict__ tok_slot,
    signed char* __restrict__ tok_dir, unsigned long long* status, int count_inline,
    unsigned long long fp_mask) {
  __shared__ int s_tok[TILE + AMG_MAX_K];
  __shared__ unsigned int s_bits[TILE_BIT_WORDS];
  const long long t0 = (long long)blockIdx.x * TILE;
  stage_tile(tokens, bnd_bits, n_tokens, k, t0, s_tok, s_bits, two_v, status);
  const int flip = two_v - 1;
#pragma unroll
  for (int it = 0; it < TILE_ITEMS; ++it) {
    int i = threadIdx.x + it * TILE_THREADS;
    long long t = t0 + i;
    if (t >= n_tokens) continue;
    bool inside, is_last;
    tile_window(s_bits, i, k, inside, is_last);
    const bool valid = (t + k <= n_tokens) && inside;
    int out_slot = -1;
    signed char out_dir = 0;
    if (valid) {
      LdsView w{s_tok + i};
      int dir = canon_dir(w, k, flip);
      if (dir == 0) {
        status[ST_PALINDROME] = 1;  // benign race: every writer stores 1
      } else {
        unsigned long long fp = canon_fingerprint(w, k, flip, dir, seed) & fp_mask;  // mask: test hook
        fp = fp ? fp : 1ull;
        unsigned long long first = ((unsigned long long)(tok_base + t) << 1) | (dir < 0 ? 1ull : 0ull);
        long long slot = table_upsert(tab, mask, fp, fp >> 20, first, probe_limit, count_inline != 0,
                                      status + ST_OVERFLOW);
        if (slot < 0) {
          status[ST_OVERFLOW] = 1;
        } else {
          out_slot = (int)((unsigned int)slot | (is_last ? AMG_LAST_FLAG : 0u));
          out_dir = (signed char)dir;
        }
      }
    }
    tok_slot[t] = out_slot;
    tok_dir[t] = out_dir;
  }
}

// ------------------------------------------------------------------ compaction
// (first_seen, slot) of every occupied slot, any order; one atomicAdd per block.
__global__ __launch_bounds__(256) void k_compact_slots(const Slot* __restrict__ tab,
                                                       unsigned long long n_slots,
                                                       unsigned long long* __restrict__ out_first,
                                                       unsigned int* __restrict__ out_slot,
                                                       unsigned long long* counter) {
  __shared__ unsigned int s_wave[4];
  __shared__ unsigned long long s_base;
  const int ITEMS = 8;
  unsigned long long base = (unsigned long long)blockIdx.x * (256 * ITEMS);
  unsigned long long firsts[ITEMS];
  unsigned int have = 0, cnt = 0;
#pragma unroll
  for (int it = 0; it < ITEMS; ++it) {
    unsigned long long s = base + it * 256 + threadIdx.x;
    if (s < n_slots && tab[s].key != 0ull) {
      firsts[it] = ~tab[s].first_inv;
      have |= 1u << it;
      ++cnt;
    }
  }
  unsigned int total;
  unsigned int off = block_exscan_256(cnt, &total, s_wave);
  if (threadIdx.x == 0) s_base = total ? atomicAdd(counter, (unsigned long long)total) : 0ull;
  __syncthreads();
  unsigned long long o = s_base + off;
#pragma unroll
  for (int it = 0; it < ITEMS; ++it) {
    if (have & (1u << it)) {
      out_first[o] = firsts[it];
      out_slot[o] = (unsigned int)(base + it * 256 + threadIdx.x);
      ++o;
    }
  }
}

// ------------------------------------------------------------------ node arrays
__global__ void k_assign_nodes(const unsigned long long* __restrict__ first_sorted,
                               const unsigned int* __restrict__ slot_sorted, long long n_nodes,
                               Slot* __restrict__ tab, const int* __restrict__ tokens, int k,
                               int two_v, long long tok_base, int packed, int* __restrict__ node_tokens,
                               unsigned int* __restrict__ node_cov,
                               long long* __restrict__ node_first,
                               unsigned char* __restrict__ node_alive) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_nodes) return;
  unsigned long long first = first_sorted[i];
  unsigned int slot = slot_sorted[i];
  tab[slot].id = (int)i;
  node_cov[i] = tab[slot].count;  // 0 when counting is deferred to k_count_ids
  node_first[i] = (long long)first;
  node_alive[i] = 1;
  long long t = (long long)(first >> 1) - tok_base;
  int dir = (first & 1ull) ? -1 : 1;
  const int flip = two_v - 1;
  int canon[AMG_MAX_K];
  for (int j = 0; j < k; ++j) {
    canon[j] = dir > 0 ? tokens[t + j] : flip - tokens[t + k - 1 - j];
    node_tokens[i * k + j] = canon[j];
  }
  if (packed) slot_pack(tab + slot, (int)i, canon, k);
}

// ------------------------------------------------------------------ K3 + K4
__global__ __launch_bounds__(TILE_THREADS) void k_edges(
    const int* __restrict__ tokens, long long n_tokens, int k, int two_v,
    const Slot* __restrict__ node_tab, const int* __restrict__ node_tokens,
    const int* __restrict__ tok_slot, const signed char* __restrict__ tok_dir,
    int* __restrict__ tok_node, Slot* __restrict__ edge_tab, unsigned long long edge_mask,
    unsigned int probe_limit, int verify, long long tok_base, unsigned long long* status,
    int count_inline, int* __restrict__ tok_pair, int packed) {
  __shared__ int s_id[TILE + 1];
  __shared__ int s_raw[TILE + 1];
  __shared__ signed char s_dir[TILE + 1];
  const long long t0 = (long long)blockIdx.x * TILE;
  const int flip = two_v - 1;
  for (int i = threadIdx.x; i < TILE + 1; i += TILE_THREADS) {
    long long t = t0 + i;
    int raw = -1;
    signed char d = 0;
    if (t < n_tokens) {
      raw = tok_slot[t];
      d = tok_dir[t];
    }
    int id = -1;
    if (raw != -1 && packed) {
      // one 32-byte gather: node id + the node's canonical tuple (16-bit tokens)
      const uint4* rec = reinterpret_cast<const uint4*>(node_tab + ((unsigned int)raw & ~AMG_LAST_FLAG));
      const uint4 lo = rec[0], hi = rec[1];
      id = (int)hi.y;
      if (verify && i < TILE && id >= 0) {
        const int* w = tokens + t;
        bool same = true;
        for (int j = 0; j < k; ++j) {
          int cj = d > 0 ? w[j] : flip - w[k - 1 - j];
          same = same && ((unsigned int)cj == packed_tok(lo, hi, j));
        }
        if (!same) status[ST_COLLISION] = 1;
      }
    } else if (raw != -1) {
      id = node_tab[(unsigned int)raw & ~AMG_LAST_FLAG].id;
      if (verify && i < TILE && id >= 0) {
        // exact check: the window's canonical tuple must equal the node's tuple
        const int* w = tokens + t;
        const int* nt = node_tokens + (long long)id * k;
        bool same = true;
        for (int j = 0; j < k; ++j) {
          int c = d > 0 ? w[j] : flip - w[k - 1 - j];
          same = same && (c == nt[j]);
        }
        if (!same) status[ST_COLLISION] = 1;
      }
    }
    s_id[i] = id;
    s_raw[i] = raw;
    s_dir[i] = d;
    if (i < TILE && t < n_tokens) tok_node[t] = id;
  }
  __syncthreads();
#pragma unroll
  for (int it = 0; it < TILE_ITEMS; ++it) {
    int i = threadIdx.x + it * TILE_THREADS;
    int raw = s_raw[i];
    if (raw == -1 || ((unsigned int)raw & AMG_LAST_FLAG)) {
      if (tok_pair && t0 + i < n_tokens) tok_pair[t0 + i] = -1;
      continue;
    }
    // adjacency (A, dA) -> (B, dB): windows t and t + 1 of the same read.  (ids < 0 only in a
    // merged build with a fused coverage filter: the node was dropped, no edge is recorded)
    if (s_id[i] < 0 || s_id[i + 1] < 0) {
      if (tok_pair && t0 + i < n_tokens) tok_pair[t0 + i] = -1;
      continue;
    }
    unsigned int a = (unsigned int)s_id[i], b = (unsigned int)s_id[i + 1];
    int dA = s_dir[i], dB = s_dir[i + 1];
    unsigned int lo = a < b ? a : b, hi = a < b ? b : a;
    unsigned long long sign = (dA * dB < 0) ? 1ull : 0ull;
    unsigned long long key = (sign << 63) | ((unsigned long long)lo << 32) |
                             (unsigned long long)(hi + 1u);
    unsigned long long orient = (a == lo ? 1ull : 0ull) | (dA > 0 ? 2ull : 0ull) |
                                (dB > 0 ? 4ull : 0ull);
    unsigned long long first = ((unsigned long long)(tok_base + t0 + i) << 3) | orient;
    long long slot = table_upsert(edge_tab, edge_mask, key, mix64(key), first, probe_limit,
                                  count_inline != 0);
    if (slot < 0) status[ST_OVERFLOW] = 2;
    if (tok_pair) tok_pair[t0 + i] = (int)slot;
  }
}

// ------------------------------------------------------------------ edge classes in order, counts by slot
// edge classes ("pairs") in first-seen order as plain arrays: key, count, first
__global__ void k_gather_pairs(const unsigned int* __restrict__ slot_sorted, long long n_pairs,
                               const Slot* __restrict__ edge_tab, unsigned long long* __restrict__ pkey,
                               unsigned int* __restrict__ pcnt) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_pairs) return;
  const Slot* s = edge_tab + slot_sorted[i];
  pkey[i] = s->key;
  pcnt[i] = s->count;
}

__global__ void k_set_pair_ids(const unsigned int* __restrict__ slot_sorted, long long n_pairs,
                               Slot* __restrict__ edge_tab) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_pairs) edge_tab[slot_sorted[i]].id = (int)i;
}

__global__ void k_slots_to_ids(const int* __restrict__ slots, long long n, const Slot* __restrict__ tab,
                               int* __restrict__ ids) {
  long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int raw = slots[t];
  ids[t] = raw == -1 ? -1 : tab[(unsigned int)raw & ~AMG_LAST_FLAG].id;
}

// Occurrences per table entry without per-window atomics, for the merge path: entries get
// dense ids in first-seen order (slot_sorted), the per-window slots are turned into ids
// (ids_scratch may alias slots) and counted by k_count_ids.  out[i] = count of entry i.
int bs_count_by_slot(amg_ctx* c, CountKind what, const int* slots, int* ids_scratch, long long n, Slot* tab,
                     const unsigned int* slot_sorted, long long n_ids, unsigned int* out) {
  hipStream_t st = c->stream;
  if (n_ids > 0)
    hipLaunchKernelGGL(k_set_pair_ids, dim3((unsigned)((n_ids + 255) / 256)), dim3(256), 0, st, slot_sorted,
                       n_ids, tab);
  if (n > 0)
    hipLaunchKernelGGL(k_slots_to_ids, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, slots, n, tab,
                       ids_scratch);
  return count_ids(c, what, IdsPlain, ids_scratch, n, n_ids, out);
}

// ------------------------------------------------------------------ host stages
// the tail of both table passes: the key list of the table's occupied slots (c->fp_keys, with room for its sorted form),
// their number into status word `counter`, and the status words to the host
static int compact_table(amg_ctx* c, const DevBuf& tab, int64_t slots, int counter, unsigned long long* hs) {
  // worst case every slot is occupied; size scratch by min(slots, windows upper bound)
  const size_t max_keys = (size_t)((long long)slots < c->n_tokens ? slots : c->n_tokens) + 1;
  AMGCHK(c->s1.ensure(max_keys * sizeof(unsigned long long)));
  AMGCHK(c->s2.ensure(max_keys * sizeof(unsigned long long)));
  AMGCHK(c->s3.ensure(max_keys * sizeof(unsigned int)));
  AMGCHK(c->s4.ensure(max_keys * sizeof(unsigned int)));
  hipLaunchKernelGGL(k_compact_slots, dim3(nblk(slots, 2048)), dim3(256), 0, c->stream, tab.as<Slot>(),
                     (unsigned long long)slots, c->s1.as<unsigned long long>(), c->s3.as<unsigned int>(),
                     c->status.as<unsigned long long>() + counter);
  AMGCHK(fetch_status(c, hs));
  c->fp_keys = FpKeyList{c->s1.as<unsigned long long>(), c->s3.as<unsigned int>(), c->s2.as<unsigned long long>(),
                         c->s4.as<unsigned int>(), (long long)hs[counter]};
  return AMG_OK;
}

int fp_list_sort(amg_ctx* c, const FpKeyList& list, int first_bits, unsigned long long* sorted_first_out) {
  if (!list.first || list.first != c->s1.p || list.first_sorted != c->s2.p || list.slot != c->s3.p || list.slot_sorted != c->s4.p)
    return amg_fail(AMG_E_STATE, "fp_list_sort: the key list is not the ctx's current one: something reserved scratch "
                                 "between the table pass and its ranking");
  return prim_sort_u64_u32(c, list.first, sorted_first_out ? sorted_first_out : list.first_sorted, list.slot, list.slot_sorted,
                           (size_t)list.n, first_bits);
}

// returns AMG_OK, or AMG_E_OVERFLOW with *which = OV_NODE_TABLE (node table too small)
int bs_nodes_pass(amg_ctx* c, int k, Overflow* which) {
  *which = OV_NONE;
  hipStream_t st = c->stream;
  const long long T = c->n_tokens;
  unsigned long long hs[ST_WORDS];
  HIPCHK(hipMemsetAsync(c->status.p, 0, ST_WORDS * sizeof(unsigned long long), st));

  AMGCHK(bs_read_stats(c, k));
  const long long n_tiles = (T + TILE - 1) / TILE;

  AMGCHK(c->tok_slot.ensure((size_t)(T + 1) * sizeof(int)));
  AMGCHK(c->tok_node.ensure((size_t)(T + 1) * sizeof(int)));
  AMGCHK(c->tok_dir.ensure((size_t)(T + 1)));
  AMGCHK(c->node_tab.ensure((size_t)c->node_slots * sizeof(Slot)));

  stage_begin(c, "node_table_clear");
  HIPCHK(hipMemsetAsync(c->node_tab.p, 0, (size_t)c->node_slots * sizeof(Slot), st));
  stage_end(c);

  stage_begin(c, "node_upsert");
  if (n_tiles > 0)
    hipLaunchKernelGGL(k_node_upsert, dim3((unsigned)n_tiles), dim3(TILE_THREADS), 0, st,
                       c->tokens.as<int>(), c->bnd_bits.as<unsigned int>(), T, k,
                       c->two_v, c->seed, c->node_tab.as<Slot>(),
                       (unsigned long long)(c->node_slots - 1), kProbeLimit, (long long)c->tok_base,
                       c->tok_slot.as<int>(), c->tok_dir.as<signed char>(),
                       c->status.as<unsigned long long>(), c->count_inline ? 1 : 0,
                       c->weak_fp_builds > 0 ? 0x00000FFF00000000ull : ~0ull);
  stage_end(c);

  stage_begin(c, "node_rank");
  AMGCHK(compact_table(c, c->node_tab, c->node_slots, ST_COMPACT_A, hs));
  stage_end(c);
  if (hs[ST_BADINPUT])
    return amg_fail(AMG_E_ARG, hs[ST_BADINPUT] == 1 ? "read_offsets must start at 0, never decrease and end at the token count"
                                                    : "a token lies outside [0, two_v)");
  if (hs[ST_PALINDROME])
    return amg_fail(AMG_E_PALINDROME, "Gene-mer and reverse complement gene-mer are identical");
  if (hs[ST_OVERFLOW]) return overflowed(which, OV_NODE_TABLE);
  c->n_windows = (int64_t)hs[ST_N_WINDOWS];
  c->n_short = (int64_t)hs[ST_N_SHORT];
  c->n_local_nodes = (int64_t)hs[ST_COMPACT_A];
  return AMG_OK;
}

int bs_nodes_rank_local(amg_ctx* c) {
  hipStream_t st = c->stream;
  stage_begin(c, "node_rank");
  c->packed_nodes = (c->two_v <= 65536 && c->k <= AMG_PACK_MAX_K);
  c->n_nodes = c->n_local_nodes;
  const long long D = c->n_nodes;
  int first_bits = ilog2_ceil((uint64_t)(c->tok_total > 0 ? c->tok_total : 1) * 2 + 2) + 1;
  const FpKeyList& keys = c->fp_keys;
  AMGCHK(fp_list_sort(c, keys, first_bits));
  AMGCHK(bs_alloc_nodes(c, D));
  if (D > 0)
    hipLaunchKernelGGL(k_assign_nodes, dim3(nblk(D, 256)), dim3(256), 0, st, keys.first_sorted, keys.slot_sorted, D,
                       c->node_tab.as<Slot>(), c->tokens.as<int>(), c->k, c->two_v,
                       (long long)c->tok_base, c->packed_nodes ? 1 : 0, c->node_tokens.as<int>(),
                       c->node_cov.as<unsigned int>(), c->node_first.as<long long>(),
                       c->node_alive.as<unsigned char>());
  stage_end(c);
  return AMG_OK;
}

// returns AMG_OK, or AMG_E_OVERFLOW with *which = OV_EDGE_TABLE / OV_COLLISION (fingerprint collision)
int bs_edges_pass(amg_ctx* c, Overflow* which) {
  *which = OV_NONE;
  hipStream_t st = c->stream;
  const long long T = c->n_tokens, D = c->n_nodes;
  const long long n_tiles = (T + TILE - 1) / TILE;
  unsigned long long hs[ST_WORDS];
  if (c->edge_slots < (int64_t)slots_for((uint64_t)D)) c->edge_slots = (int64_t)slots_for((uint64_t)D);
  if (!c->count_inline) AMGCHK(c->tok_pair.ensure((size_t)(T + 4) * sizeof(int)));
  AMGCHK(c->edge_tab.ensure((size_t)c->edge_slots * sizeof(Slot)));
  stage_begin(c, "edge_table_clear");
  HIPCHK(hipMemsetAsync(c->edge_tab.p, 0, (size_t)c->edge_slots * sizeof(Slot), st));
  HIPCHK(hipMemsetAsync(c->status.as<unsigned long long>() + ST_OVERFLOW, 0, sizeof(unsigned long long), st));
  HIPCHK(hipMemsetAsync(c->status.as<unsigned long long>() + ST_COMPACT_B, 0, sizeof(unsigned long long), st));
  stage_end(c);
  stage_begin(c, "edge_upsert");
  if (n_tiles > 0)
    hipLaunchKernelGGL(k_edges, dim3((unsigned)n_tiles), dim3(TILE_THREADS), 0, st,
                       c->tokens.as<int>(), T, c->k, c->two_v, c->node_tab.as<Slot>(),
                       c->node_tokens.as<int>(), c->tok_slot.as<int>(),
                       c->tok_dir.as<signed char>(), c->tok_node.as<int>(),
                       c->edge_tab.as<Slot>(), (unsigned long long)(c->edge_slots - 1),
                       kProbeLimit, 1, (long long)c->tok_base, c->status.as<unsigned long long>(),
                       c->count_inline ? 1 : 0, c->count_inline ? (int*)nullptr : c->tok_pair.as<int>(),
                       c->packed_nodes ? 1 : 0);
  stage_end(c);

  stage_begin(c, "edge_rank");
  AMGCHK(compact_table(c, c->edge_tab, c->edge_slots, ST_COMPACT_B, hs));
  stage_end(c);
  if (hs[ST_COLLISION]) return overflowed(which, OV_COLLISION);
  if (hs[ST_OVERFLOW]) return overflowed(which, OV_EDGE_TABLE);
  c->n_local_pairs = (int64_t)hs[ST_COMPACT_B];
  if (!c->count_inline && !c->dist_mode) {
    // node coverage (construct_node.py:33-36) from the per-window node ids
    stage_begin(c, "node_count");
    AMGCHK(count_ids(c, CountNodes, IdsPlain, c->tok_node.as<int>(), T, D, c->node_cov.as<unsigned int>()));
    stage_end(c);
  }
  return AMG_OK;
}

int bs_pairs_from_local(amg_ctx* c) {
  hipStream_t st = c->stream;
  stage_begin(c, "edge_rank");
  const long long P = c->n_local_pairs;
  c->n_pairs = P;
  AMGCHK(bs_alloc_pairs(c, P));
  int efirst_bits = ilog2_ceil((uint64_t)(c->tok_total > 0 ? c->tok_total : 1) * 8 + 8) + 1;
  const FpKeyList& keys = c->fp_keys;
  AMGCHK(fp_list_sort(c, keys, efirst_bits, c->pair_first.as<unsigned long long>()));
  if (P > 0)
    hipLaunchKernelGGL(k_gather_pairs, dim3(nblk(P, 256)), dim3(256), 0, st,
                       keys.slot_sorted, P, c->edge_tab.as<Slot>(),
                       c->pair_key.as<unsigned long long>(), c->pair_cnt.as<unsigned int>());
  stage_end(c);
  if (!c->count_inline && P > 0) {
    // edge-class coverage: pair ids into the table, then count the per-adjacency slots
    stage_begin(c, "edge_count");
    hipLaunchKernelGGL(k_set_pair_ids, dim3(nblk(P, 256)), dim3(256), 0, st,
                       keys.slot_sorted, P, c->edge_tab.as<Slot>());
    AMGCHK(count_ids(c, CountEdgeClasses, IdsPlain, c->tok_pair.as<int>(), c->n_tokens, P, c->pair_cnt.as<unsigned int>(),
                     c->edge_tab.as<Slot>()));
    stage_end(c);
  }
  return AMG_OK;
}
