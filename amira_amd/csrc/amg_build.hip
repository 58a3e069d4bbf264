// amg_build.hip — the driver of a build (GeneMerGraph.__init__, reference construct_graph.py:31-102): the entry points
// amg_build / amg_build_filtered / amg_build_multi / amg_finalize, the environment switches, table sizing and growth after
// an overflow, and the stages that every key scheme shares (read statistics, the node and edge-class arrays, the edge
// emission).  No kernel of a table pass lives here.
//
// The build is split into stages so that the multi-GPU path (amg_dist*.hip) can put its exchanges between them:
//   read statistics      bs_read_stats, here
//   nodes, edge classes  by key scheme (build_impl chooses, bx_applicable):
//     exact tuple keys, or verified 94-bit fingerprints of a tuple that does not fit, in 16-byte slots with claim ids:
//       amg_build_x.hip         the table passes (bx_nodes_upsert, bx_edges_upsert)
//       amg_build_x_claims.hip  per claim: coverage, the fused filter, ranking; bx_nodes / bx_nodes_filtered, bx_edges
//       amg_build_x_comp.hip    a filtered build's components and touched reads
//     verified 64-bit fingerprints in 32-byte slots (2^29 tokens and more, a merged build whose tuple does not fit a slot,
//     AMG_KEY_MODE=fp, AMG_COUNT_INLINE, a fitting tuple under the weak-fingerprint hook):
//       amg_build_fp.hip bs_nodes_pass        local windows -> local node table (+ its key list, ctx->fp_keys)
//                        bs_nodes_rank_local  single GPU: node ids from the key list, sorted by first-seen (fp_list_sort)
//                        bs_edges_pass        local adjacencies -> local edge-class table (+ its key list)
//                        bs_pairs_from_local  single GPU: edge classes in first-seen order as arrays, from the key list
//   coverage             amg_count.hip (count_ids), called by the node / edge-class stage of each scheme
//   directed edges       bs_finish_from_pairs, here (the scan that emits them: amg_scan.hip)
//   components, adjacency lists: on first use, amg_adjacency.hip (ensure_components / ensure_adjacency)
#include "amg_device.h"

#include "amg_tile.h"

uint64_t pow2_at_least(uint64_t x) {
  uint64_t p = 1024;
  while (p < x) p <<= 1;
  return p;
}

// window / short-read counts into the status words + the read-end bitmap the tile kernels use
int bs_read_stats(amg_ctx* c, int k, const ClearList* also) {
  hipStream_t st = c->stream;
  const long long T = c->n_tokens, R = c->n_reads;
  stage_begin(c, "read_stats");
  const size_t words = (size_t)(T >> 5) + BND_PAD_WORDS;
  AMGCHK(c->bnd_bits.ensure(words * sizeof(unsigned int)));
  {  // the read-end bitmap and whatever else the caller wants zeroed before its table pass: one launch
    ClearList cl;
    if (also) cl = *also;
    cl.add(c->bnd_bits.p, words * sizeof(unsigned int));
    AMGCHK(clear_many(c, cl));
  }
  if (R > 0)
    hipLaunchKernelGGL(k_read_stats, dim3(nblk(R, 256) < 512u ? nblk(R, 256) : 512u), dim3(256), 0, st,
                       c->read_off.as<long long>(), R, T, k, c->status.as<unsigned long long>(),
                       c->bnd_bits.as<unsigned int>());
  stage_end(c);
  return AMG_OK;
}

int bs_alloc_nodes(amg_ctx* c, long long D) {
  AMGCHK(c->node_tokens.ensure((size_t)(D * c->k + 1) * sizeof(int)));
  AMGCHK(c->node_cov.ensure((size_t)(D + 1) * sizeof(unsigned int)));
  AMGCHK(c->node_first.ensure((size_t)(D + 1) * sizeof(long long)));
  AMGCHK(c->node_comp.ensure((size_t)(D + 1) * sizeof(int)));
  AMGCHK(c->node_alive.ensure((size_t)(D + 1)));
  return AMG_OK;
}

int bs_alloc_pairs(amg_ctx* c, long long P) {
  AMGCHK(c->pair_key.ensure((size_t)(P + 2) * sizeof(unsigned long long)));
  AMGCHK(c->pair_first.ensure((size_t)(P + 2) * sizeof(unsigned long long)));
  AMGCHK(c->pair_cnt.ensure((size_t)(P + 2) * sizeof(unsigned int)));
  return AMG_OK;
}

// pair_key / pair_cnt / pair_first hold the c->n_pairs edge classes in first-seen order: directed
// edges in _edges order.  Component ids and the forward / backward edge lists are made when
// somebody asks for them (ensure_components / ensure_adjacency; amg_finalize does both): of the three
// graphs of a cleaning sweep only the second needs its components (tip clipping) and none needs the
// lists of removed edges — the correction walks the LIVE adjacency, built from the live edges alone.
int bs_finish_from_pairs(amg_ctx* c) {
  const long long P = c->n_pairs, R = c->n_reads;
  stage_begin(c, "edge_emit");
  AMGCHK(c->s5.ensure((size_t)(P + 2) * sizeof(long long)));
  long long* base = c->s5.as<long long>();
  // at most two directed edges per class: the arrays are sized before the exact count is known
  const long long cap = 2 * P;
  AMGCHK(c->edge_src.ensure((size_t)(cap + 2) * sizeof(int)));
  AMGCHK(c->edge_tgt.ensure((size_t)(cap + 2) * sizeof(int)));
  AMGCHK(c->edge_sdir.ensure((size_t)(cap + 2)));
  AMGCHK(c->edge_tdir.ensure((size_t)(cap + 2)));
  AMGCHK(c->edge_cov.ensure((size_t)(cap + 2) * sizeof(unsigned int)));
  AMGCHK(c->edge_alive.ensure((size_t)(cap + 2)));
  AMGCHK(c->read_fix.ensure((size_t)R + 1));
  long long total = 0;
  {
    ClearList cl;  // (zeroed by the scan's workgroups)
    cl.add(c->read_fix.p, (size_t)R + 1);
    if (P > 0) {
      // a class is one directed edge (self-loop) or two: the scan that sums the widths writes the edges at their
      // places (base[P] = the number of directed edges)
      AMGCHK(prim_exscan_emit_edges(c, c->pair_key.as<unsigned long long>(), c->pair_cnt.as<unsigned int>(),
                                    c->pair_first.as<unsigned long long>(), (size_t)P, base + P, c->edge_src.as<int>(),
                                    c->edge_tgt.as<int>(), c->edge_sdir.as<signed char>(), c->edge_tdir.as<signed char>(),
                                    c->edge_cov.as<unsigned int>(), c->edge_alive.as<unsigned char>(), &cl));
    } else {
      AMGCHK(clear_many(c, cl));
    }
  }
  {  // the build's final synchronisation; the done flags of its counting sweeps ride along
    FetchList l;
    l.add(P > 0 ? static_cast<const void*>(base + P) : c->status.p);
    const bool learn = count_learn_add(c, &l);
    unsigned long long v[1 + COUNT_LEARN_WORDS] = {0};
    AMGCHK(fetch(c, l, v));
    if (P > 0) total = (long long)v[0];
    if (learn) count_learn_take(c, v + 1);
  }
  c->n_edges = total;
  stage_end(c);
  return AMG_OK;  // (the caller says that a graph is in place: ctx_graph_in_place)
}

extern "C" int amg_finalize(amg_ctx* c) {
  if (!c) return amg_fail(AMG_E_ARG, "null ctx");
  if (!c->built) return amg_fail(AMG_E_STATE, "amg_build first");
  HIPCHK(hipSetDevice(c->device));
  stages_reset(c);
  AMGCHK(ensure_components(c));
  AMGCHK(ensure_adjacency(c));
  HIPCHK(hipStreamSynchronize(c->stream));
  return AMG_OK;
}

// Slots for n expected keys.  All 64 lanes of a wave wait for the longest probe chain among
// them, so a low load factor pays even when every probe is an L2 hit (measured on 20 000 hot
// keys: 0.99 ms per pass at load 0.31, 0.67 ms at 0.02): 32 slots per key while that stays
// within 4 M slots (a 64 MB table clears in ~25 us), never less than 3 per key.
uint64_t slots_for(uint64_t n) {
  const uint64_t lo = n * 3, hi = n * 32, cap = 4ull << 20;
  const uint64_t want = hi < cap ? hi : cap;
  return pow2_at_least(want > lo ? want : lo);
}

// table sizing: previous distinct-node count when known, otherwise the window bound
void bs_size_tables(amg_ctx* c) {
  // no history: a quarter of a slot per token.  Real gene-call data repeat every gene-mer tens to
  // thousands of times, so this is already generous; inputs with more distinct gene-mers than
  // that overflow once (cheaply, see table_upsert's abort flag) and are rebuilt 4x larger.
  uint64_t want = c->node_hint > 0 ? slots_for((uint64_t)c->node_hint) : (uint64_t)c->n_tokens / 4;
  c->node_slots = (int64_t)pow2_at_least(want);
  if (c->node_slots > (1ll << 30)) c->node_slots = 1ll << 30;
  c->edge_slots = 1024;
}

BuildSwitches read_build_switches() {
  BuildSwitches sw;
  auto is_zero = [](const char* v) { return v && atoi(v) == 0; };
  if (const char* e = getenv("AMG_X_HEAD_TILES")) sw.head_tiles_set = true, sw.head_tiles = atoll(e);
  if (const char* e = getenv("AMG_CLAIM_SHARDS")) sw.claim_shards = atoi(e) != 0;
  sw.tight_bits = getenv("AMG_X_TIGHT_BITS") != nullptr;
  if (const char* e = getenv("AMG_KEY_MODE")) sw.key_fp = e[0] == 'f';
  sw.node_buckets = !is_zero(getenv("AMG_NODE_BUCKETS"));
  sw.generic_k = getenv("AMG_X_GENERIC_K") != nullptr;
  if (const char* e = getenv("AMG_EDGE_LONE")) sw.edge_lone = atoi(e) != 0;
  sw.edge_home = !is_zero(getenv("AMG_EDGE_HOME"));
  sw.no_derive = getenv("AMG_NO_DERIVE") != nullptr;
  if (const char* e = getenv("AMG_TEST_WEAK_FP")) sw.weak_fp = atoi(e);
  if (const char* e = getenv("AMG_COUNT_INLINE")) sw.count_inline = e[0] == '1';
  if (const char* e = getenv("AMG_COUNT_LIST_SEG")) sw.count_list_seg = atoi(e);
  sw.count_debug = getenv("AMG_COUNT_DEBUG") != nullptr;
  return sw;
}

// what the next attempt changes after a table pass returned AMG_E_OVERFLOW for `cause`
int grow_after_overflow(amg_ctx* c, Overflow cause) {
  ++c->retries;
  if (cause == OV_NODE_TABLE) {
    if (c->node_slots >= (1ll << 30)) return amg_fail(AMG_E_OVERFLOW, "node table at maximum size");
    c->node_slots = c->node_slots * 4 > (1ll << 30) ? (1ll << 30) : c->node_slots * 4;
  } else if (cause == OV_EDGE_TABLE) {
    c->edge_slots *= 4;
  } else {
    c->seed = c->seed * 6364136223846793005ull + 1442695040888963407ull;  // new fingerprint
    if (c->weak_fp_builds > 0) --c->weak_fp_builds;
  }
  return AMG_OK;
}

static int build_impl(amg_ctx* c, int32_t k, uint32_t min_node_cov, uint32_t min_edge_cov, bool* fused) {
  *fused = false;
  if (!c) return amg_fail(AMG_E_ARG, "null ctx");
  if (k < 1 || k > AMG_MAX_K) return amg_fail(AMG_E_ARG, "k must be in [1, %d]", AMG_MAX_K);
  if (c->two_v <= 0) return amg_fail(AMG_E_STATE, "amg_set_reads first");
  HIPCHK(hipSetDevice(c->device));
  stages_reset(c);
  c->sw = read_build_switches();
  // the reads are what the last correction left of the reads of the graph still held, nothing re-threaded: that graph's
  // live part IS the graph to build (amg_derive.hip; AMG_NO_DERIVE=1: A/B + test switch)
  // The derive stands between the two halves of "a build begins": it still needs the k and dist_mode of the graph at
  // hand (to decide, and to squeeze that graph), and a derived graph keeps them
  const bool derive = ctx_build_begins(c) && k == c->k && !c->dist_mode && !c->sw.no_derive;
  if (derive) {
    bool done = false;
    AMGCHK(derive_from_previous(c, k, &done));
    if (done) return AMG_OK;  // (amg_build_filtered goes on with amg_filter)
  }
  ctx_build_from_reads(c, k, false);
  // test hook: the first AMG_TEST_WEAK_FP attempts use a 12-bit fingerprint, which is
  // certain to collide; the exact verification must catch it and the retry must succeed
  c->weak_fp_builds = c->sw.weak_fp;
  c->count_inline = c->sw.count_inline;  // A/B switch: 1 = one global atomic per window
  bs_size_tables(c);
  c->exact_keys = false;
  const bool exact = bx_applicable(c, k);  // 16-byte slots: exact tuple keys or verified 94-bit fingerprints, claim ids
  for (int attempt = 0; attempt < 12; ++attempt) {
    Overflow which = OV_NONE;
    int r;
    if (exact && min_node_cov > 0) {
      r = bx_nodes_filtered(c, k, min_node_cov, &which);
      if (r == AMG_OK) r = bx_edges(c, &which, PassCaller::FilteredBuild, min_edge_cov);
      *fused = true;
    } else if (exact) {
      r = bx_nodes(c, k, &which);
      if (r == AMG_OK) r = bx_edges(c, &which, PassCaller::PlainBuild, 0);
    } else {
      r = bs_nodes_pass(c, k, &which);
      if (r == AMG_OK) r = bs_nodes_rank_local(c);
      if (r == AMG_OK) r = bs_edges_pass(c, &which);
      if (r == AMG_OK) r = bs_pairs_from_local(c);
    }
    if (r == AMG_OK) r = bs_finish_from_pairs(c);
    if (r == AMG_OK && *fused) r = bx_flag_dead_reads(c);
    if (r == AMG_OK) {
      // (a filtered build keeps only the survivors: the next table is sized by what the pass saw)
      ctx_graph_in_place(c, *fused ? c->n_local_nodes : c->n_nodes, false);
      return AMG_OK;
    }
    if (r != AMG_E_OVERFLOW || which == OV_NONE) return r;
    AMGCHK(grow_after_overflow(c, which));
  }
  return amg_fail(AMG_E_OVERFLOW, "build did not converge after 12 attempts");
}

extern "C" int amg_build(amg_ctx* c, int32_t k) {
  bool fused = false;
  return build_impl(c, k, 0, 0, &fused);
}

// GeneMerGraph.__init__ followed by filter_graph(min_node_cov, min_edge_cov) (graph_utils.py:147-149 — what every
// cleaning iteration does with a freshly built graph).  On the exact-key path the filter is applied ON THE WAY:
// nodes below the threshold never get an id, an array entry or an edge (an uncorrected graph is ~99 % such
// nodes), their windows read None and their reads are queued for correction — the state a caller of
// amg_build + amg_filter finds, except that ids number the survivors only (first-seen order among them).
// Elsewhere (fingerprint keys) it IS amg_build + amg_filter.
extern "C" int amg_build_filtered(amg_ctx* c, int32_t k, uint32_t min_node_cov, uint32_t min_edge_cov) {
  bool fused = false;
  const int r = build_impl(c, k, min_node_cov < 1 ? 1 : min_node_cov, min_edge_cov < 1 ? 1 : min_edge_cov, &fused);
  if (r != AMG_OK || fused) return r;
  return amg_filter(c, min_node_cov, min_edge_cov);
}

// ------------------------------------------------------------------ several k over one read set
// choose_kmer_size (graph_utils.py:258-296) builds the graph of the SAME reads for k = 3, 5, ..., 15.  amg_build_multi
// puts the reads on the device ONCE — graph i's ctx borrows the first ctx's token arrays — and builds every graph with
// the ordinary amg_build on its own ctx, one after the other on the first ctx's stream.  (Rounds 2-5 also staged every
// tile of tokens once for the node passes of all k and once for their edge passes, k_node_upsert_multi / k_edges_multi:
// measured on cfg 3, `multi_k` in bench.py, the seven graphs took 28.2 ms that way and 28.0 ms as seven builds — the
// table work of a pass, not the reading of the tokens, is what a build costs — so those kernels are gone.)
#define MULTI_MAX 8
extern "C" int amg_build_multi(amg_ctx* const* ctxs, const int32_t* ks, int32_t n) {
  if (!ctxs || !ks || n < 1 || n > MULTI_MAX) return amg_fail(AMG_E_ARG, "amg_build_multi: 1 .. %d graphs", MULTI_MAX);
  amg_ctx* c0 = ctxs[0];
  if (!c0 || c0->two_v <= 0) return amg_fail(AMG_E_STATE, "amg_set_reads on the first ctx first");
  for (int i = 0; i < n; ++i) {
    if (!ctxs[i]) return amg_fail(AMG_E_ARG, "null ctx");
    if (ctxs[i]->device != c0->device) return amg_fail(AMG_E_ARG, "amg_build_multi: one device");
    if (ks[i] < 1 || ks[i] > AMG_MAX_K) return amg_fail(AMG_E_ARG, "k must be in [1, %d]", AMG_MAX_K);
    for (int j = 0; j < i; ++j)
      if (ctxs[j] == ctxs[i]) return amg_fail(AMG_E_ARG, "amg_build_multi: one ctx per graph");
  }
  HIPCHK(hipSetDevice(c0->device));
  HIPCHK(hipStreamSynchronize(c0->stream));
  const long long T = c0->n_tokens, R = c0->n_reads;
  // the other graphs read the first ctx's token arrays (borrowed: nothing is copied) and, for the length of this
  // call, work on its stream
  std::vector<hipStream_t> own(n);
  for (int i = 0; i < n; ++i) {
    amg_ctx* c = ctxs[i];
    own[i] = c->stream;
    if (i == 0) continue;
    HIPCHK(hipStreamSynchronize(c->stream));
    c->tokens.borrow(c0->tokens.p, (size_t)T * sizeof(int32_t));
    c->read_off.borrow(c0->read_off.p, (size_t)(R + 1) * sizeof(int64_t));
    ctx_reads_replaced(c, R, T, c0->two_v);
    c->stream = c0->stream;
  }
  struct Restore {
    amg_ctx* const* ctxs;
    std::vector<hipStream_t>& own;
    int n;
    ~Restore() {
      for (int i = 0; i < n; ++i) ctxs[i]->stream = own[i];
    }
  } restore{ctxs, own, n};
  for (int i = 0; i < n; ++i) AMGCHK(amg_build(ctxs[i], ks[i]));
  HIPCHK(hipStreamSynchronize(c0->stream));
  return AMG_OK;
}
