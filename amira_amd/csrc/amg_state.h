// amg_state.h — what a ctx currently holds: one function per EVENT; the flags below are assigned nowhere else
// (amg_nw_probe.hip alone saves and restores the position flags around its test probe).  Host only: flags and plain
// counters, no device call, no buffer — state_check.cpp drives every function on a bare amg_ctx.  Flags that say "X has
// been made" (comp_valid, adj_valid, match_valid, have_routes) are SET by X's maker and CLEARED only here.
//
// The table: what the event does to the flag; empty = kept.
//                  reads     positions  lengths  corrected  corrected  corrected  build    build from  graph in   removal  nodes      edge     lists
//                  replaced  replaced   set      begun      made       adopted    begins   reads       place      begins   died       died     made
//  built           cleared                                             cleared    cleared              set
//  have_pos        cleared   set
//  have_read_len   cleared   cleared    set
//  pos_identity              set                                       from (1)
//  pos0_own                  from arg                                  from (1)
//  have_corrected  cleared   cleared             cleared    set        cleared    cleared                         cleared
//  c_derivable                                   cleared    from (2)   cleared
//  derive_ready    cleared                                             from (3)   cleared
//  dist_candidate  cleared                                             from (4)   cleared
//  derived                                                                        cleared              from arg
//  edge_own_deaths                                                                                     cleared                        set
//  pristine                                                                                            from (5)            cleared    cleared
//  comp_valid, adj_valid                                                                               cleared
//  match_valid     cleared                                             cleared    cleared                                  cleared    cleared
//  live_lists                                                                                          Absent              from (6)   Absent   Current
//  win_masks       Absent                                              Absent     Absent               Absent              (11)
//  cnt_hint_reset  set
//  node_hint       0                                                   from (7)            from (8)    from (9)
//  hint_bound      0 (10)                                                                  0 (8)
//  c_node_bound                                             from arg   0
//  (1) with positions: compacted — both set (pool 0 is the engine's own gather); not compacted — pos_identity cleared (the
//      reads point into pool 0 and the pool of produced positions), pos0_own kept
//  (2) the caller's verdict (nothing re-threaded, no read kept around a dead window; a selection: never) and no edge_own_deaths
//  (3) c_derivable: the offer of the derived rebuild, taken or declined by the next build (ctx_take_derive_offer)
//  (4) dist_mode: a rank of a merged build asks the other ranks whatever ITS correction did
//  (5) not comp_from_claims: a filtered build's labels are those of the graph BEFORE its filter
//  (6) Current becomes BehindNodes (Absent with AMG_NO_LADJ_PATCH=1), the other two stay
//  (7) the correction's bound where it was made for this k and is below the hint (or there is none), at least 256
//  (8) single build only: hint_bound where it was made for this k, at least 256, and used up
//  (9) the nodes the build saw, at least 256
//  (10) amg_set_reads_from_corrected then sets hint_bound / hint_bound_k from the source's c_node_bound
//  (11) a removal's read walk (k_mask_reads over every read, apply_removals) makes them Current: window_masks_made; a
//      removal that walks no reads (amg_remove_edges, a clip that finds nothing) leaves them as they are
//  And: a new search of amg_match_patterns clears match_valid (ctx_match_begun); amg_count.hip takes cnt_hint_reset.
#pragma once
#include <cstdlib>

#include "amg_internal.h"

static inline int64_t ctx_hint_floor(int64_t n) { return n > 256 ? n : 256; }

// ---- 0. the live-window masks of the reads (WindowMasks, amg_internal.h).  Made by the read walk of a removal, which
// visits every read and is then the last writer of tok_node; void as soon as anything else writes tok_node or read_fix
// or the reads change: new reads, an adopted correction, a build from its first step (tok_node is scratch of a merged
// build's node pass) to the graph in place (plain, filtered — whose dead-read flags have no masks —, merged, derived)
static inline void window_masks_made(amg_ctx* c) { c->win_masks = WindowMasks::Current; }
static inline void window_masks_void(amg_ctx* c) { c->win_masks = WindowMasks::Absent; }

// ---- 1. a read set arrives from outside (amg_set_reads, amg_build_multi's borrowers, amg_set_reads_from_corrected's dst)
static inline void ctx_reads_replaced(amg_ctx* c, int64_t n_reads, int64_t n_tokens, int32_t two_v) {
  c->n_reads = n_reads, c->n_tokens = n_tokens, c->two_v = two_v;
  c->have_pos = c->have_read_len = false;
  c->built = c->have_corrected = c->match_valid = false;
  c->derive_ready = c->dist_candidate = false;
  c->node_hint = c->hint_bound = 0;
  c->cnt_hint_reset = true;  // what the counting sweeps learned belongs to the previous read set
  window_masks_void(c);
}

// ---- 2. positions arrive.  own: pool 0 is the engine's own gather, not arrays a caller holds (amg_get_corrected32)
static inline void ctx_positions_replaced(amg_ctx* c, int64_t n_tokens, bool own) {
  c->have_pos = c->pos_identity = true;
  c->pos0_own = own;
  c->pos_n0 = n_tokens;
  c->pos1_used = c->c_pos1_used = 0;
  c->have_corrected = c->have_read_len = false;
}
static inline void ctx_read_lengths_set(amg_ctx* c) { c->have_read_len = true; }

// ---- 3. a corrected set is begun / made (amg_correct_reads, amg_select_reads)
static inline void ctx_corrected_begun(amg_ctx* c) { c->have_corrected = c->c_derivable = false; }
// only_drops_and_trims: note (2); bound: the nodes the graph of the set can have at this k; test_bound: AMG_TEST_NODE_BOUND
// as the caller read it (a bound that does not hold) or null
static inline void ctx_corrected_made(amg_ctx* c, int64_t reads, int64_t tokens, int64_t pos1_used, bool only_drops_and_trims,
                                      int64_t bound, const char* test_bound) {
  c->c_reads = reads, c->c_tokens = tokens;
  c->c_pos1_used = pos1_used;  // becomes current with amg_adopt_corrected
  c->c_derivable = only_drops_and_trims && !c->edge_own_deaths;
  c->c_node_bound = test_bound ? atoll(test_bound) : bound;
  c->c_node_bound_k = c->k;
  c->have_corrected = true;
}

// ---- 4. the corrected set becomes the read set: the flag half of amg_adopt_corrected (compacted: it has gathered the
// positions into flat arrays of the engine's own, and the pool of produced positions starts empty again)
static inline void ctx_corrected_adopted(amg_ctx* c, bool compacted) {
  c->derive_ready = c->c_derivable;  // (the graph the reads were corrected against is still in place: amg_build may reuse it)
  c->dist_candidate = c->dist_mode;  // (a rank of a merged build: the ranks decide together, amg_dist.hip S_DV_*)
  if (c->have_pos && compacted) {
    c->pos0_own = c->pos_identity = true;
    c->pos_n0 = c->c_tokens;
    c->pos1_used = c->c_pos1_used = 0;
  } else if (c->have_pos) {
    c->pos_identity = false;
    c->pos1_used = c->c_pos1_used;
  }
  c->n_reads = c->c_reads, c->n_tokens = c->c_tokens;
  c->c_derivable = c->have_corrected = c->built = c->match_valid = false;
  window_masks_void(c);
  // the next build's node table: not larger than the correction's bound asks for (a graph of uncorrected reads is
  // mostly error nodes that do not come back: 5.4 M nodes before, 0.5 M after on BASELINE config 3).  A build with
  // another k, or a bound that does not hold, costs what any undersized table costs: one repeated pass.
  if (c->c_node_bound > 0 && c->c_node_bound_k == c->k && (c->node_hint == 0 || c->c_node_bound < c->node_hint))
    c->node_hint = ctx_hint_floor(c->c_node_bound);
  c->c_node_bound = 0;
}

// ---- 5. a build begins.  The offer of the derived rebuild is good once: whoever asks uses it up (amg_build; every rank
// of a merged build, amg_dist.hip).  Returns whether the reads are what a correction left of the reads of the graph held
static inline bool ctx_take_derive_offer(amg_ctx* c) {
  const bool offered = c->derive_ready;
  c->derive_ready = c->dist_candidate = false;
  return offered;
}
// single and merged builds alike; returns ctx_take_derive_offer.  The graph at hand stays as it is (arrays, counts, k,
// dist_mode): a derive reads it
static inline bool ctx_build_begins(amg_ctx* c) {
  c->derived = c->built = c->have_corrected = c->match_valid = false;
  c->retries = c->tok_base = 0;
  c->tok_total = c->n_tokens;
  window_masks_void(c);
  return ctx_take_derive_offer(c);
}
// ... and goes on from the reads (no derive, or the derive declined)
static inline void ctx_build_from_reads(amg_ctx* c, int32_t k, bool merged) {
  c->k = k;
  c->dist_mode = merged;
  c->comp_from_claims = false;
  if (!merged && c->hint_bound > 0) {  // reads taken over from another ctx's correction: its bound holds at ITS gene-mer size
    if (c->hint_bound_k == k) c->node_hint = ctx_hint_floor(c->hint_bound);
    c->hint_bound = 0;
  }
}

// ---- 6. a graph is in place (amg_build, derive_commit, the last step of a merged build).  seen: the nodes the build saw —
// of a filtered build those before its filter: the next table is sized by what the pass meets
static inline void ctx_graph_in_place(amg_ctx* c, int64_t seen, bool derived) {
  c->live_lists = LiveLists::Absent;  // there are no lists of this graph
  window_masks_void(c);               // ... and no masks of its tok_node
  c->pristine = !c->comp_from_claims;
  c->edge_own_deaths = c->comp_valid = c->adj_valid = false;
  c->n_components = 0;
  c->built = true;
  c->derived = derived;
  c->node_hint = ctx_hint_floor(seen);
}

// ---- 7. the graph loses something.  A removing call has passed its argument checks: the corrected set no longer belongs to
// this graph, whatever the call goes on to remove (a clip or a walk that finds nothing drops it too; an empty id list
// returns before this)
static inline void ctx_removal_begins(amg_ctx* c) { c->have_corrected = false; }
// nodes died, and every edge that died with them has a dead end: lists that exist are kept and brought up to date
// (k_lr_patch) when somebody walks them again (AMG_NO_LADJ_PATCH=1: they are made again; A/B + test switch)
static inline void live_lists_after_node_deaths(amg_ctx* c) {
  if (c->live_lists == LiveLists::Current)
    c->live_lists = getenv("AMG_NO_LADJ_PATCH") ? LiveLists::Absent : LiveLists::BehindNodes;
  c->pristine = c->match_valid = false;  // (node-id patterns of a cached K6 result may name removed nodes)
}
// an edge died with both its ends alive (a coverage threshold above 1, amg_remove_edges): the lists are made again
static inline void live_lists_after_edge_deaths(amg_ctx* c) {
  c->live_lists = LiveLists::Absent;
  c->edge_own_deaths = true;
  c->pristine = c->match_valid = false;
}
static inline void live_lists_made(amg_ctx* c) { c->live_lists = LiveLists::Current; }  // ensure_live_adj, made or patched
static inline void ctx_match_begun(amg_ctx* c) { c->match_valid = false; }  // amg_match_patterns starts a new search
