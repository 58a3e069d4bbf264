// window_masks_check.cpp — the transitions of the live-window masks' state (WindowMasks, amg_state.h) on a bare amg_ctx
// on the stack, as a plain host program: `make -C amira_amd/csrc window_masks_check`, then ./window_masks_check_asan, by
// hand on a CPU.  No part of `all`, no device call, nothing of the library linked.  (state_check.cpp holds the other
// flags against the header's table; this one holds win_masks alone, from both of its states.)
//   1  every event from both states: Current only after the read walk of a removal, Absent after everything that writes
//      tok_node / read_fix or replaces the reads, kept by everything else
//   2  the sequences the entry points make of the events: the cleaning sweep, a filtered build, a second read set
#include <cstdio>
#include <cstdlib>

#include "amg_state.h"

#define CHECK(cond)                                                                          \
  do {                                                                                       \
    if (!(cond)) {                                                                           \
      fprintf(stderr, "window_masks_check: line %d: %s does not hold\n", __LINE__, #cond);  \
      exit(1);                                                                               \
    }                                                                                        \
  } while (0)

enum Event {
  READS_REPLACED, POSITIONS_CALLERS, POSITIONS_OWN, LENGTHS_SET, CORRECTED_BEGUN, MADE_TRIMS_ONLY, MADE_OTHER, ADOPTED,
  ADOPTED_COMPACTED, OFFER_TAKEN, BUILD_BEGINS, FROM_READS_SINGLE, FROM_READS_MERGED, GRAPH_IN_PLACE, GRAPH_DERIVED,
  REMOVAL_BEGINS, NODES_DIED, EDGE_DIED, LISTS_MADE, MATCH_BEGUN, MASKS_MADE, MASKS_VOID, N_EVENTS
};
static void apply(amg_ctx* c, int e) {
  switch (e) {
    case READS_REPLACED: ctx_reads_replaced(c, 7, 70, 20); break;
    case POSITIONS_CALLERS: ctx_positions_replaced(c, 70, false); break;
    case POSITIONS_OWN: ctx_positions_replaced(c, 70, true); break;
    case LENGTHS_SET: ctx_read_lengths_set(c); break;
    case CORRECTED_BEGUN: ctx_corrected_begun(c); break;
    case MADE_TRIMS_ONLY: ctx_corrected_made(c, 5, 50, 0, true, 300, nullptr); break;
    case MADE_OTHER: ctx_corrected_made(c, 5, 50, 0, false, 300, nullptr); break;
    case ADOPTED: ctx_corrected_adopted(c, false); break;
    case ADOPTED_COMPACTED: ctx_corrected_adopted(c, true); break;
    case OFFER_TAKEN: (void)ctx_take_derive_offer(c); break;
    case BUILD_BEGINS: (void)ctx_build_begins(c); break;
    case FROM_READS_SINGLE: ctx_build_from_reads(c, 3, false); break;
    case FROM_READS_MERGED: ctx_build_from_reads(c, 3, true); break;
    case GRAPH_IN_PLACE: ctx_graph_in_place(c, 1000, false); break;
    case GRAPH_DERIVED: ctx_graph_in_place(c, 1000, true); break;
    case REMOVAL_BEGINS: ctx_removal_begins(c); break;
    case NODES_DIED: live_lists_after_node_deaths(c); break;
    case EDGE_DIED: live_lists_after_edge_deaths(c); break;
    case LISTS_MADE: live_lists_made(c); break;
    case MATCH_BEGUN: ctx_match_begun(c); break;
    case MASKS_MADE: window_masks_made(c); break;
    case MASKS_VOID: window_masks_void(c); break;
  }
}
static WindowMasks expected(int e, WindowMasks was) {
  switch (e) {
    case MASKS_MADE: return WindowMasks::Current;
    case READS_REPLACED: case ADOPTED: case ADOPTED_COMPACTED: case BUILD_BEGINS: case GRAPH_IN_PLACE: case GRAPH_DERIVED:
    case MASKS_VOID:
      return WindowMasks::Absent;
    default: return was;  // (the flags of a removal alone change nothing: the read walk that follows them does)
  }
}

int main() {
  long long n = 0;
  for (int e = 0; e < N_EVENTS; ++e)
    for (int had_pos = 0; had_pos < 2; ++had_pos)
      for (WindowMasks was : {WindowMasks::Absent, WindowMasks::Current}) {
        amg_ctx c;
        c.have_pos = had_pos != 0;
        c.win_masks = was;
        apply(&c, e);
        CHECK(c.win_masks == expected(e, was));
        ++n;
      }
  {
    amg_ctx c;
    CHECK(c.win_masks == WindowMasks::Absent);  // a new ctx has none
    // the cleaning sweep: reads, build, filter (its read walk), correct, adopt, derived rebuild, clip, correct, adopt, build
    ctx_reads_replaced(&c, 7, 70, 20);
    (void)ctx_build_begins(&c);
    ctx_build_from_reads(&c, 3, false);
    ctx_graph_in_place(&c, 100, false);
    CHECK(c.win_masks == WindowMasks::Absent);
    ctx_removal_begins(&c);
    live_lists_after_node_deaths(&c);
    CHECK(c.win_masks == WindowMasks::Absent);  // (not before the walk has run)
    window_masks_made(&c);
    CHECK(c.win_masks == WindowMasks::Current);
    // a second removal walks every read again; an edge removal walks none and leaves the masks of tok_node as it is
    ctx_removal_begins(&c);
    live_lists_after_node_deaths(&c);
    window_masks_made(&c);
    ctx_removal_begins(&c);
    live_lists_after_edge_deaths(&c);
    CHECK(c.win_masks == WindowMasks::Current);
    ctx_corrected_begun(&c);
    ctx_corrected_made(&c, 5, 50, 0, true, 90, nullptr);
    CHECK(c.win_masks == WindowMasks::Current);  // (a correction reads tok_node: a second one may take the masks too)
    ctx_corrected_adopted(&c, false);
    CHECK(c.win_masks == WindowMasks::Absent);   // the reads are others now
    window_masks_made(&c);                        // (were something to make them between adoption and build ...)
    (void)ctx_build_begins(&c);                   // ... the build voids them at its first step: tok_node is its to write
    CHECK(c.win_masks == WindowMasks::Absent);
    window_masks_made(&c);
    ctx_graph_in_place(&c, 90, true);             // the derived rebuild swaps tok_node
    CHECK(c.win_masks == WindowMasks::Absent);
    // a filtered build flags its dead reads itself, without a read walk: flags, no masks
    (void)ctx_build_begins(&c);
    ctx_build_from_reads(&c, 3, false);
    ctx_graph_in_place(&c, 100, false);
    ctx_corrected_begun(&c);
    CHECK(c.win_masks == WindowMasks::Absent);
    // a merged build
    window_masks_made(&c);
    (void)ctx_build_begins(&c);
    ctx_build_from_reads(&c, 3, true);
    CHECK(c.win_masks == WindowMasks::Absent);
    ctx_graph_in_place(&c, 100, false);
    CHECK(c.win_masks == WindowMasks::Absent);
    // another read set on the same ctx
    window_masks_made(&c);
    ctx_reads_replaced(&c, 3, 30, 20);
    CHECK(c.win_masks == WindowMasks::Absent);
  }
  printf("window_masks_check: %lld transitions and the sequences passed\n", n);
  return 0;
}
