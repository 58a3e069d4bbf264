// state_check.cpp — the transitions of amg_state.h on a bare amg_ctx on the stack, held against the header's table, as a
// plain host program: `make -C amira_amd/csrc state_check`, then ./state_check_asan, by hand on a CPU.  No part of `all`,
// no device call, nothing of the library linked.
//   1  every event from every combination of the flags (and of what the "from" cells read): the whole flag set afterwards
//      is what the table below says — a second statement of amg_state.h's table, as data
//   2  the hints and counters, and the sequences that entry points make of the events
#include <cstdio>
#include <cstdlib>

#include "amg_state.h"

#define CHECK(cond)                                                                   \
  do {                                                                                \
    if (!(cond)) {                                                                    \
      fprintf(stderr, "state_check: line %d: %s does not hold\n", __LINE__, #cond);  \
      exit(1);                                                                        \
    }                                                                                 \
  } while (0)

// ------------------------------------------------------------------ the flags as one word
enum Flag {
  BUILT, HAVE_POS, HAVE_READ_LEN, POS_IDENTITY, POS0_OWN, HAVE_CORRECTED, C_DERIVABLE, DERIVE_READY, DIST_CANDIDATE, DERIVED,
  EDGE_OWN_DEATHS, PRISTINE, COMP_VALID, ADJ_VALID, MATCH_VALID, CNT_HINT_RESET, N_FLAGS,
  DIST_MODE = N_FLAGS, COMP_FROM_CLAIMS, N_BITS  // read by "from" cells, changed by no event but "build from reads"
};
static const char* kFlagName[N_FLAGS] = {"built", "have_pos", "have_read_len", "pos_identity", "pos0_own", "have_corrected",
                                         "c_derivable", "derive_ready", "dist_candidate", "derived", "edge_own_deaths",
                                         "pristine", "comp_valid", "adj_valid", "match_valid", "cnt_hint_reset"};

static bool* flag_of(amg_ctx* c, int f) {
  bool* p[N_BITS] = {&c->built, &c->have_pos, &c->have_read_len, &c->pos_identity, &c->pos0_own, &c->have_corrected,
                     &c->c_derivable, &c->derive_ready, &c->dist_candidate, &c->derived, &c->edge_own_deaths, &c->pristine,
                     &c->comp_valid, &c->adj_valid, &c->match_valid, &c->cnt_hint_reset, &c->dist_mode, &c->comp_from_claims};
  return p[f];
}
static void put(amg_ctx* c, unsigned bits, LiveLists lists) {
  for (int f = 0; f < N_BITS; ++f) *flag_of(c, f) = (bits >> f) & 1u;
  c->live_lists = lists;
}
static unsigned get(amg_ctx* c) {
  unsigned bits = 0;
  for (int f = 0; f < N_BITS; ++f) bits |= (*flag_of(c, f) ? 1u : 0u) << f;
  return bits;
}

// ------------------------------------------------------------------ the events
enum Event {
  READS_REPLACED, POSITIONS_CALLERS, POSITIONS_OWN, LENGTHS_SET, CORRECTED_BEGUN, MADE_TRIMS_ONLY, MADE_OTHER, ADOPTED,
  ADOPTED_COMPACTED, OFFER_TAKEN, BUILD_BEGINS, FROM_READS_SINGLE, FROM_READS_MERGED, GRAPH_IN_PLACE, GRAPH_DERIVED,
  REMOVAL_BEGINS, NODES_DIED, EDGE_DIED, LISTS_MADE, MATCH_BEGUN, N_EVENTS
};
static const char* kEventName[N_EVENTS] = {"reads replaced", "positions replaced (caller's)", "positions replaced (own)",
                                           "lengths set", "corrected begun", "corrected made (drops and trims only)",
                                           "corrected made (other)", "adopted", "adopted (compacted)", "offer taken",
                                           "build begins", "build from reads (single)", "build from reads (merged)",
                                           "graph in place", "graph in place (derived)", "removal begins", "nodes died",
                                           "edge died", "lists made", "match begun"};
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
  }
}

// The table, a row per event in the order of Event, a letter per flag in the order of Flag:
//   . kept   1 set   0 cleared   and the "from" cells:   d c_derivable   m dist_mode   p have_pos ? 0 : kept
//   P have_pos ? 1 : kept   e !edge_own_deaths   q !comp_from_claims
//                                         b h h p p h c d d d e p c a m c
//                                         u p r i 0 c d r c e o r v v v h
static const char* kTable[N_EVENTS] = {"0 0 0 . . 0 . 0 0 . . . . . 0 1",   // reads replaced
                                       ". 1 0 1 0 0 . . . . . . . . . .",   // positions replaced, the caller's arrays
                                       ". 1 0 1 1 0 . . . . . . . . . .",   // positions replaced, the engine's own
                                       ". . 1 . . . . . . . . . . . . .",   // lengths set
                                       ". . . . . 0 0 . . . . . . . . .",   // corrected begun
                                       ". . . . . 1 e . . . . . . . . .",   // corrected made: only drops and trims
                                       ". . . . . 1 0 . . . . . . . . .",   // corrected made: something else
                                       "0 . . p . 0 0 d m . . . . . 0 .",   // adopted
                                       "0 . . P P 0 0 d m . . . . . 0 .",   // adopted, positions compacted
                                       ". . . . . . . 0 0 . . . . . . .",   // offer taken
                                       "0 . . . . 0 . 0 0 0 . . . . 0 .",   // build begins
                                       ". . . . . . . . . . . . . . . .",   // build from reads, single
                                       ". . . . . . . . . . . . . . . .",   // build from reads, merged
                                       "1 . . . . . . . . 0 0 q 0 0 . .",   // graph in place
                                       "1 . . . . . . . . 1 0 q 0 0 . .",   // graph in place, derived
                                       ". . . . . 0 . . . . . . . . . .",   // removal begins
                                       ". . . . . . . . . . . 0 . . 0 .",   // nodes died
                                       ". . . . . . . . . . 1 0 . . 0 .",   // edge died
                                       ". . . . . . . . . . . . . . . .",   // lists made
                                       ". . . . . . . . . . . . . . 0 ."};  // match begun
static bool bit(unsigned bits, int f) { return (bits >> f) & 1u; }
static bool expected(int e, int f, unsigned before) {
  const bool was = bit(before, f);
  switch (kTable[e][2 * f]) {
    case '.': return was;
    case '1': return true;
    case '0': return false;
    case 'd': return bit(before, C_DERIVABLE);
    case 'm': return bit(before, DIST_MODE);
    case 'p': return bit(before, HAVE_POS) ? false : was;
    case 'P': return bit(before, HAVE_POS) ? true : was;
    case 'e': return !bit(before, EDGE_OWN_DEATHS);
    case 'q': return !bit(before, COMP_FROM_CLAIMS);
  }
  CHECK(!"a letter of the table");
  return false;
}
static LiveLists expected_lists(int e, LiveLists was) {
  switch (e) {
    case GRAPH_IN_PLACE: case GRAPH_DERIVED: case EDGE_DIED: return LiveLists::Absent;
    case NODES_DIED: return was == LiveLists::Current ? LiveLists::BehindNodes : was;
    case LISTS_MADE: return LiveLists::Current;
    default: return was;
  }
}

static long long every_event_from_every_state(amg_ctx* c) {
  const LiveLists lists[3] = {LiveLists::Absent, LiveLists::Current, LiveLists::BehindNodes};
  long long n = 0;
  for (int e = 0; e < N_EVENTS; ++e)
    for (unsigned before = 0; before < (1u << N_BITS); ++before)
      for (LiveLists l : lists) {
        put(c, before, l);
        apply(c, e);
        const unsigned after = get(c);
        for (int f = 0; f < N_FLAGS; ++f)
          if (bit(after, f) != expected(e, f, before)) {
            fprintf(stderr, "state_check: %s from state %#x: %s is %d\n", kEventName[e], before, kFlagName[f], (int)bit(after, f));
            exit(1);
          }
        // dist_mode and comp_from_claims: "build from reads" alone
        const bool merged = e == FROM_READS_MERGED, from_reads = merged || e == FROM_READS_SINGLE;
        CHECK(bit(after, DIST_MODE) == (from_reads ? merged : bit(before, DIST_MODE)));
        CHECK(bit(after, COMP_FROM_CLAIMS) == (from_reads ? false : bit(before, COMP_FROM_CLAIMS)));
        CHECK(c->live_lists == expected_lists(e, l));
        ++n;
      }
  return n;
}

// ------------------------------------------------------------------ hints, counters, sequences
static void hints_and_counters() {
  amg_ctx c;
  // reads replaced: sizes in, every hint gone
  c.node_hint = 900, c.hint_bound = 40, c.hint_bound_k = 3;
  ctx_reads_replaced(&c, 7, 70, 20);
  CHECK(c.n_reads == 7 && c.n_tokens == 70 && c.two_v == 20 && c.node_hint == 0 && c.hint_bound == 0);
  ctx_positions_replaced(&c, 70, false);
  CHECK(c.pos_n0 == 70 && c.pos1_used == 0 && c.c_pos1_used == 0);
  // a build from reads: no hint; the graph leaves one, never below 256
  c.retries = 3, c.tok_base = 11, c.tok_total = 0;
  CHECK(!ctx_build_begins(&c));
  CHECK(c.retries == 0 && c.tok_base == 0 && c.tok_total == 70);
  ctx_build_from_reads(&c, 3, false);
  CHECK(c.k == 3 && c.node_hint == 0);
  c.n_components = 9;
  ctx_graph_in_place(&c, 100, false);
  CHECK(c.node_hint == 256 && c.n_components == 0);
  ctx_graph_in_place(&c, 5000, false);
  CHECK(c.node_hint == 5000);
  // a corrected set: its sizes and bound wait for the adoption; the test hook overrides the bound
  ctx_corrected_begun(&c);
  ctx_corrected_made(&c, 5, 50, 12, true, 700, nullptr);
  CHECK(c.c_reads == 5 && c.c_tokens == 50 && c.c_pos1_used == 12 && c.c_node_bound == 700 && c.c_node_bound_k == 3);
  CHECK(c.n_reads == 7 && c.node_hint == 5000);
  ctx_corrected_made(&c, 5, 50, 12, true, 700, "33");
  CHECK(c.c_node_bound == 33);
  ctx_corrected_made(&c, 5, 50, 12, true, 700, nullptr);
  ctx_corrected_adopted(&c, false);
  CHECK(c.n_reads == 5 && c.n_tokens == 50 && c.pos1_used == 12 && c.pos_n0 == 70 && c.node_hint == 700 && c.c_node_bound == 0);
  // ... compacted: the pools start again; a bound above the hint, or made for another k, changes nothing
  c.node_hint = 400;
  ctx_corrected_made(&c, 4, 40, 30, false, 600, nullptr);
  ctx_corrected_adopted(&c, true);
  CHECK(c.pos_n0 == 40 && c.pos1_used == 0 && c.c_pos1_used == 0 && c.node_hint == 400 && c.c_node_bound == 0);
  ctx_corrected_made(&c, 4, 40, 0, false, 100, nullptr);
  c.c_node_bound_k = 5;
  ctx_corrected_adopted(&c, false);
  CHECK(c.node_hint == 400);
  ctx_corrected_made(&c, 4, 40, 0, false, 100, nullptr);
  ctx_corrected_adopted(&c, false);
  CHECK(c.node_hint == 256);
  // a bound handed over from another ctx: used by a single build at its k, used up by any single build, kept by a
  // merged one
  for (int k = 3; k <= 5; k += 2)
    for (int merged = 0; merged < 2; ++merged) {
      ctx_reads_replaced(&c, 4, 40, 20);
      c.hint_bound = 2000, c.hint_bound_k = 3;
      (void)ctx_build_begins(&c);
      ctx_build_from_reads(&c, k, merged != 0);
      CHECK(c.node_hint == (k == 3 && !merged ? 2000 : 0));
      CHECK(c.hint_bound == (merged ? 2000 : 0));
    }
}

// the flag half of the three callers of "reads replaced" (amg_set_reads, a borrower of amg_build_multi, the destination
// of amg_set_reads_from_corrected) and of the two position entry points, from every state
static void callers_agree() {
  amg_ctx a, b, d, src;
  src.c_node_bound = 123, src.c_node_bound_k = 3;
  for (unsigned before = 0; before < (1u << N_BITS); ++before) {
    for (amg_ctx* c : {&a, &b, &d}) {
      put(c, before, LiveLists::Current);
      c->node_hint = 77, c->hint_bound = 55, c->hint_bound_k = 5;
    }
    ctx_reads_replaced(&a, 7, 70, 20);  // amg_set_reads
    ctx_reads_replaced(&b, 7, 70, 20);  // amg_build_multi
    ctx_reads_replaced(&d, 7, 70, 20);  // amg_set_reads_from_corrected of a source without positions ...
    d.hint_bound = src.c_node_bound, d.hint_bound_k = src.c_node_bound_k;
    CHECK(get(&a) == get(&b) && get(&a) == get(&d));
    CHECK(a.node_hint == 0 && b.node_hint == 0 && d.node_hint == 0 && a.hint_bound == 0 && b.hint_bound == 0);
    CHECK(d.hint_bound == 123 && d.hint_bound_k == 3);
    CHECK(!bit(get(&a), BUILT) && !bit(get(&a), HAVE_CORRECTED) && !bit(get(&a), MATCH_VALID) && !bit(get(&a), DIST_CANDIDATE));
    // ... and of one with positions and lengths: what amg_set_reads + amg_set_positions leave, but for pos0_own
    ctx_positions_replaced(&d, 70, true);
    ctx_read_lengths_set(&d);
    ctx_positions_replaced(&a, 70, false);  // amg_set_positions with read lengths
    ctx_read_lengths_set(&a);
    ctx_positions_replaced(&b, 70, false);  // amg_set_positions32 with read lengths
    ctx_read_lengths_set(&b);
    CHECK(get(&a) == get(&b) && a.pos_n0 == b.pos_n0 && a.pos1_used == b.pos1_used);
    CHECK((get(&a) | 1u << POS0_OWN) == get(&d) && !bit(get(&a), POS0_OWN));
  }
}

static void sequences() {
  amg_ctx c;
  ctx_reads_replaced(&c, 7, 70, 20);
  (void)ctx_build_begins(&c);
  ctx_build_from_reads(&c, 3, false);
  ctx_graph_in_place(&c, 100, false);
  CHECK(c.built && c.pristine && !c.derived);
  // adopt turns c_derivable into derive_ready exactly once
  ctx_corrected_begun(&c);
  ctx_corrected_made(&c, 5, 50, 0, true, 90, nullptr);
  CHECK(c.c_derivable && !c.derive_ready);
  ctx_corrected_adopted(&c, false);
  CHECK(c.derive_ready && !c.c_derivable && !c.dist_candidate && !c.built);
  CHECK(ctx_build_begins(&c));   // the offer, taken
  CHECK(!ctx_build_begins(&c));  // and used up
  ctx_graph_in_place(&c, 90, true);
  CHECK(c.derived && c.built);
  ctx_corrected_begun(&c);
  ctx_corrected_made(&c, 5, 50, 0, false, 90, nullptr);
  ctx_corrected_adopted(&c, false);
  CHECK(!c.derive_ready);
  // a correction after an edge died on its own is never derivable; the next graph forgets the edge
  ctx_graph_in_place(&c, 90, false);
  ctx_removal_begins(&c);
  live_lists_after_edge_deaths(&c);
  ctx_corrected_begun(&c);
  ctx_corrected_made(&c, 5, 50, 0, true, 90, nullptr);
  CHECK(!c.c_derivable);
  ctx_graph_in_place(&c, 90, false);
  ctx_corrected_made(&c, 5, 50, 0, true, 90, nullptr);
  CHECK(c.c_derivable);
  // "build begins" clears derive_ready and dist_candidate in both variants: the single build; the merged build, which
  // declines in amg_dist_merge_begin or takes in st_dv_local, and begins in nodes_local
  for (int variant = 0; variant < 3; ++variant) {
    c.dist_mode = variant != 0;
    ctx_corrected_made(&c, 5, 50, 0, true, 90, nullptr);
    ctx_corrected_adopted(&c, false);
    CHECK(c.derive_ready && c.dist_candidate == (variant != 0));
    if (variant == 0) CHECK(ctx_build_begins(&c));
    if (variant == 1) CHECK(ctx_take_derive_offer(&c));  // (not a candidate: declined)
    if (variant == 2) CHECK(ctx_take_derive_offer(&c) && !ctx_build_begins(&c));
    CHECK(!c.derive_ready && !c.dist_candidate);
    ctx_build_from_reads(&c, 3, variant != 0);
    ctx_graph_in_place(&c, 90, false);
  }
  // "graph in place" after a filtered build leaves pristine false
  c.comp_from_claims = true;
  ctx_graph_in_place(&c, 90, false);
  CHECK(c.built && !c.pristine && !c.comp_valid);
  (void)ctx_build_begins(&c);
  ctx_build_from_reads(&c, 3, false);
  ctx_graph_in_place(&c, 90, false);
  CHECK(c.pristine);
  // a removal that begins drops the corrected set even if no live_lists_after_* follows (a clip that finds nothing)
  ctx_corrected_made(&c, 5, 50, 0, true, 90, nullptr);
  live_lists_made(&c);
  ctx_removal_begins(&c);
  CHECK(!c.have_corrected && c.pristine && c.live_lists == LiveLists::Current && c.built);
  // nodes die: lists that exist fall behind (or are dropped with AMG_NO_LADJ_PATCH=1), are made current again
  live_lists_after_node_deaths(&c);
  CHECK(c.live_lists == LiveLists::BehindNodes && !c.pristine);
  live_lists_made(&c);
  setenv("AMG_NO_LADJ_PATCH", "1", 1);
  live_lists_after_node_deaths(&c);
  CHECK(c.live_lists == LiveLists::Absent);
  unsetenv("AMG_NO_LADJ_PATCH");
}

int main() {
  unsetenv("AMG_NO_LADJ_PATCH");
  amg_ctx c;
  const long long n = every_event_from_every_state(&c);
  hints_and_counters();
  callers_agree();
  sequences();
  printf("state_check: %d events x %u states x 3 list states = %lld transitions match the table; hints, callers and sequences passed\n",
         (int)N_EVENTS, 1u << N_BITS, n);
  return 0;
}
