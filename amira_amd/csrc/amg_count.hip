// amg_count.hip — deferred counting: how often every node / edge-class id occurs among the per-window ids a table pass
// left behind (node coverage, construct_node.py:33-36; edge coverage), for all three key schemes.  Here: the sweep
// kernel, count_ids that launches it, and what a build learns from one count for the next one of its kind
// (count_learn_*).  Nothing else belongs here; the switches a count obeys are read with the build's (c->sw).
#include "amg_device.h"

// Occurrence counts without one global atomic per window.  Persistent 1024-thread blocks keep
// HOT_IDS counters in LDS for the id range [lo, lo + HOT_IDS) and sweep the whole id array;
// ids are first-seen ranks (or claim order), so the frequently hit (genome) nodes / edges are
// the LOW ids and a few ranges absorb almost every increment.  Every sweep also counts the
// ids that lie beyond its range (beyond[r]); the next sweep reads that number and, when at
// most 1/8 of the array is left, finishes the job with global atomics (27 G/s, cheaper than
// further 4-byte-per-id sweeps at that point); sweeps after that see its done flag and exit.
// The first sweep takes the same decision from what the first sweep of the PREVIOUS count of
// this kind left behind (hint = {beyond, n}; rebuilds of a cleaning sweep look alike).
// With GATHER the array holds table slots on entry and is rewritten to dense ids
// (tab[slot].id) during the first sweep.
// (HOT_IDS: 156 of the CU's 160 KB of LDS — the head launch of cfg 3's first build hands out 36 k claims, four
// thousand more than the 32 k counters of rounds 1-3 held, and their windows were what a second sweep was for)
#define HOT_IDS 39936
#define COUNT_MAX_SWEEPS 4
// The first sweep also LISTS the ids it finds beyond its range while they are few — every workgroup in a segment of
// its own (COUNT_LIST_SEG ids, filled through a counter in LDS: one shared list cost 20 k returning atomics on one word,
// 0.5 ms) — so that a count whose first sweep had no hint to finish the job itself (the first count of a read set) ends
// with a second launch that walks the segments, microseconds, instead of a second sweep over the whole array for a few
// thousand increments.  list: [0] a segment ran over (the list is then not used), [2 + b] ids in workgroup b's segment,
// segments from COUNT_LIST_HEAD on.
#define COUNT_LIST_SEG 256
#define COUNT_MAX_BLOCKS 256
#define COUNT_LIST_HEAD (2 + COUNT_MAX_BLOCKS)
// The state words of the counting sweeps in device memory (ctx->cnt_state), host and kernel alike: the sweeps of the last
// count of either kind, then what the first sweep of that count left for the next count of its kind to start from.
struct CountSweeps {
  unsigned long long beyond[COUNT_MAX_SWEEPS];  // ids beyond the range of sweep r
  unsigned long long done[COUNT_MAX_SWEEPS];    // sweep r finished the job
};
struct CountHint { unsigned long long beyond, n; };
struct CountState {
  CountSweeps sweeps[2];  // [CountKind]
  CountHint hint[2];
};

template <bool GATHER>
__global__ __launch_bounds__(1024) void k_count_ids(int* __restrict__ ids, long long n,
                                                    const Slot* __restrict__ tab, long long lo,
                                                    int sweep, int last, CountSweeps* state,
                                                    CountHint* hint, unsigned int* __restrict__ out,
                                                    bool marked, unsigned int* list, unsigned int seg_cap) {
  __shared__ unsigned int s_cnt[HOT_IDS];
  __shared__ unsigned int s_listed;
  bool tail_all = last != 0;
  if (sweep > 0) {
    for (int q = 0; q < sweep; ++q)
      if (state->done[q]) return;  // an earlier sweep already finished
    const unsigned long long left = state->beyond[sweep - 1];
    if (sweep == 1 && blockIdx.x == 0 && threadIdx.x == 0) {  // what the next count of this kind starts from
      hint->beyond = left;
      hint->n = (unsigned long long)n;
    }
    if (left == 0ull) return;
    if (sweep == 1 && list && list[1] == 1u && list[0] == 0u) {  // everything left is in the first sweep's segments
      const unsigned int mine = list[2 + blockIdx.x];
      for (unsigned int i = threadIdx.x; i < mine; i += 1024u)
        atomicAdd(&out[list[COUNT_LIST_HEAD + blockIdx.x * COUNT_LIST_SEG + i]], 1u);
      if (blockIdx.x == 0 && threadIdx.x == 0) state->done[sweep] = 1ull;
      return;
    }
    if (left * 8ull <= (unsigned long long)n) tail_all = true;
  } else if (hint->n != 0ull && hint->beyond * 8ull <= hint->n) {
    tail_all = true;
  }
  const bool listing = sweep == 0 && !tail_all && list != nullptr && gridDim.x <= COUNT_MAX_BLOCKS;
  if (threadIdx.x == 0) s_listed = 0u;  // (ordered before its first use by the barrier below)
  auto list_id = [&](int id) {
    const unsigned int at = atomicAdd(&s_listed, 1u);
    if (at < seg_cap) list[COUNT_LIST_HEAD + blockIdx.x * COUNT_LIST_SEG + at] = (unsigned int)id;
  };
  for (int i = threadIdx.x; i < HOT_IDS; i += 1024) s_cnt[i] = 0;
  __syncthreads();
  const long long stride = (long long)gridDim.x * 1024;
  unsigned int beyond = 0;
  // marked: claims as the table pass wrote them (flags in the top bits), and the occurrence that created a key is not
  // counted (every counter started at 1: count_ids)
  auto tally = [&](int id, long long t) {
    bool made = false;
    if (marked && id != -1) {
      made = ((unsigned int)id & AMG_MADE_FLAG) != 0u;
      id = (int)((unsigned int)id & ~AMG_FLAG_MASK);
    }
    if (GATHER) {
      id = id < 0 ? -1 : tab[id].id;
      ids[t] = id;
    }
    if (id < 0 || made) return;
    const long long rel = (long long)id - lo;
    if (rel < 0) return;
    if (rel < HOT_IDS) {
      atomicAdd(&s_cnt[rel], 1u);
    } else {
      ++beyond;
      if (tail_all) atomicAdd(&out[id], 1u);
      else if (listing) list_id(id);
    }
  };
  // one block per CU (the counters fill the LDS), so the bytes in flight have to come from the threads themselves:
  // 16-byte loads, four of them in flight per thread (64 MB chip-wide; with 4-byte loads the sweep ran at 2.2 TB/s)
  typedef int i4 __attribute__((ext_vector_type(4)));
  const long long n4 = ((reinterpret_cast<uintptr_t>(ids) & 15) == 0) ? (n >> 2) : 0;
  i4* ids4 = reinterpret_cast<i4*>(ids);
  long long q = (long long)blockIdx.x * 1024 + threadIdx.x;
  auto tally4 = [&](i4 x, long long qi) {
    unsigned int mades = 0;
    if (marked) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (x[j] != -1 && ((unsigned int)x[j] & AMG_MADE_FLAG)) mades |= 1u << j;
    }
    if (GATHER) {
      i4 y;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        int id = x[j];
        if (marked && id != -1) id = (int)((unsigned int)id & ~AMG_FLAG_MASK);
        y[j] = id < 0 ? -1 : tab[id].id;
      }
      ids4[qi] = y;
      x = y;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int id = x[j];
      if (!GATHER && marked && id != -1) id = (int)((unsigned int)id & ~AMG_FLAG_MASK);
      if (id < 0 || (mades & (1u << j))) continue;
      const long long rel = (long long)id - lo;
      if (rel < 0) continue;
      if (rel < HOT_IDS) {
        atomicAdd(&s_cnt[rel], 1u);
      } else {
        ++beyond;
        if (tail_all) atomicAdd(&out[id], 1u);
        else if (listing) list_id(id);
      }
    }
  };
  for (; q + 3 * stride < n4; q += 4 * stride) {
    i4 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = GATHER ? ids4[q + j * stride] : __builtin_nontemporal_load(ids4 + q + j * stride);
#pragma unroll
    for (int j = 0; j < 4; ++j) tally4(v[j], q + j * stride);
  }
  for (; q < n4; q += stride) tally4(GATHER ? ids4[q] : __builtin_nontemporal_load(ids4 + q), q);
  // what the 16-byte chunks leave (at most three ids; everything when the array is not 16-byte aligned)
  for (long long t = 4 * n4 + (long long)blockIdx.x * 1024 + threadIdx.x; t < n; t += stride) tally(ids[t], t);
  for (int d = 32; d > 0; d >>= 1) beyond += __shfl_down(beyond, d, 64);
  if ((threadIdx.x & 63) == 0 && beyond) atomicAdd(&state->beyond[sweep], (unsigned long long)beyond);
  if (tail_all && blockIdx.x == 0 && threadIdx.x == 0) state->done[sweep] = 1ull;
  __syncthreads();
  if (listing && threadIdx.x == 0) {
    const unsigned int got = s_listed;
    list[2 + blockIdx.x] = got < seg_cap ? got : seg_cap;
    if (got > seg_cap) list[0] = 1u;
    if (blockIdx.x == 0) list[1] = 1u;  // "the first sweep listed"
  }
  for (int i = threadIdx.x; i < HOT_IDS; i += 1024) {
    const unsigned int cnt = s_cnt[i];
    if (cnt) atomicAdd(&out[lo + i], cnt);
  }
}

static_assert(sizeof(CountState) == (4 * COUNT_MAX_SWEEPS + 4) * sizeof(unsigned long long), "cnt_state: two blocks, two hints");

// counts[id] = occurrences of id in ids[0..n); n_ids distinct ids.  `what` selects the state block, the hint and the
// learnt number of sweeps (counts of one kind look alike from build to build); `form` says what the array holds
// (CountIds, amg_internal.h).  With gather_tab the array holds table slots on entry: it is rewritten to tab[slot].id.
int count_ids(amg_ctx* c, CountKind what, CountIds form, int* ids, long long n, long long n_ids, unsigned int* out,
              const Slot* gather_tab) {
  hipStream_t st = c->stream;
  // IdsClaimsMarked: the ids carry AMG_MADE_FLAG on the occurrence that created their key — exactly one per id — so every
  // counter starts at 1 and the sweeps leave those occurrences out: an id seen once costs nothing
  const bool marked = form == IdsClaimsMarked;
  ClearList cl;
  cl.add(out, (size_t)(n_ids + 1) * sizeof(unsigned int), marked ? 1u : 0u);
  const bool fresh = !c->cnt_state.p || c->cnt_hint_reset;
  AMGCHK(c->cnt_state.ensure(sizeof(CountState)));
  if (fresh) c->cnt_sweeps[CountNodes] = c->cnt_sweeps[CountEdgeClasses] = COUNT_MAX_SWEEPS;
  c->cnt_hint_reset = false;
  CountState* cs = c->cnt_state.as<CountState>();
  CountSweeps* state = &cs->sweeps[what];
  CountHint* hint = &cs->hint[what];
  // (fresh: both kinds' sweeps and both hints — the done flags of the kind that is not counted now are read when a
  // build learns, and nothing has written them yet on a new context)
  if (fresh) cl.add(cs, sizeof(CountState));
  else cl.add(state, sizeof(CountSweeps));
  AMGCHK(c->cnt_list.ensure((size_t)(COUNT_LIST_HEAD + COUNT_MAX_BLOCKS * COUNT_LIST_SEG) * sizeof(unsigned int)));
  unsigned int* list = c->cnt_list.as<unsigned int>();
  cl.add(list, COUNT_LIST_HEAD * sizeof(unsigned int));
  // AMG_COUNT_LIST_SEG: test switch (a small segment runs over: the second launch sweeps)
  const unsigned int seg_cap = (unsigned int)std::min(std::max(c->sw.count_list_seg, 0), COUNT_LIST_SEG);
  AMGCHK(clear_many(c, cl));
  c->cnt_launched[0] = c->cnt_launched[1] = 0;
  if (n <= 0 || n_ids <= 0) return AMG_OK;
  long long ranges = (n_ids + HOT_IDS - 1) / HOT_IDS;
  if (ranges > COUNT_MAX_SWEEPS) ranges = COUNT_MAX_SWEEPS;
  // no more sweeps than the previous count of this kind made use of (count_learn_take): the last one launched finishes
  // with global atomics whatever is left, so too few sweeps cost time, never counts
  if (ranges > c->cnt_sweeps[what]) ranges = c->cnt_sweeps[what];
  // every block flushes up to HOT_IDS counters with global atomics at the end of a sweep: give a
  // block at least twice that many ids to count (small inputs: fewer blocks, not a shorter sweep)
  long long want_blocks = (n + 2 * HOT_IDS - 1) / (2 * HOT_IDS);
  unsigned int blocks = (unsigned int)(want_blocks < 1 ? 1 : (want_blocks < COUNT_MAX_BLOCKS ? want_blocks : COUNT_MAX_BLOCKS));
  c->cnt_launched[0] = (int)ranges;
  c->cnt_launched[1] = (int)blocks;
  for (long long r = 0; r < ranges; ++r) {
    const long long lo = r * HOT_IDS;
    const int last = (r == ranges - 1) ? 1 : 0;
    if (gather_tab && r == 0)
      hipLaunchKernelGGL(k_count_ids<true>, dim3(blocks), dim3(1024), 0, st, ids, n, gather_tab, lo,
                         (int)r, last, state, hint, out, marked, list, seg_cap);
    else
      hipLaunchKernelGGL(k_count_ids<false>, dim3(blocks), dim3(1024), 0, st, ids, n, gather_tab, lo,
                         (int)r, last, state, hint, out, marked, list, seg_cap);
  }
  if (c->sw.count_debug) {  // what every sweep left beyond its range, which one finished (synchronises: debugging only)
    CountSweeps h;
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipMemcpy(&h, state, sizeof(h), hipMemcpyDeviceToHost));
    fprintf(stderr, "[amg] count %s%s: n %lld ids %lld sweeps %lld beyond %llu %llu %llu %llu done %llu %llu %llu %llu\n",
            what == CountNodes ? "nodes" : "edge classes", marked ? " (marked claims)" : "", n, n_ids, ranges, h.beyond[0],
            h.beyond[1], h.beyond[2], h.beyond[3], h.done[0], h.done[1], h.done[2], h.done[3]);
  }
  return AMG_OK;
}

// What a build learns from its counts for the next build: how many sweeps each of them made use of.  The done flags of
// both kinds ride along with the build's final read-back (bs_finish_from_pairs): count_learn_add puts them on its list
// (false: there is nothing to learn, no count has run since the hints were reset), count_learn_take turns the
// COUNT_LEARN_WORDS words fetched into cnt_sweeps[].
static_assert(COUNT_LEARN_WORDS == 2 * COUNT_MAX_SWEEPS, "the done flags of both kinds");
bool count_learn_add(amg_ctx* c, FetchList* l) {
  if (!c->cnt_state.p || c->cnt_hint_reset) return false;
  CountState* cs = c->cnt_state.as<CountState>();
  for (int s = 0; s < 2; ++s) l->add_words(cs->sweeps[s].done, COUNT_MAX_SWEEPS);
  return true;
}

void count_learn_take(amg_ctx* c, const unsigned long long* done) {
  for (int s = 0; s < 2; ++s) {
    int used = COUNT_MAX_SWEEPS;
    for (int q = COUNT_MAX_SWEEPS - 1; q >= 0; --q)
      if (done[s * COUNT_MAX_SWEEPS + q]) used = q + 1;
    c->cnt_sweeps[s] = used;
  }
}

// ------------------------------------------------------------------ amg_count_probe (tests: one count on host arrays)
extern "C" int amg_count_probe(amg_ctx* c, int kind, int form, int32_t* ids, int64_t n, int64_t n_ids, const int32_t* tab_ids,
                               int64_t n_slots, int misalign, int flags, uint32_t* counts, int64_t* state) {
  if (!c || (kind != CountNodes && kind != CountEdgeClasses) || form < 0 || form > 2 || n < 0 || n_ids < 0 ||
      n_ids >= (1ll << 29) || (n > 0 && !ids) || misalign < 0 || misalign > 3 || !counts || !state ||
      (form == 2 && (n_slots < 0 || (n_slots > 0 && !tab_ids))))
    return amg_fail(AMG_E_ARG, "count_probe: bad arguments");
  // the sweeps index their counters by what the array holds: nothing out of range goes to the device
  for (int64_t i = 0; i < n; ++i) {
    long long id = ids[i];
    if (form == 1 && id != -1) id = (long long)((unsigned int)ids[i] & ~AMG_FLAG_MASK);
    if (form == 2 && id >= 0) {
      if (id >= n_slots) return amg_fail(AMG_E_ARG, "count_probe: slot %lld at %lld beyond the table", id, (long long)i);
      id = tab_ids[id];
    }
    if (id >= n_ids) return amg_fail(AMG_E_ARG, "count_probe: id %lld at %lld, n_ids %lld", id, (long long)i, (long long)n_ids);
  }
  HIPCHK(hipSetDevice(c->device));
  const size_t guard = 64;  // words in front of and behind the id array, and behind the counts: 0xff before the call
  const size_t ids_words = guard + (size_t)n + 4 + guard, cnt_words = (size_t)n_ids + 1 + guard;
  const size_t tab_bytes = form == 2 ? ((size_t)n_slots + 1) * sizeof(Slot) : 0;
  const size_t ids_cap = (ids_words * 4 + 255) & ~(size_t)255, cnt_cap = (cnt_words * 4 + 255) & ~(size_t)255;
  char* d = nullptr;
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&d), ids_cap + cnt_cap + tab_bytes));
  int* dbuf = reinterpret_cast<int*>(d);
  int* dids = dbuf + guard + misalign;  // (hipMalloc aligns to 256 bytes, the guard is 256 bytes)
  unsigned int* dcnt = reinterpret_cast<unsigned int*>(d + ids_cap);
  Slot* dtab = form == 2 ? reinterpret_cast<Slot*>(d + ids_cap + cnt_cap) : nullptr;
  std::vector<unsigned int> back;
  int rc = AMG_OK;
  do {
    if (hipMemset(d, 0xff, ids_cap + cnt_cap) != hipSuccess) { rc = amg_fail(AMG_E_HIP, "count_probe: memset"); break; }
    if (n && hipMemcpy(dids, ids, (size_t)n * 4, hipMemcpyHostToDevice) != hipSuccess) { rc = amg_fail(AMG_E_HIP, "h2d"); break; }
    if (form == 2) {
      std::vector<Slot> tab((size_t)n_slots + 1);
      memset(tab.data(), 0xff, tab.size() * sizeof(Slot));
      for (int64_t i = 0; i < n_slots; ++i) tab[i].id = tab_ids[i];
      if (hipMemcpy(dtab, tab.data(), tab_bytes, hipMemcpyHostToDevice) != hipSuccess) { rc = amg_fail(AMG_E_HIP, "h2d"); break; }
    }
    if (hipDeviceSynchronize() != hipSuccess) { rc = amg_fail(AMG_E_HIP, "count_probe: sync"); break; }
    c->sw = read_build_switches();
    if (flags & 1) c->cnt_hint_reset = true;  // what amg_set_reads does: the next count starts without hints
    rc = count_ids(c, (CountKind)kind, form == 1 ? IdsClaimsMarked : IdsPlain, dids, n, n_ids, dcnt, dtab);
    if (rc != AMG_OK) break;
    if (flags & 2) {  // what a build's final read-back does
      FetchList l;
      unsigned long long v[COUNT_LEARN_WORDS] = {0};
      if (count_learn_add(c, &l)) {
        if ((rc = fetch(c, l, v)) != AMG_OK) break;
        count_learn_take(c, v);
      }
    }
    if (hipStreamSynchronize(c->stream) != hipSuccess) { rc = amg_fail(AMG_E_HIP, "count_probe: stream"); break; }
    CountSweeps h;
    unsigned int lst[2];
    if (hipMemcpy(&h, &c->cnt_state.as<CountState>()->sweeps[kind], sizeof(h), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(lst, c->cnt_list.p, sizeof(lst), hipMemcpyDeviceToHost) != hipSuccess) {
      rc = amg_fail(AMG_E_HIP, "d2h");
      break;
    }
    back.resize(ids_words > cnt_words ? ids_words : cnt_words);
    bool intact = true;
    if (hipMemcpy(back.data(), dbuf, ids_words * 4, hipMemcpyDeviceToHost) != hipSuccess) { rc = amg_fail(AMG_E_HIP, "d2h"); break; }
    const size_t first = guard + (size_t)misalign;
    for (size_t i = 0; i < ids_words; ++i)
      if ((i < first || i >= first + (size_t)n) && back[i] != 0xffffffffu) intact = false;
    if (n) memcpy(ids, back.data() + first, (size_t)n * 4);
    if (hipMemcpy(back.data(), dcnt, cnt_words * 4, hipMemcpyDeviceToHost) != hipSuccess) { rc = amg_fail(AMG_E_HIP, "d2h"); break; }
    for (size_t i = (size_t)n_ids + 1; i < cnt_words; ++i)
      if (back[i] != 0xffffffffu) intact = false;
    memcpy(counts, back.data(), ((size_t)n_ids + 1) * 4);
    for (int q = 0; q < COUNT_MAX_SWEEPS; ++q) state[q] = (int64_t)h.beyond[q], state[4 + q] = (int64_t)h.done[q];
    state[8] = lst[0];
    state[9] = lst[1];
    state[10] = c->cnt_launched[0];
    state[11] = c->cnt_launched[1];
    state[12] = c->cnt_sweeps[kind];
    state[13] = intact ? 1 : 0;
  } while (false);
  (void)hipFree(d);
  return rc;
}
