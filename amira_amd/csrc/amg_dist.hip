// amg_dist.hip — read-sharded build with a key-owner table merge, driven from HERE.
//
// Every rank holds a contiguous shard of the reads.  The single-graph result (graph_utils.py:105-124 at cores = 1,
// i.e. GeneMerGraph over all reads) is obtained, for the nodes and then for the edge classes, in six steps:
//
//   local    the ordinary table pass on the shard (exact keys + claim ids when the tuple fits, else 32-byte fingerprint
//            slots), occurrence counts per local key, one 24-byte record {merge key, local first-seen, count} per
//            local key, bucketed by owner = hash(key) mod world; the per-peer record counts are written into a COUNT
//            MESSAGE on the device (with the shard's token count, the retry counter and — in place of the count — a
//            negative code when a device phase of this rank failed)                       --> all-to-all of the messages
//   counts   ONE read-back: what I send, what I receive, every shard's token count (first-seen values become global
//            token indices from here on), everybody's verdict; records in destination order --> all-to-all of records
//   reduce   owner side: equal keys meet in an open-addressing table of 16-byte slots {key, ~min first-seen}, counts in
//            a dense array by slot; every received record is answered with {the key's global first-seen | "dropped by
//            the fused filter", its total count}                                          --> all-to-all back
//   hold     the rank whose own first-seen IS the global one HOLDS the key: holders are ranked by their local
//            first-seen (a bitmap over the LOCAL tokens) and emit {first-seen, total, tuple} in that order; the
//            number held (or a failure code) goes into a second device-built message      --> all-gather of the messages
//   hcounts  ONE read-back: held records of every rank, everybody's verdict               --> all-gather of held records
//   global   shards are contiguous read ranges, so the gathered buffer — rank 0's held records, then rank 1's, ... —
//            IS the table in global first-seen order: id = records of the ranks before + index.  No bitmap over the
//            global token space, no sort, no scatter: a coalesced unpack.  A local key finds its id by binary search
//            of its reply among the (ascending) first-seen values and checks its tuple against the holder's (two
//            gene-mers under one 64-bit merge key: every rank repeats the build with the next seed).
//
// Two host waits per kind, four per merged build.  The exchanges are `amg_xfer`s: amg_dist_merge performs them with
// RCCL (ncclSend / ncclRecv groups and ncclAllGather on the ctx's stream; librccl is opened at amg_dist_init, not
// linked), amg_dist_merge_local with device copies between the ctxs of one process (emulated ranks: tests, the scaling
// model), and amg_dist_merge_begin / _next hand them to the caller (tests between processes over gloo).
// The read walks of a merged graph (amg_dist_walk.hip) travel over the same three transports.
#include <dlfcn.h>

#include "amg_dist.h"

static const char* const kPhaseNames[2 * S_N] = {  // [kind * S_N + state]
    "", "nodes_local", "nodes_counts_pack", "nodes_reduce", "nodes_hold", "nodes_hcounts", "nodes_global",
    "derive_local", "derive_ask", "derive_fill",
    "", "edges_local", "edges_counts_pack", "edges_reduce", "edges_hold", "edges_hcounts", "edges_global", "", "", ""};

DistState* dist_state(amg_ctx* c) {
  if (!c->dist) c->dist = new DistState();
  return c->dist;
}

// ------------------------------------------------------------------ RCCL, opened on demand
struct Rccl {
  void* h = nullptr;
#define RCCL_ENTRIES(X) \
  X(GetUniqueId) X(CommInitRank) X(CommDestroy) X(GetErrorString) X(GroupStart) X(GroupEnd) X(Send) X(Recv) X(AllGather)
#define RDECL(name) decltype(&nccl##name) name = nullptr;
  RCCL_ENTRIES(RDECL)
#undef RDECL
};
static Rccl g_rccl;

static int rccl_open() {
  if (g_rccl.h) return AMG_OK;
  // (a process that has imported torch already holds its librccl under this soname: the same library is reused)
  void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
  if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
  if (!h) return amg_fail(AMG_E_DIST, "librccl.so.1 not found: %s", dlerror());
#define RSYM(name)                                                                          \
  g_rccl.name = reinterpret_cast<decltype(g_rccl.name)>(dlsym(h, "nccl" #name));            \
  if (!g_rccl.name) return amg_fail(AMG_E_DIST, "librccl lacks nccl" #name);
  RCCL_ENTRIES(RSYM)
#undef RSYM
  g_rccl.h = h;
  return AMG_OK;
}
#define NCCLCHK(call)                                                                                        \
  do {                                                                                                       \
    ncclResult_t r_ = (call);                                                                                \
    if (r_ != ncclSuccess) return amg_fail(AMG_E_DIST, "%s:%d %s -> %s", __FILE__, __LINE__, #call, g_rccl.GetErrorString(r_)); \
  } while (0)

extern "C" int amg_dist_unique_id(void* out, int32_t bytes) {
  if (!out || bytes < (int32_t)sizeof(ncclUniqueId)) return amg_fail(AMG_E_ARG, "amg_dist_unique_id: room for %d bytes", (int)sizeof(ncclUniqueId));
  AMGCHK(rccl_open());
  ncclUniqueId id;
  NCCLCHK(g_rccl.GetUniqueId(&id));
  memcpy(out, &id, sizeof(id));
  return AMG_OK;
}

void dist_release(amg_ctx* c) {
  DistState* d = c->dist;
  if (!d) return;
  if (d->comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(d->comm);
  DevBuf* all[] = {&d->cnt_send, &d->cnt_recv, &d->hc_send,    &d->hc_recv,      &d->offs,      &d->send,
                   &d->recv,     &d->rep_out,  &d->rep_in,     &d->held,         &d->held_pad,  &d->gathered,
                   &d->own_tab,  &d->loc_cnt,  &d->loc_bucket, &d->loc_dest_cnt, &d->loc_first, &d->loc_slot,
                   &d->walk.msg, &d->walk.msg_all, &d->walk.send, &d->walk.recv};
  for (DevBuf* b : all) b->release();
  delete d;
  c->dist = nullptr;
}

static int set_world(amg_ctx* c, int rank, int world) {
  if (world < 1 || rank < 0 || rank >= world) return amg_fail(AMG_E_ARG, "bad rank %d / world %d", rank, world);
  DistState* d = dist_state(c);
  if (d->state != S_IDLE) return amg_fail(AMG_E_STATE, "a merged build is under way");
  d->walk.state = W_IDLE;  // (a walk somebody abandoned ends here)
  if (d->comm) {
    (void)g_rccl.CommDestroy(d->comm);
    d->comm = nullptr;
  }
  d->rank = rank;
  d->world = world;
  const char* e = getenv("AMG_DIST_ALWAYS_EXCHANGE");  // test hook
  d->always_exchange = e && e[0] == '1';
  return AMG_OK;
}

extern "C" int amg_dist_init(amg_ctx* c, const void* unique_id, int32_t rank, int32_t world) {
  NEED_CTX(c);
  if (!unique_id) return amg_fail(AMG_E_ARG, "null unique id");
  AMGCHK(rccl_open());
  AMGCHK(set_world(c, rank, world));
  ncclUniqueId id;
  memcpy(&id, unique_id, sizeof(id));
  NCCLCHK(g_rccl.CommInitRank(&dist_state(c)->comm, world, id, rank));
  return AMG_OK;
}

extern "C" int amg_dist_init_external(amg_ctx* c, int32_t rank, int32_t world) {
  NEED_CTX(c);
  return set_world(c, rank, world);
}

extern "C" int amg_dist_finalize(amg_ctx* c) {
  if (!c) return amg_fail(AMG_E_ARG, "null ctx");
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  dist_release(c);
  return AMG_OK;
}

static int copy_sync(amg_ctx* c, void* to, const void* from, int64_t bytes, hipMemcpyKind kind) {
  NEED_CTX(c);
  if (bytes < 0 || (bytes > 0 && (!to || !from))) return amg_fail(AMG_E_ARG, "bad copy");
  if (bytes) HIPCHK(hipMemcpyAsync(to, from, (size_t)bytes, kind, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return AMG_OK;
}
extern "C" int amg_copy_d2h(amg_ctx* c, const void* device_ptr, void* host_ptr, int64_t bytes) {
  return copy_sync(c, host_ptr, device_ptr, bytes, hipMemcpyDeviceToHost);
}
extern "C" int amg_copy_h2d(amg_ctx* c, void* device_ptr, const void* host_ptr, int64_t bytes) {
  return copy_sync(c, device_ptr, host_ptr, bytes, hipMemcpyHostToDevice);
}

// ------------------------------------------------------------------ what the states share
static long long n_local_of(const amg_ctx* c, int kind) { return kind ? c->n_local_pairs : c->n_local_nodes; }

// what every rank saw in a count exchange decides what every rank does: 0 go on, 1 repeat the build with the next
// seed (all failures were merge-key collisions), < 0 this rank's return code
static int verdict(DistState* d, const long long* codes, int stride, const long long* attempts) {
  bool any = false, all_collisions = true;
  std::string who;
  for (int r = 0; r < d->world; ++r) {
    const long long v = codes[(size_t)r * stride];
    if (attempts && v >= 0 && attempts[(size_t)r * stride] != d->attempt)
      return amg_fail(AMG_E_DIST, "rank %d is at attempt %lld of the merged build, this rank at %d", r,
                      attempts[(size_t)r * stride], d->attempt);
    if (v >= 0) continue;
    any = true;
    if (v != CODE_COLLISION) all_collisions = false;
    who += (who.empty() ? "" : ", ") + std::to_string(r);
  }
  if (!any) return 0;
  if (all_collisions) {
    if (d->attempt + 1 < MAX_ATTEMPTS) return 1;
    return amg_fail(AMG_E_COLLISION, "merge keys still collide after %d seeds", MAX_ATTEMPTS);
  }
  if (d->fail_ret && d->fail_ret != AMG_E_COLLISION) {  // this rank's own error, as it was reported
    g_amg_err = d->fail_msg;
    return d->fail_ret;
  }
  if (codes[(size_t)d->rank * stride] < 0 && codes[(size_t)d->rank * stride] != CODE_COLLISION)
    return amg_fail(AMG_E_DIST, "merged build inconsistent on this rank (a reply without a record, or the owner table full)");
  return amg_fail(AMG_E_DIST, "merged build abandoned: device phase failed on rank(s) %s", who.c_str());
}

static void restart(DistState* d) {
  ++d->attempt;
  d->kind = 0;
  d->state = S_LOCAL;
  d->fail_ret = 0;
}

// stat: where the most bytes to one peer are booked (DS_REC_PEER_BYTES: the bytes to all peers as well), or DS_NONE
static void xfer_a2a(DistState* d, amg_xfer* x, const void* send, void* recv, int elem_bytes, const std::vector<int64_t>& sc,
                     const std::vector<int64_t>& rc, DistStat stat) {
  d->x_send = sc;
  d->x_recv = rc;
  x->kind = AMG_XFER_ALL_TO_ALL;
  x->elem_bytes = elem_bytes;
  x->send = send;
  x->recv = recv;
  x->send_counts = d->x_send.data();
  x->recv_counts = d->x_recv.data();
  x->count = 0;
  ++d->st[DS_EXCHANGES];
  if (stat != DS_NONE) {
    int64_t most = 0, sum = 0;
    for (int p = 0; p < d->world; ++p)
      if (p != d->rank) {
        most = sc[p] > most ? sc[p] : most;
        sum += sc[p];
      }
    d->st[stat] += most * elem_bytes;
    if (stat == DS_REC_PEER_BYTES) d->st[DS_REC_BYTES] += sum * elem_bytes;
  }
}

void dist_xfer_ag(DistState* d, amg_xfer* x, const void* send, void* recv, int elem_bytes, int64_t count, bool stat) {
  x->kind = AMG_XFER_ALL_GATHER;
  x->elem_bytes = elem_bytes;
  x->send = send;
  x->recv = recv;
  x->send_counts = x->recv_counts = nullptr;
  x->count = count;
  ++d->st[DS_EXCHANGES];
  if (stat) d->st[DS_HELD_BYTES] += count * elem_bytes;
}

// ONE read-back: the message words of every rank (world blocks of `stride` words at a, then — if given — at b) in
// d->words, through the pinned mailbox while they fit one list, by a copy otherwise
static int read_exchanged(amg_ctx* c, DistState* d, int stride, const void* a, const void* b = nullptr) {
  const int n = d->world * stride, parts = b ? 2 : 1;
  const void* const src[2] = {a, b};
  d->words.assign((size_t)n * parts, 0);
  long long* out = reinterpret_cast<long long*>(d->words.data());
  if (n * parts <= FETCH_MAX) {
    FetchList l;
    for (int i = 0; i < parts; ++i) l.add_words(src[i], n);
    AMGCHK(fetch(c, l, reinterpret_cast<unsigned long long*>(out)));
  } else {
    for (int i = 0; i < parts; ++i)
      HIPCHK(hipMemcpyAsync(out + (size_t)i * n, src[i], (size_t)n * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  ++d->st[DS_WAITS];
  return AMG_OK;
}
// ... and everybody's verdict on them (attempt counters at word `attempt_at` of a block): as verdict(), restart() made
static int read_and_judge(amg_ctx* c, DistState* d, int stride, int attempt_at, const void* a, const void* b = nullptr) {
  AMGCHK(read_exchanged(c, d, stride, a, b));
  const long long* got = reinterpret_cast<const long long*>(d->words.data());
  const int v = verdict(d, got, stride, got + attempt_at);
  if (v == 1) restart(d);
  return v;
}

// first-seen values are global token indices: this shard's tokens follow those of the ranks before it (d->tokens)
static void set_token_base(amg_ctx* c, const DistState* d) {
  long long base = 0, total = 0;
  for (int p = 0; p < d->world; ++p) {
    if (p < d->rank) base += d->tokens[p];
    total += d->tokens[p];
  }
  c->tok_base = base;
  c->tok_total = total;
}

// per-phase clock of the driver (amg_dist_phase_ms): the phase that ends is booked, `next` begins (-1: none)
static void phase_tick(amg_ctx* c, DistState* d, int next) {
  if (!d->time_phases) return;
  (void)hipStreamSynchronize(c->stream);
  const auto now = std::chrono::steady_clock::now();
  if (d->phase_now >= 0) d->phase_ms[d->phase_now] += std::chrono::duration<double, std::milli>(now - d->phase_t0).count();
  d->phase_now = next;
  d->phase_t0 = now;
}

// ------------------------------------------------------------------ the states
// What a state function tells the driver.  STEP_DONE and STEP_XFER are amg_dist_merge_next's own return values, and so
// is every AMG_E_* code (< 0: AMGCHK and HIPCHK return through); whoever receives one of those puts the machine to rest.
typedef int Step;
enum { STEP_DONE = 0 /* the build is complete */, STEP_XFER = 1 /* perform *x, then come back */, STEP_ON = 2 /* d->state next */ };

// one rank sends nothing (what it packs is what arrives) unless the test hook asks for it
bool dist_on_wire(const DistState* d) { return d->world > 1 || d->always_exchange; }

static Step st_local(amg_ctx* c, DistState* d, amg_xfer* x) {
  const int is_edge = d->kind, W = d->world;
  const bool wire = dist_on_wire(d);
  const int r = is_edge ? edges_local(c, d) : nodes_local(c, d);
  if (r != AMG_OK) {
    if (!wire) {
      if (r != AMG_E_COLLISION || d->attempt + 1 >= MAX_ATTEMPTS) return r;
      restart(d);
      return STEP_ON;
    }
    d->fail_ret = r;  // (the peers are told in the count exchange; verdict() reports it as it was)
    d->fail_msg = g_amg_err;
  }
  d->n_send = d->fail_ret ? 0 : n_local_of(c, is_edge);
  d->state = S_COUNTS;
  if (!wire) {
    d->send_counts.assign(1, d->n_send);
    d->recv_counts = d->send_counts;
    d->tokens.assign(1, c->n_tokens);
    return STEP_ON;
  }
  AMGCHK(d->cnt_send.ensure((size_t)W * CNT_WORDS * sizeof(long long)));
  AMGCHK(d->cnt_recv.ensure((size_t)W * CNT_WORDS * sizeof(long long)));
  count_message(c, d, is_edge);
  d->one.assign(W, 1);
  xfer_a2a(d, x, d->cnt_send.p, d->cnt_recv.p, CNT_WORDS * (int)sizeof(long long), d->one, d->one, DS_NONE);
  return STEP_XFER;
}

static Step st_counts(amg_ctx* c, DistState* d, amg_xfer* x) {
  const int is_edge = d->kind, W = d->world;
  const bool wire = dist_on_wire(d);
  if (wire) {
    const int v = read_and_judge(c, d, CNT_WORDS, 2, d->cnt_recv.p, d->cnt_send.p);
    if (v != 0) return v < 0 ? v : STEP_ON;
    const long long* got = reinterpret_cast<const long long*>(d->words.data());
    const long long* sent = got + (size_t)W * CNT_WORDS;
    d->send_counts.resize(W);
    d->recv_counts.resize(W);
    d->tokens.resize(W);
    for (int p = 0; p < W; ++p) {
      d->recv_counts[p] = got[(size_t)p * CNT_WORDS];
      d->send_counts[p] = sent[(size_t)p * CNT_WORDS];
      d->tokens[p] = got[(size_t)p * CNT_WORDS + 1];
      if (got[(size_t)p * CNT_WORDS + 3] != is_edge)
        return amg_fail(AMG_E_DIST, "rank %d is in another phase of the merged build", p);
    }
  }
  if (!is_edge) {
    set_token_base(c, d);
    if (c->tok_total >= (1ll << 60)) return amg_fail(AMG_E_ARG, "too many tokens");
  }
  d->n_recv = 0;
  d->n_sources = 0;
  long long n_send = 0;
  for (int p = 0; p < W; ++p) {
    d->n_recv += d->recv_counts[p];
    n_send += d->send_counts[p];
    if (d->recv_counts[p] > 0) ++d->n_sources;
  }
  if (n_send != d->n_send)
    return amg_fail(AMG_E_DIST, "%lld local records but %lld destinations", (long long)d->n_send, n_send);
  // every buffer up to the next count exchange is made here: nothing between two exchanges fails for want of memory
  AMGCHK(d->send.ensure((size_t)(d->n_send + 1) * REC_BYTES));
  AMGCHK(d->rep_in.ensure((size_t)(d->n_send + 1) * REPLY_WORDS * sizeof(long long)));
  AMGCHK(d->rep_out.ensure((size_t)(d->n_recv + 1) * REPLY_WORDS * sizeof(long long)));
  AMGCHK(d->held.ensure((size_t)(d->n_send + 1) * held_bytes(c, is_edge)));
  AMGCHK(d->hc_send.ensure(HC_WORDS * sizeof(long long)));
  AMGCHK(d->hc_recv.ensure((size_t)W * HC_WORDS * sizeof(long long)));
  AMGCHK(d->offs.ensure((size_t)(W + 2) * sizeof(long long)));
  if (wire) AMGCHK(d->recv.ensure((size_t)(d->n_recv + 1) * REC_BYTES));
  AMGCHK(reduce_reserve(c, d));
  stage_begin(c, is_edge ? "merge_edge_pack" : "merge_node_pack");
  pack_records(c, d, is_edge);
  stage_end(c);
  d->state = S_REDUCE;
  if (!wire) return STEP_ON;
  xfer_a2a(d, x, d->send.p, d->recv.p, REC_BYTES, d->send_counts, d->recv_counts, DS_REC_PEER_BYTES);
  return STEP_XFER;
}

static Step st_reduce(amg_ctx* c, DistState* d, amg_xfer* x) {
  const int is_edge = d->kind;
  const bool wire = dist_on_wire(d);
  // (one rank, nothing on the wire: what was packed is what arrives, and the answers are read where they are written)
  d->recv_p = wire ? d->recv.p : d->send.p;
  d->rep_out_p = wire ? d->rep_out.p : d->rep_in.p;
  d->rep_in_p = d->rep_in.p;
  stage_begin(c, is_edge ? "merge_edge_reduce" : "merge_node_reduce");
  const int r = reduce_records(c, d, is_edge);
  stage_end(c);
  if (r != AMG_OK) return r;
  d->state = S_HOLD;
  if (!wire) return STEP_ON;
  xfer_a2a(d, x, d->rep_out.p, d->rep_in.p, REPLY_WORDS * (int)sizeof(long long), d->recv_counts, d->send_counts,
           DS_REPLY_PEER_BYTES);
  return STEP_XFER;
}

static Step st_hold(amg_ctx* c, DistState* d, amg_xfer* x) {
  const int is_edge = d->kind;
  stage_begin(c, is_edge ? "merge_edge_hold" : "merge_node_hold");
  const int r = hold_records(c, d, is_edge);
  stage_end(c);
  if (r != AMG_OK) return r;
  d->state = S_HCOUNTS;
  if (!dist_on_wire(d)) return STEP_ON;
  dist_xfer_ag(d, x, d->hc_send.p, d->hc_recv.p, HC_WORDS * (int)sizeof(long long), 1, false);
  return STEP_XFER;
}

static Step st_hcounts(amg_ctx* c, DistState* d, amg_xfer* x) {
  const int is_edge = d->kind, W = d->world;
  const bool wire = dist_on_wire(d);
  const void* msg = wire ? d->hc_recv.p : d->hc_send.p;
  const int v = read_and_judge(c, d, HC_WORDS, 1, msg);
  if (v != 0) return v < 0 ? v : STEP_ON;
  const long long* got = reinterpret_cast<const long long*>(d->words.data());
  d->held_counts.resize(W);
  d->m_pad = 0;
  d->n_total = 0;
  for (int p = 0; p < W; ++p) {
    d->held_counts[p] = got[(size_t)p * HC_WORDS];
    d->n_total += d->held_counts[p];
    if (d->held_counts[p] > d->m_pad) d->m_pad = d->held_counts[p];
  }
  d->n_held = d->held_counts[d->rank];
  if (d->n_held > d->n_send)
    return amg_fail(AMG_E_DIST, "%lld records held of %lld sent", (long long)d->n_held, (long long)d->n_send);
  if (d->n_total >= (is_edge ? (1ll << 30) : (1ll << 29)))
    return amg_fail(AMG_E_OVERFLOW, "merged graph beyond 2^%d %s", is_edge ? 30 : 29, is_edge ? "edge classes" : "nodes");
  held_offsets(c, d, static_cast<const long long*>(msg));
  d->state = S_GLOBAL;
  if (!wire || d->m_pad == 0) {
    d->gathered_p = d->held.p;
    return STEP_ON;
  }
  const int hb = held_bytes(c, is_edge);
  // equal-size contributions of m record slots; what lies behind a rank's own records is never read
  const void* src = d->held.p;
  if (d->held.cap < (size_t)d->m_pad * hb) {
    AMGCHK(d->held_pad.ensure((size_t)d->m_pad * hb));
    HIPCHK(hipMemcpyAsync(d->held_pad.p, d->held.p, (size_t)d->n_held * hb, hipMemcpyDeviceToDevice, c->stream));
    src = d->held_pad.p;
  }
  AMGCHK(d->gathered.ensure((size_t)W * (size_t)d->m_pad * hb));
  d->gathered_p = d->gathered.p;
  dist_xfer_ag(d, x, src, d->gathered.p, hb, d->m_pad, true);
  return STEP_XFER;
}

static Step st_global(amg_ctx* c, DistState* d, amg_xfer*) {
  if (!d->kind) {
    AMGCHK(nodes_global(c, d));
    d->kind = 1;
    d->state = S_LOCAL;
    return STEP_ON;
  }
  AMGCHK(edges_global(c, d));
  d->st[DS_REPEATS] += d->attempt;
  return STEP_DONE;
}

// ---- the merged rebuild that reuses the previous one (amg_derive.hip: when NO rank re-threaded a read the graph every
// rank holds, restricted to its live nodes, is the graph of the corrected reads — every rank squeezes its copy; what
// only the rank that holds a first occurrence knows, its token index in the NEW reads, travels in one all-gather: two
// exchanges and one host wait instead of ten and four)
__global__ void k_dv_msg(long long ok, long long n_tokens, long long attempt, long long n_nodes, long long* __restrict__ msg) {
  msg[0] = ok;
  msg[1] = n_tokens;
  msg[2] = attempt;
  msg[3] = n_nodes;
}
// this rank's part of the all-gather: the first-seen values of the nodes, then of the classes, first seen on its shard
// (local token indices so far: the shard's new first token is added), each padded to the largest part
__global__ void k_dv_contrib(const long long* __restrict__ nfirst, long long n_n, long long add_n,
                             const unsigned long long* __restrict__ pfirst, long long n_p, unsigned long long add_p,
                             long long m_n, long long m_p, unsigned long long* __restrict__ out) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_n) out[i] = (unsigned long long)(nfirst[i] + add_n);
  else if (i >= m_n && i - m_n < n_p) out[i] = pfirst[i - m_n] + add_p;
}
__global__ void k_dv_fill(const unsigned long long* __restrict__ all, long long m_n, long long m_p, int world,
                          const long long* __restrict__ bounds, long long* __restrict__ nfirst,
                          unsigned long long* __restrict__ pfirst) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long m = m_n + m_p;
  if (i >= m * world) return;
  const int r = (int)(i / m);
  const long long j = i - (long long)r * m;
  if (j < m_n) {
    if (j < bounds[r + 1] - bounds[r]) nfirst[bounds[r] + j] = (long long)all[i];
  } else {
    const long long* pb = bounds + world + 1;
    const long long q = j - m_n;
    if (q < pb[r + 1] - pb[r]) pfirst[pb[r] + q] = all[i];
  }
}

static Step dv_done(amg_ctx* c, DistState* d) {
  AMGCHK(derive_commit(c, d->dv_D2, d->dv_P2));
  ++d->st[DS_DERIVED];
  return STEP_DONE;
}

static Step st_dv_local(amg_ctx* c, DistState* d, amg_xfer* x) {
  const int W = d->world;
  // every rank squeezes its copy of the graph (when ITS correction allows it) and says so; only if all do is the
  // squeezed graph taken — otherwise the ordinary merged build runs, nothing it reads has been touched
  d->dv_ok = false;
  const bool mine = ctx_take_derive_offer(c) && (int)d->tokens.size() == W;
  if (mine) {
    d->dv_bases.assign(W + 1, 0);
    for (int p = 0; p < W; ++p) d->dv_bases[p + 1] = d->dv_bases[p] + d->tokens[p];
    AMGCHK(d->offs.ensure((size_t)(2 * W + 4) * sizeof(long long)));
    HIPCHK(hipMemcpyAsync(d->offs.p, d->dv_bases.data(), (size_t)(W + 1) * sizeof(long long), hipMemcpyHostToDevice, c->stream));
    d->dv_bounds.assign(2 * (W + 1), 0);
    AMGCHK(derive_local(c, d->k, d->dv_bases[d->rank], d->tokens[d->rank], d->offs.as<long long>(), W,
                        d->dv_bounds.data(), &d->dv_D2, &d->dv_P2, &d->dv_ok));
  }
  if (!dist_on_wire(d)) {
    if (!d->dv_ok) {
      d->state = S_LOCAL;
      return STEP_ON;
    }
    d->tokens.assign(1, c->n_tokens);
    c->tok_base = 0;
    c->tok_total = c->n_tokens;
    return dv_done(c, d);
  }
  AMGCHK(d->cnt_send.ensure((size_t)W * CNT_WORDS * sizeof(long long)));
  AMGCHK(d->cnt_recv.ensure((size_t)W * CNT_WORDS * sizeof(long long)));
  hipLaunchKernelGGL(k_dv_msg, dim3(1), dim3(1), 0, c->stream, d->dv_ok ? 1ll : 0ll, (long long)c->n_tokens,
                     (long long)d->attempt, d->dv_ok ? d->dv_D2 : -1ll, d->cnt_send.as<long long>());
  dist_xfer_ag(d, x, d->cnt_send.p, d->cnt_recv.p, CNT_WORDS * (int)sizeof(long long), 1, false);
  d->state = S_DV_ASK;
  return STEP_XFER;
}

static Step st_dv_ask(amg_ctx* c, DistState* d, amg_xfer* x) {
  const int W = d->world;
  AMGCHK(read_exchanged(c, d, CNT_WORDS, d->cnt_recv.p));
  const long long* got = reinterpret_cast<const long long*>(d->words.data());
  bool all_ok = true;
  for (int p = 0; p < W; ++p) all_ok = all_ok && got[(size_t)p * CNT_WORDS] == 1 && got[(size_t)p * CNT_WORDS + 3] == d->dv_D2;
  if (!all_ok) {  // somebody re-threaded a read (or disagrees about the graph): the ordinary merged build
    d->state = S_LOCAL;
    return STEP_ON;
  }
  for (int p = 0; p < W; ++p) d->tokens[p] = got[(size_t)p * CNT_WORDS + 1];
  set_token_base(c, d);
  const long long* nb = d->dv_bounds.data();
  const long long* pb = nb + W + 1;
  d->dv_mN = d->dv_mP = 0;
  for (int p = 0; p < W; ++p) {
    if (nb[p + 1] - nb[p] > d->dv_mN) d->dv_mN = nb[p + 1] - nb[p];
    if (pb[p + 1] - pb[p] > d->dv_mP) d->dv_mP = pb[p + 1] - pb[p];
  }
  const long long m = d->dv_mN + d->dv_mP;
  d->state = S_DV_FILL;
  if (m == 0) return STEP_ON;
  AMGCHK(d->held.ensure((size_t)m * sizeof(unsigned long long)));
  AMGCHK(d->gathered.ensure((size_t)W * (size_t)m * sizeof(unsigned long long)));
  const long long base = c->tok_base;
  hipLaunchKernelGGL(k_dv_contrib, dim3(nblk(m, 256)), dim3(256), 0, c->stream, c->alt_nfirst.as<long long>() + nb[d->rank],
                     nb[d->rank + 1] - nb[d->rank], (long long)(base << 1), c->alt_pfirst.as<unsigned long long>() + pb[d->rank],
                     pb[d->rank + 1] - pb[d->rank], (unsigned long long)base << 3, d->dv_mN, d->dv_mP,
                     d->held.as<unsigned long long>());
  dist_xfer_ag(d, x, d->held.p, d->gathered.p, (int)sizeof(unsigned long long), m, true);
  return STEP_XFER;
}

static Step st_dv_fill(amg_ctx* c, DistState* d, amg_xfer*) {
  const int W = d->world;
  const long long m = d->dv_mN + d->dv_mP;
  if (m > 0) {
    HIPCHK(hipMemcpyAsync(d->offs.p, d->dv_bounds.data(), (size_t)(2 * (W + 1)) * sizeof(long long), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_dv_fill, dim3(nblk(m * W, 256)), dim3(256), 0, c->stream, d->gathered.as<unsigned long long>(),
                       d->dv_mN, d->dv_mP, W, d->offs.as<long long>(), c->alt_nfirst.as<long long>(),
                       c->alt_pfirst.as<unsigned long long>());
  }
  return dv_done(c, d);
}

// ------------------------------------------------------------------ the driver
static constexpr decltype(&st_local) kStates[S_N] = {nullptr,    st_local,    st_counts, st_reduce, st_hold,
                                     st_hcounts, st_global, st_dv_local, st_dv_ask, st_dv_fill};

// runs the machine up to its next exchange.  1: *x is to be performed, then call again; 0: the build is complete
static int advance(amg_ctx* c, amg_xfer* x) {
  DistState* d = dist_state(c);
  for (;;) {
    if (d->state <= S_IDLE || d->state >= S_N) return amg_fail(AMG_E_STATE, "amg_dist_merge_begin first");
    phase_tick(c, d, d->kind * S_N + d->state);
    const Step s = kStates[d->state](c, d, x);
    if (s != STEP_ON) return s;
  }
}

extern "C" int amg_dist_merge_begin(amg_ctx* c, int32_t k, uint32_t min_node_cov, uint32_t min_edge_cov) {
  NEED_CTX(c);
  if (k < 1 || k > AMG_MAX_K) return amg_fail(AMG_E_ARG, "k must be in [1, %d]", AMG_MAX_K);
  if (c->two_v <= 0) return amg_fail(AMG_E_STATE, "amg_set_reads first");
  DistState* d = dist_state(c);
  d->k = k;
  d->mn = min_node_cov < 1 ? 1 : min_node_cov;
  d->me = min_edge_cov < 1 ? 1 : min_edge_cov;
  d->attempt = 0;
  d->kind = 0;
  d->fail_ret = 0;
  d->walk.state = W_IDLE;  // (a walk somebody abandoned ends here: the graph it asked about is being replaced)
  // the reads are what a correction left of the reads of the merged graph still held (amg_adopt_corrected), same k, plain
  // build: the ranks first find out whether that graph's live part will do (S_DV_*; AMG_NO_DERIVE=1: A/B + test switch)
  const bool candidate = c->dist_candidate && c->dist_mode && c->world == d->world && k == c->k && d->mn == 1 && d->me == 1 &&
                         !getenv("AMG_NO_DERIVE");  // (not c->sw: this build reads its switches later, in nodes_local)
  if (!candidate) (void)ctx_take_derive_offer(c);  // (declined; a candidate's offer is taken in st_dv_local)
  d->state = candidate ? S_DV_LOCAL : S_LOCAL;
  return AMG_OK;
}

extern "C" int amg_dist_merge_next(amg_ctx* c, amg_xfer* out) {
  NEED_CTX(c);
  if (!out) return amg_fail(AMG_E_ARG, "null xfer");
  DistState* d = dist_state(c);
  if (d->state == S_IDLE) return amg_fail(AMG_E_STATE, "amg_dist_merge_begin first");
  const int r = advance(c, out);
  if (r <= 0) d->state = S_IDLE;  // (complete, or failed: the one place that puts the machine to rest)
  phase_tick(c, d, -1);
  return r;
}

// ---- the exchanges over RCCL, on the ctx's stream
int dist_rccl_perform(amg_ctx* c, DistState* d, const amg_xfer& x) {
  hipStream_t st = c->stream;
  if (x.kind == AMG_XFER_ALL_GATHER) {
    NCCLCHK(g_rccl.AllGather(x.send, x.recv, (size_t)x.count * x.elem_bytes, ncclChar, d->comm, st));
    return AMG_OK;
  }
  const char* sp = static_cast<const char*>(x.send);
  char* rp = static_cast<char*>(x.recv);
  size_t so = 0, ro = 0;
  NCCLCHK(g_rccl.GroupStart());
  for (int p = 0; p < d->world; ++p) {
    const size_t sb = (size_t)x.send_counts[p] * x.elem_bytes, rb = (size_t)x.recv_counts[p] * x.elem_bytes;
    if (sb) NCCLCHK(g_rccl.Send(sp + so, sb, ncclChar, p, d->comm, st));
    if (rb) NCCLCHK(g_rccl.Recv(rp + ro, rb, ncclChar, p, d->comm, st));
    so += sb;
    ro += rb;
  }
  NCCLCHK(g_rccl.GroupEnd());
  return AMG_OK;
}

extern "C" int amg_dist_merge(amg_ctx* c, int32_t k, uint32_t min_node_cov, uint32_t min_edge_cov) {
  NEED_CTX(c);
  DistState* d = dist_state(c);
  if ((d->world > 1 || d->always_exchange) && !d->comm)
    return amg_fail(AMG_E_STATE, "amg_dist_init first (or drive the exchanges yourself: amg_dist_merge_begin / _next)");
  AMGCHK(amg_dist_merge_begin(c, k, min_node_cov, min_edge_cov));
  for (;;) {
    amg_xfer x;
    const int r = amg_dist_merge_next(c, &x);
    if (r <= 0) return r;
    const int e = dist_rccl_perform(c, d, x);
    if (e != AMG_OK) {
      d->state = S_IDLE;
      return e;
    }
  }
}

// ---- emulated ranks: the ctxs of one process, one device; the exchanges are device copies (the merge's and the walks')
int dist_local_exchange(amg_ctx* const* ctxs, int world, const amg_xfer* xs) {
  for (int r = 0; r < world; ++r) HIPCHK(hipStreamSynchronize(ctxs[r]->stream));
  hipStream_t st = ctxs[0]->stream;
  for (int r = 1; r < world; ++r)
    if (xs[r].kind != xs[0].kind || xs[r].elem_bytes != xs[0].elem_bytes)
      return amg_fail(AMG_E_DIST, "emulated ranks ask for different exchanges");
  const size_t eb = (size_t)xs[0].elem_bytes;
  if (xs[0].kind == AMG_XFER_ALL_GATHER) {
    for (int dst = 0; dst < world; ++dst)
      for (int src = 0; src < world; ++src) {
        if (xs[src].count != xs[0].count) return amg_fail(AMG_E_DIST, "all-gather sizes differ");
        if (xs[src].count)
          HIPCHK(hipMemcpyAsync(static_cast<char*>(xs[dst].recv) + (size_t)src * xs[0].count * eb, xs[src].send,
                                (size_t)xs[0].count * eb, hipMemcpyDeviceToDevice, st));
      }
  } else {
    for (int dst = 0; dst < world; ++dst) {
      size_t ro = 0;
      for (int src = 0; src < world; ++src) {
        size_t so = 0;
        for (int p = 0; p < dst; ++p) so += (size_t)xs[src].send_counts[p] * eb;
        const size_t bytes = (size_t)xs[src].send_counts[dst] * eb;
        if (xs[dst].recv_counts[src] != xs[src].send_counts[dst])
          return amg_fail(AMG_E_DIST, "all-to-all counts of ranks %d and %d disagree", src, dst);
        if (bytes)
          HIPCHK(hipMemcpyAsync(static_cast<char*>(xs[dst].recv) + ro, static_cast<const char*>(xs[src].send) + so, bytes,
                                hipMemcpyDeviceToDevice, st));
        ro += bytes;
      }
    }
  }
  HIPCHK(hipStreamSynchronize(st));
  return AMG_OK;
}

extern "C" int amg_dist_merge_local(amg_ctx* const* ctxs, int32_t world, int32_t k, uint32_t min_node_cov,
                                    uint32_t min_edge_cov) {
  if (!ctxs || world < 1) return amg_fail(AMG_E_ARG, "bad ctx list");
  for (int r = 0; r < world; ++r) {
    if (!ctxs[r]) return amg_fail(AMG_E_ARG, "null ctx");
    if (ctxs[r]->device != ctxs[0]->device) return amg_fail(AMG_E_ARG, "emulated ranks share one device");
    DistState* d = dist_state(ctxs[r]);
    if (d->world != world || d->rank != r || d->comm) AMGCHK(set_world(ctxs[r], r, world));
    AMGCHK(amg_dist_merge_begin(ctxs[r], k, min_node_cov, min_edge_cov));
  }
  HIPCHK(hipSetDevice(ctxs[0]->device));
  std::vector<amg_xfer> xs(world);
  auto abandon = [&](int ret) {
    const std::string msg = g_amg_err;
    for (int r = 0; r < world; ++r) dist_state(ctxs[r])->state = S_IDLE;
    g_amg_err = msg;
    return ret;
  };
  for (;;) {
    int pending = 0, done = 0, err = 0;
    std::string err_msg;
    for (int r = 0; r < world; ++r) {
      const int v = amg_dist_merge_next(ctxs[r], &xs[r]);
      if (v == 1) ++pending;
      else if (v == 0) ++done;
      else if (!err || err == AMG_E_DIST) {  // (a peer's "rank r failed" gives way to the failing rank's own message)
        err = v;
        err_msg = g_amg_err;
      }
    }
    if (err) {
      g_amg_err = err_msg;
      return abandon(err);
    }
    if (done == world) return AMG_OK;
    if (pending != world) return abandon(amg_fail(AMG_E_DIST, "emulated ranks fell out of step"));
    const int e = dist_local_exchange(ctxs, world, xs.data());
    if (e != AMG_OK) return abandon(e);
  }
}

// out[i]: the statistic DistStat i (amg_dist.h), since the last reset
extern "C" int amg_dist_stats(amg_ctx* c, int64_t* out, int32_t reset) {
  if (!c) return amg_fail(AMG_E_ARG, "null ctx");
  DistState* d = dist_state(c);
  if (out)
    for (int i = 0; i < DS_N; ++i) out[i] = d->st[i];
  if (reset)
    for (int i = 0; i < DS_N; ++i) d->st[i] = 0;
  return AMG_OK;
}

// synchronised wall time per phase of the driver since the last reset (on = 1 starts the measurement, which
// synchronises the stream around every phase): names[i] points at static strings; returns the number of phases
extern "C" int amg_dist_phase_ms(amg_ctx* c, int32_t on, const char** names, double* ms, int32_t cap) {
  if (!c) return amg_fail(AMG_E_ARG, "null ctx");
  DistState* d = dist_state(c);
  int n = 0;
  for (int i = 0; i < 2 * S_N; ++i) {
    if (!kPhaseNames[i][0]) continue;
    if (n < cap) {
      if (names) names[n] = kPhaseNames[i];
      if (ms) ms[n] = d->phase_ms[i];
    }
    ++n;
    d->phase_ms[i] = 0.0;
  }
  d->time_phases = on != 0;
  return n < cap ? n : cap;
}
