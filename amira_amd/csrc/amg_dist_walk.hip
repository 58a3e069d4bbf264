// amg_dist_walk.hip — the read walks of amg_read_walk.hip on a graph made by amg_dist_merge*: depth by read length (A),
// AMR trimming (B), AMR reads per component (C) over the reads of ALL ranks.  The node arrays, aliveness and component
// labels are the same on every rank, every rank has the node ids of its own reads' windows, and the reads are disjoint:
// each rank walks its reads (the local phases of amg_read_walk.h), the ranks exchange their parts, every rank folds them.
//
//   local    the rank's walk; its header (amg_dist_walk_hdr.h) is written on the device, A's sums behind it
//                                                                                    --> all-gather of the headers
//   judge    ONE read-back of all headers.  A rank whose local phase failed says so there, and arguments or graphs that
//            differ show there: then EVERY rank returns AMG_E_DIST, nothing has been removed, the machine rests.  The
//            size of what follows comes from the agreed header alone.  A is complete here: pairs summed over the ranks,
//            the alive nodes counted locally (the graph is replicated).
//            B: a bit per node, "a read of mine with a live AMR window has a live window on it"
//            C: n_reads[], n_long[] of the rank's reads                              --> all-gather of the parts
//   fold     B: the ranks' bitmaps are ORed, kill = alive and not kept, then finish_kill as amg_remove_non_amr_nodes:
//               every rank ends with the same graph and count, its own windows masked, its own reads marked
//            C: the ranks' counts are summed
//
// One all-gather for A, two for B and C; a graph without nodes (B) or components (C) needs no second one, on all ranks
// alike.  One rank without the test hook exchanges nothing.  The transports are the merge's (amg_dist.hip): RCCL
// (amg_dist_walk), device copies between emulated ranks (amg_dist_walk_local), or the caller's own (amg_dist_walk_begin /
// _next / _result).  This machine runs beside the merge's, never at the same time.
#include "amg_dist.h"
#include "amg_dist_walk_hdr.h"
#include "amg_read_walk.h"

static_assert(DW_DEPTH == AMG_WALK_DEPTH && DW_AMR_TRIM == AMG_WALK_AMR_TRIM && DW_COMPONENT_READS == AMG_WALK_COMPONENT_READS,
              "amg_dist_walk_hdr.h restates the AMG_WALK_* values");
static_assert(DW_DEPTH_LENGTHS == RW_MAX_LENGTHS, "the depth walk's sums travel behind its header");
#define DW_MSG_WORDS (DW_HDR_WORDS + RW_DEPTH_WORDS)  // this rank's message: header, pairs[16], alive nodes (not sent)

struct DwHdr {
  long long w[DW_HDR_WORDS];
};
__global__ void k_dw_header(DwHdr h, long long* __restrict__ msg) {
  if (threadIdx.x < DW_HDR_WORDS) msg[threadIdx.x] = h.w[threadIdx.x];
}

// keep bytes -> one bit per node, a 64-bit ballot per wave; bits[words], words = ceil(D / 64)
__global__ __launch_bounds__(256) void k_dw_pack_keep(const unsigned char* __restrict__ keep, long long D, long long words,
                                                      unsigned long long* __restrict__ bits) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long m = __ballot(i < D && keep[i] != 0);
  if ((threadIdx.x & 63) == 0 && (i >> 6) < words) bits[i >> 6] = m;
}

// all = world bitmaps of `words` words: a node any rank keeps stays; every kill byte below D is written
__global__ __launch_bounds__(256) void k_dw_fold_kill(const unsigned long long* __restrict__ all, int world, long long words,
                                                      const unsigned char* __restrict__ alive, long long D,
                                                      unsigned char* __restrict__ kill) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= D) return;
  unsigned long long m = 0;
  for (int r = 0; r < world; ++r) m |= all[(size_t)r * words + (i >> 6)];
  kill[i] = (alive[i] && !((m >> (i & 63)) & 1ull)) ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_dw_fold_sum(const unsigned long long* __restrict__ all, int world, long long n,
                                                     unsigned long long* __restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  unsigned long long s = 0;
  for (int r = 0; r < world; ++r) s += all[(size_t)r * n + i];
  out[i] = s;
}

// ------------------------------------------------------------------ the states
static const char* single_gpu_call(int which) {
  return which == AMG_WALK_DEPTH ? "amg_depth_by_length" : which == AMG_WALK_AMR_TRIM ? "amg_remove_non_amr_nodes" : "amg_component_amr_reads";
}

// the rank's walk and its part of the data exchange; every buffer up to the fold is made here
static int local_phase(amg_ctx* c, DistState* d, WalkState* w) {
  const int W = d->world;
  const long long D = c->n_nodes;
  switch (w->which) {
    case AMG_WALK_DEPTH:
      return rw_depth_local(c, w->min_genes.data(), w->n, w->msg.as<unsigned long long>() + DW_HDR_WORDS);
    case AMG_WALK_AMR_TRIM: {
      if (D == 0) return AMG_OK;
      const long long words = (D + 63) / 64;
      AMGCHK(w->send.ensure((size_t)words * sizeof(unsigned long long)));
      AMGCHK(w->recv.ensure((size_t)W * (size_t)words * sizeof(unsigned long long)));
      stage_begin(c, "amr_trim_local");
      AMGCHK(rw_keep_local(c, w->gene_flags.data(), &w->flag_words, &w->kept));
      hipLaunchKernelGGL(k_dw_pack_keep, dim3(nblk(words * 64, 256)), dim3(256), 0, c->stream, w->kept.keep, D, words,
                         w->send.as<unsigned long long>());
      stage_end(c);
      return AMG_OK;
    }
    default: {
      AMGCHK(ensure_components(c));
      const long long nc = c->n_components;
      w->hdr[DW_H_COMPS] = nc;
      if (nc == 0) return AMG_OK;
      AMGCHK(w->send.ensure(2 * (size_t)nc * sizeof(unsigned long long)));  // (the folded answer)
      AMGCHK(w->recv.ensure((size_t)W * 2 * (size_t)nc * sizeof(unsigned long long)));
      return rw_comp_local(c, w->gene_flags.data(), w->min_genes[0], &w->flag_words, &w->comp);
    }
  }
}

static int st_walk_local(amg_ctx* c, DistState* d, WalkState* w, amg_xfer* x) {
  stages_reset(c);
  const int r = local_phase(c, d, w);
  if (r != AMG_OK) {
    if (!dist_on_wire(d)) return r;
    w->fail_ret = r;  // (the peers are told in the header)
    w->fail_msg = g_amg_err;
  }
  w->hdr[DW_H_STATUS] = r;
  DwHdr h;
  for (int i = 0; i < DW_HDR_WORDS; ++i) h.w[i] = w->hdr[i];
  hipLaunchKernelGGL(k_dw_header, dim3(1), dim3(64), 0, c->stream, h, w->msg.as<long long>());
  w->state = W_JUDGE;
  if (!dist_on_wire(d)) return 2;
  dist_xfer_ag(d, x, w->msg.p, w->msg_all.p, (int)sizeof(long long), dw_first_words(w->which), w->which == AMG_WALK_DEPTH);
  return 1;
}

// device words to the host, through the mailbox while they fit one list
static int read_words(amg_ctx* c, const void* a, int n_a, const void* b, int n_b, int64_t* out) {
  if (n_a + n_b <= FETCH_MAX) {
    FetchList l;
    l.add_words(a, n_a);
    if (n_b) l.add_words(b, n_b);
    return fetch(c, l, reinterpret_cast<unsigned long long*>(out));
  }
  HIPCHK(hipMemcpyAsync(out, a, (size_t)n_a * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  if (n_b) HIPCHK(hipMemcpyAsync(out + n_a, b, (size_t)n_b * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return AMG_OK;
}

static int st_walk_judge(amg_ctx* c, DistState* d, WalkState* w, amg_xfer* x) {
  const bool wire = dist_on_wire(d);
  const int W = wire ? d->world : 1, self = wire ? d->rank : 0, stride = dw_first_words(w->which);
  std::vector<int64_t> got((size_t)W * stride + 1);
  // (the alive nodes of the depth walk lie behind this rank's own sums: read with the headers, never sent)
  AMGCHK(read_words(c, wire ? w->msg_all.p : w->msg.p, W * stride, w->msg.as<long long>() + DW_HDR_WORDS + RW_MAX_LENGTHS,
                    w->which == AMG_WALK_DEPTH ? 1 : 0, got.data()));
  ++d->st[DS_WAITS];
  char why[256];
  if (dw_judge(got.data(), W, stride, self, why, sizeof why) != 0) {
    if (w->fail_ret) return amg_fail(AMG_E_DIST, "walk across ranks abandoned: %s: %s", why, w->fail_msg.c_str());
    return amg_fail(AMG_E_DIST, "walk across ranks abandoned: %s", why);
  }
  const int64_t* mine = got.data() + (size_t)self * stride;
  for (int i = 0; i < DW_HDR_WORDS; ++i)
    if (mine[i] != w->hdr[i]) return amg_fail(AMG_E_DIST, "this rank's header came back changed: the exchange was not performed as asked");
  w->data_words = dw_data_words(mine);
  if (w->which == AMG_WALK_DEPTH) {
    w->result.assign((size_t)w->n + 1, 0);
    for (int r = 0; r < W; ++r)
      for (int j = 0; j < w->n; ++j) w->result[j] += got[(size_t)r * stride + DW_HDR_WORDS + j];
    w->result[w->n] = got[(size_t)W * stride];
    return 0;
  }
  if (w->data_words == 0) {  // no node to trim, no component to count in: on all ranks alike
    if (w->which == AMG_WALK_AMR_TRIM) w->result.assign(1, 0);
    else w->result.clear();
    return 0;
  }
  w->state = W_FOLD;
  if (!wire) return 2;
  const void* part = w->which == AMG_WALK_AMR_TRIM ? w->send.p : w->comp.n_reads;
  dist_xfer_ag(d, x, part, w->recv.p, (int)sizeof(unsigned long long), w->data_words, true);
  return 1;
}

static int st_walk_fold(amg_ctx* c, DistState* d, WalkState* w, amg_xfer*) {
  const bool wire = dist_on_wire(d);
  const int W = wire ? d->world : 1;
  const long long n = w->data_words;
  if (w->which == AMG_WALK_AMR_TRIM) {
    const long long D = c->n_nodes;
    const unsigned long long* all = wire ? w->recv.as<unsigned long long>() : w->send.as<unsigned long long>();
    AMGCHK(kill_marks_check(c, w->kept.marks));  // (the caller's exchanges ran since the local phase reserved them)
    ctx_removal_begins(c);  // (here, not at the walk's begin: a walk that finds no node to trim on any rank keeps the set)
    stage_begin(c, "amr_trim_fold");
    hipLaunchKernelGGL(k_dw_fold_kill, dim3(nblk(D, 256)), dim3(256), 0, c->stream, all, W, n, c->node_alive.as<unsigned char>(), D,
                       w->kept.marks.bytes);
    int64_t n_removed = 0;
    const int r = finish_kill(c, w->kept.marks, &n_removed, nullptr);
    stage_end(c);
    if (r != AMG_OK) return r;
    w->result.assign(1, n_removed);
    return 0;
  }
  const unsigned long long* all = wire ? w->recv.as<unsigned long long>() : w->comp.n_reads;
  stage_begin(c, "amr_reads_fold");
  hipLaunchKernelGGL(k_dw_fold_sum, dim3(nblk(n, 256)), dim3(256), 0, c->stream, all, W, n, w->send.as<unsigned long long>());
  stage_end(c);
  w->result.assign((size_t)n, 0);
  HIPCHK(hipMemcpyAsync(w->result.data(), w->send.p, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// ------------------------------------------------------------------ the driver
extern "C" int amg_dist_walk_begin(amg_ctx* c, int32_t which, const uint8_t* gene_flags, const int32_t* min_genes, int32_t n) {
  NEED_CTX(c);
  if (which != AMG_WALK_DEPTH && which != AMG_WALK_AMR_TRIM && which != AMG_WALK_COMPONENT_READS)
    return amg_fail(AMG_E_ARG, "which must be one of AMG_WALK_*");
  DistState* d = dist_state(c);
  WalkState* w = &d->walk;
  if (d->state != S_IDLE) return amg_fail(AMG_E_STATE, "a merged build is under way");
  if (w->state != W_IDLE) return amg_fail(AMG_E_STATE, "another walk is under way");
  if (!c->built) return amg_fail(AMG_E_STATE, "amg_dist_merge first");
  if (!c->dist_mode)
    return amg_fail(AMG_E_STATE, "the graph is not from a merged build: this ctx holds all its reads, %s answers for them",
                    single_gpu_call(which));
  if (c->world != d->world)
    return amg_fail(AMG_E_STATE, "the graph was merged over %d ranks, the ctx is now a rank of %d", c->world, d->world);
  const bool wants_flags = which != AMG_WALK_DEPTH, wants_lengths = which != AMG_WALK_AMR_TRIM;
  if ((wants_flags && !gene_flags) || (wants_lengths && !min_genes)) return amg_fail(AMG_E_ARG, "null argument");
  if (which == AMG_WALK_DEPTH && (n < 1 || n > RW_MAX_LENGTHS)) return amg_fail(AMG_E_ARG, "n must be in [1, %d]", RW_MAX_LENGTHS);
  if (which == AMG_WALK_COMPONENT_READS && n != 1) return amg_fail(AMG_E_ARG, "one min_genes value (n = 1) for the component reads");
  const int V = c->two_v / 2;
  w->which = which;
  w->n = wants_lengths ? n : 0;
  w->min_genes.clear();
  w->gene_flags.clear();
  if (wants_lengths) w->min_genes.assign(min_genes, min_genes + n);
  if (wants_flags) w->gene_flags.assign(gene_flags, gene_flags + V);
  w->fail_ret = 0;
  w->fail_msg.clear();
  w->have_result = false;
  w->result.clear();
  w->data_words = 0;
  w->kept = RwKeep();
  w->comp = RwComp();
  w->hdr[DW_H_WHICH] = which;
  w->hdr[DW_H_STATUS] = 0;
  w->hdr[DW_H_K] = c->k;
  w->hdr[DW_H_N] = w->n;
  w->hdr[DW_H_NODES] = c->n_nodes;
  w->hdr[DW_H_COMPS] = 0;
  w->hdr[DW_H_HASH] = (int64_t)dw_hash_args(wants_flags ? w->gene_flags.data() : nullptr, V,
                                            wants_lengths ? w->min_genes.data() : nullptr, w->n);
  w->hdr[DW_H_TWO_V] = c->two_v;
  // the two message buffers exist before anything can fail on this rank alone: a failing rank still sends its header
  AMGCHK(w->msg.ensure(DW_MSG_WORDS * sizeof(long long)));
  AMGCHK(w->msg_all.ensure((size_t)d->world * (DW_HDR_WORDS + RW_MAX_LENGTHS) * sizeof(long long)));
  w->state = W_LOCAL;
  return AMG_OK;
}

// runs the machine up to its next exchange.  1: *x is to be performed, then call again; 0: the answer is there
extern "C" int amg_dist_walk_next(amg_ctx* c, amg_xfer* out) {
  NEED_CTX(c);
  if (!out) return amg_fail(AMG_E_ARG, "null xfer");
  DistState* d = dist_state(c);
  WalkState* w = &d->walk;
  if (w->state == W_IDLE) return amg_fail(AMG_E_STATE, "amg_dist_walk_begin first");
  int r = 2;
  while (r == 2) {  // (2: the next state at once)
    switch (w->state) {
      case W_LOCAL: r = st_walk_local(c, d, w, out); break;
      case W_JUDGE: r = st_walk_judge(c, d, w, out); break;
      case W_FOLD: r = st_walk_fold(c, d, w, out); break;
      default: r = amg_fail(AMG_E_STATE, "amg_dist_walk_begin first");
    }
  }
  if (r <= 0) w->state = W_IDLE;  // (complete, or failed: the one place that puts the machine to rest)
  if (r == 0) w->have_result = true;
  return r;
}

extern "C" int amg_dist_walk_result(amg_ctx* c, int64_t* out, int64_t cap, int64_t* n_out) {
  if (!c) return amg_fail(AMG_E_ARG, "null ctx");
  if (!n_out) return amg_fail(AMG_E_ARG, "null argument");
  const WalkState* w = &dist_state(c)->walk;
  if (!w->have_result) return amg_fail(AMG_E_STATE, "no walk of this ctx has been completed");
  const int64_t n = (int64_t)w->result.size();
  *n_out = n;
  if (cap < n) return amg_fail(AMG_E_ARG, "room for %lld values, the answer has %lld", (long long)cap, (long long)n);
  if (n && !out) return amg_fail(AMG_E_ARG, "null argument");
  if (n) memcpy(out, w->result.data(), (size_t)n * sizeof(int64_t));
  return AMG_OK;
}

extern "C" int amg_dist_walk(amg_ctx* c, int32_t which, const uint8_t* gene_flags, const int32_t* min_genes, int32_t n,
                             int64_t* out, int64_t cap, int64_t* n_out) {
  NEED_CTX(c);
  DistState* d = dist_state(c);
  if (dist_on_wire(d) && !d->comm)
    return amg_fail(AMG_E_STATE, "amg_dist_init first (or drive the exchanges yourself: amg_dist_walk_begin / _next)");
  AMGCHK(amg_dist_walk_begin(c, which, gene_flags, min_genes, n));
  for (;;) {
    amg_xfer x;
    const int r = amg_dist_walk_next(c, &x);
    if (r < 0) return r;
    if (r == 0) break;
    const int e = dist_rccl_perform(c, d, x);
    if (e != AMG_OK) {
      d->walk.state = W_IDLE;
      return e;
    }
  }
  return amg_dist_walk_result(c, out, cap, n_out);
}

extern "C" int amg_dist_walk_local(amg_ctx* const* ctxs, int32_t world, int32_t which, const uint8_t* gene_flags,
                                   const int32_t* min_genes, int32_t n, int64_t* out, int64_t cap, int64_t* n_out) {
  if (!ctxs || world < 1) return amg_fail(AMG_E_ARG, "bad ctx list");
  for (int r = 0; r < world; ++r) {
    if (!ctxs[r]) return amg_fail(AMG_E_ARG, "null ctx");
    if (ctxs[r]->device != ctxs[0]->device) return amg_fail(AMG_E_ARG, "emulated ranks share one device");
  }
  auto abandon = [&](int ret) {
    const std::string msg = g_amg_err;
    for (int r = 0; r < world; ++r) dist_state(ctxs[r])->walk.state = W_IDLE;
    g_amg_err = msg;
    return ret;
  };
  for (int r = 0; r < world; ++r) {
    const int e = amg_dist_walk_begin(ctxs[r], which, gene_flags, min_genes, n);
    if (e != AMG_OK) return abandon(e);
    const DistState* d = dist_state(ctxs[r]);
    if (d->world != world || d->rank != r)
      return abandon(amg_fail(AMG_E_ARG, "ctx %d is rank %d of %d: hand over the ctxs of the merged build in rank order", r,
                              d->rank, d->world));
  }
  HIPCHK(hipSetDevice(ctxs[0]->device));
  std::vector<amg_xfer> xs(world);
  for (;;) {
    int pending = 0, done = 0, err = 0;
    std::string err_msg;
    for (int r = 0; r < world; ++r) {  // (every rank hears the verdict, also after the first error)
      const int v = amg_dist_walk_next(ctxs[r], &xs[r]);
      if (v == 1) ++pending;
      else if (v == 0) ++done;
      else if (!err) {
        err = v;
        err_msg = g_amg_err;
      }
    }
    if (err) {
      g_amg_err = err_msg;
      return abandon(err);
    }
    if (done == world) break;
    if (pending != world) return abandon(amg_fail(AMG_E_DIST, "emulated ranks fell out of step"));
    const int e = dist_local_exchange(ctxs, world, xs.data());
    if (e != AMG_OK) return abandon(e);
  }
  for (int r = 1; r < world; ++r)
    if (dist_state(ctxs[r])->walk.result != dist_state(ctxs[0])->walk.result)
      return amg_fail(AMG_E_DIST, "rank %d folded another answer than rank 0", r);
  return amg_dist_walk_result(ctxs[0], out, cap, n_out);
}
