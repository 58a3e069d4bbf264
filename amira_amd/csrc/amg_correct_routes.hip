// amg_correct_routes.hip — the route report of amg_correct_reads (test hook, AMG_CORR_ROUTES=1): how many reads took
// which tier of the re-threading and of the position carry-over, and why a read left a tier.  Nothing here runs in a
// call without the switch: the tallies are small kernels of their own behind the steps, over what the steps left
// anyway (need_slow and the lean kernel's flags with their reason codes, the memo's answers, the NwRec records, the
// carry-over's scratch sizes, final_cls), and one extra read-back at the end of the call.  (A unit of its own so
// that no kernel of the correction is compiled next to it.)
#include "amg_correct.h"

// one thread per gapped read; a test hook: plain global atomics
__global__ __launch_bounds__(256) void k_route_gapped(long long n_gapped, const int* __restrict__ gapped,
                                                      const unsigned char* __restrict__ need_slow,
                                                      const unsigned char* __restrict__ lean_left /*nullptr: not run*/,
                                                      const int* __restrict__ gq /*nullptr: no memo*/,
                                                      const unsigned char* __restrict__ final_cls,
                                                      unsigned long long* out) {
  const long long gi = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gi >= n_gapped) return;
  atomicAdd(out + AMG_ROUTE_GAPPED, 1ull);
  const unsigned int why = need_slow[gi];
  const unsigned int lean = lean_left ? lean_left[gi] : 0u;
  if (why != 0u) {
    atomicAdd(out + AMG_ROUTE_BY_GENERAL, 1ull);
    if (why < GS_CODES) atomicAdd(out + AMG_ROUTE_ON_NOT_TRIED + (why - GS_NOT_TRIED), 1ull);
  } else if (lean_left && lean == 0u) {
    atomicAdd(out + AMG_ROUTE_BY_LEAN, 1ull);
  } else {
    atomicAdd(out + AMG_ROUTE_BY_FAST, 1ull);
  }
  if (lean != 0u && lean < GL_CODES) atomicAdd(out + AMG_ROUTE_LEAN_NO_SLOTS + (lean - GL_NO_SLOTS), 1ull);
  if (!gq || gq[gi * GF_MAXGAP] < 0) atomicAdd(out + AMG_ROUTE_NO_MEMO_SLOTS, 1ull);
  if (final_cls[gapped[gi]] == RC_KEEP_ORIG) atomicAdd(out + AMG_ROUTE_KEEP_ORIG, 1ull);
}

// one thread per question of the path memo
__global__ __launch_bounds__(256) void k_route_memo(long long n_queries, const int* __restrict__ qlist,
                                                    const int4* __restrict__ qres, unsigned long long* out) {
  const long long qi = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (qi >= n_queries) return;
  const int4 res = qres[qlist[qi]];
  atomicAdd(out + AMG_ROUTE_MEMO_QUESTIONS, 1ull);
  if (res.y < 0) atomicAdd(out + AMG_ROUTE_MEMO_UNFIT, 1ull);
  if (res.y > GM_INLINE) atomicAdd(out + AMG_ROUTE_MEMO_SPILLED, 1ull);
}

// one thread per gapped read: who carried its positions over.  This is the SIZING decision: what k_nw_sizes wrote — a
// record with N > 0 is the fast kernel's, scratch bytes mean the general kernel away from its LDS matrix.  k_corr_nw
// decides LDS against scratch by the same rule (nw_in_lds, amg_correct.h).
__global__ __launch_bounds__(256) void k_route_nw(long long n_gapped, const NwRec* __restrict__ rec,
                                                  const long long* __restrict__ nw_size,
                                                  const unsigned char* __restrict__ final_cls,
                                                  unsigned long long* out) {
  const long long gi = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gi >= n_gapped) return;
  const NwRec q = rec[gi];
  if (final_cls[q.r] == RC_KEEP_ORIG) return;  // original genes and positions kept: no carry-over
  atomicAdd(out + (q.N > 0 ? AMG_ROUTE_NW_FAST : nw_size[gi] > 0 ? AMG_ROUTE_NW_GLOBAL : AMG_ROUTE_NW_LDS), 1ull);
}

int routes_begin(amg_ctx* c) {
  c->have_routes = false;
  AMGCHK(c->routes_dev.ensure(AMG_ROUTE_WORDS * sizeof(unsigned long long)));
  ClearList cl;
  cl.add(c->routes_dev.p, AMG_ROUTE_WORDS * sizeof(unsigned long long));
  return clear_many(c, cl);
}

int routes_gapped(amg_ctx* c, const CorrScratch& S, const CorrCounts& n, const unsigned char* need_slow, const int* gq) {
  unsigned long long* out = c->routes_dev.as<unsigned long long>();
  hipLaunchKernelGGL(k_route_gapped, dim3(nblk(n.n_gapped, 256)), dim3(256), 0, c->stream, n.n_gapped,
                     S.glist->as<int>(), need_slow, n.lean_ran ? c->gm_fail.as<unsigned char>() : nullptr, gq,
                     S.final_cls, out);
  if (n.n_queries > 0)
    hipLaunchKernelGGL(k_route_memo, dim3(nblk(n.n_queries, 256)), dim3(256), 0, c->stream, n.n_queries,
                       c->gm_list.as<int>(), c->gm_res.as<int4>(), out);
  return AMG_OK;
}

int routes_nw(amg_ctx* c, const CorrScratch& S, const CorrCounts& n) {
  hipLaunchKernelGGL(k_route_nw, dim3(nblk(n.n_gapped, 256)), dim3(256), 0, c->stream, n.n_gapped,
                     c->nw_rec.as<NwRec>(), S.nw_size, S.final_cls, c->routes_dev.as<unsigned long long>());
  return AMG_OK;
}

int routes_end(amg_ctx* c, const CorrCounts& n) {
  FetchList l;
  l.add_words(c->routes_dev.p, AMG_ROUTE_WORDS);
  unsigned long long v[AMG_ROUTE_WORDS];
  AMGCHK(fetch(c, l, v));
  for (int i = 0; i < AMG_ROUTE_WORDS; ++i) c->routes[i] = (int64_t)v[i];
  c->routes[AMG_ROUTE_POOL_RETRIES] = n.pool_retries;  // (the host counts its own attempts)
  c->have_routes = true;
  return AMG_OK;
}

extern "C" int amg_correct_routes(amg_ctx* c, int64_t* out, int32_t cap) {
  if (!c || !out || cap < 0) return amg_fail(AMG_E_ARG, "correct_routes: bad arguments");
  if (!c->have_routes)
    return amg_fail(AMG_E_STATE, "correct_routes: the last amg_correct_reads ran without AMG_CORR_ROUTES=1");
  for (int i = 0; i < cap && i < AMG_ROUTE_WORDS; ++i) out[i] = c->routes[i];
  return AMG_OK;
}
