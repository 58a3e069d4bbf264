// amg_nw_probe.hip — amg_nw_probe (include/amg.h), the position carry-over's test entry: one carry-over per pair of host
// arrays through the calls amg_correct_reads makes (amg_correct_nw.hip by way of amg_correct.h).  No kernel lives here.
#include "amg_correct.h"

// The context's position pools and what fill_pos_args reads of it, lent to the probe for one call: the probe's own
// arrays stand in, and the destructor frees them and puts the context back as it was.
struct NwProbeLoan {
  amg_ctx* c;
  DevBuf gene_start, gene_end, pos_off, pos1_s, pos1_e;
  bool have_pos, pos_identity;
  int64_t pos_n0, pos1_used;
  explicit NwProbeLoan(amg_ctx* ctx)
      : c(ctx), gene_start(ctx->gene_start), gene_end(ctx->gene_end), pos_off(ctx->pos_off), pos1_s(ctx->pos1_s),
        pos1_e(ctx->pos1_e), have_pos(ctx->have_pos), pos_identity(ctx->pos_identity), pos_n0(ctx->pos_n0),
        pos1_used(ctx->pos1_used) {
    c->gene_start = c->gene_end = c->pos_off = c->pos1_s = c->pos1_e = DevBuf();
  }
  ~NwProbeLoan() {
    c->gene_start.release(), c->gene_end.release(), c->pos_off.release(), c->pos1_s.release(), c->pos1_e.release();
    c->gene_start = gene_start, c->gene_end = gene_end, c->pos_off = pos_off, c->pos1_s = pos1_s, c->pos1_e = pos1_e;
    c->have_pos = have_pos, c->pos_identity = pos_identity, c->pos_n0 = pos_n0, c->pos1_used = pos1_used;
  }
};
// the probe's own device arrays
struct NwProbeBufs {
  DevBuf tokens, read_off, tmp_tok, tmp_off, new_len, final_cls, read_len, glist, sizes, places, route;
  ~NwProbeBufs() {
    for (DevBuf* b : {&tokens, &read_off, &tmp_tok, &tmp_off, &new_len, &final_cls, &read_len, &glist, &sizes, &places,
                      &route})
      b->release();
  }
};
static int probe_up(DevBuf& b, const void* src, size_t bytes, size_t room = 0) {
  AMGCHK(b.ensure(bytes + room + 16));
  if (bytes) HIPCHK(hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
  return AMG_OK;
}

#define NWP_GUARD 64      // guard words behind the produced positions and behind the staged genes
#define NWP_GUARD_PRE 8   // and in front of the produced positions
#define NWP_N0_POOLED 5   // entries of the caller's pool when the originals live in the pool of produced positions
extern "C" int amg_nw_probe(amg_ctx* c, int64_t n_pairs, const int32_t* x_tok, const int64_t* x_off, const int32_t* y_tok,
                            const int64_t* y_off, const int64_t* y_start, const int64_t* y_end, const int64_t* read_len,
                            const uint8_t* keep_orig, int flags, int64_t* out_start, int64_t* out_end, uint8_t* route,
                            int64_t* state) {
  if (!c || n_pairs < 1 || n_pairs > (1ll << 20) || !x_off || !y_tok || !y_off || !y_start || !y_end || !route || !state ||
      flags < 0 || flags > 7 || x_off[0] != 0 || y_off[0] != 0)
    return amg_fail(AMG_E_ARG, "nw_probe: bad arguments");
  // what the kernels cannot take is refused here: nothing is launched for it
  long long want_pos = 0, want_big = 0;
  for (int64_t p = 0; p < n_pairs; ++p) {
    const long long N = x_off[p + 1] - x_off[p], M = y_off[p + 1] - y_off[p];
    const bool keep = keep_orig && keep_orig[p];
    if (N < 0 || M < 1 || (N < 1 && !keep) || N > (1 << 24) || M > (1 << 24))
      return amg_fail(AMG_E_ARG, "nw_probe: pair %lld has %lld corrected and %lld original genes", (long long)p, N, M);
    if (keep) continue;
    want_pos += N;
    if (!nw_in_lds(N, M)) want_big += N * M + 16 * (N + M) + 64;  // (more than nw_scratch_bytes, on purpose)
    if (want_big > (1ll << 30)) return amg_fail(AMG_E_ARG, "nw_probe: more than 1 GiB of matrix scratch");
  }
  const long long total_x = x_off[n_pairs], total_y = y_off[n_pairs];
  if (total_x > 0 && !x_tok) return amg_fail(AMG_E_ARG, "nw_probe: no corrected genes");
  if (want_pos > 0 && (!out_start || !out_end)) return amg_fail(AMG_E_ARG, "nw_probe: no room for the positions");
  for (long long i = 0; i < total_x; ++i)
    if (x_tok[i] < 0) return amg_fail(AMG_E_ARG, "nw_probe: negative corrected gene at %lld", i);
  for (long long i = 0; i < total_y; ++i)
    if (y_tok[i] < 0) return amg_fail(AMG_E_ARG, "nw_probe: negative original gene at %lld", i);
  HIPCHK(hipSetDevice(c->device));

  const bool pooled = (flags & 4) != 0;
  NwProbeLoan loan(c);
  NwProbeBufs B;
  CorrSwitches sw = {};
  sw.fast_nw = (flags & 1) ? 0 : 1;
  sw.nw_shortcuts = (flags & 2) ? 0 : 1;
  // ---- the read set, the staged genes and the classes, as amg_correct_reads has them before its shape step
  std::vector<unsigned int> new_len((size_t)n_pairs);
  std::vector<unsigned char> cls((size_t)n_pairs);
  std::vector<int> glist((size_t)n_pairs);
  for (int64_t p = 0; p < n_pairs; ++p) {
    new_len[p] = (unsigned int)(x_off[p + 1] - x_off[p]);
    cls[p] = (keep_orig && keep_orig[p]) ? RC_KEEP_ORIG : RC_GAPPED;
    glist[p] = (int)p;
  }
  const size_t np1 = (size_t)n_pairs + 1;
  AMGCHK(probe_up(B.tokens, y_tok, (size_t)total_y * 4));
  AMGCHK(probe_up(B.read_off, y_off, np1 * 8));
  AMGCHK(probe_up(B.tmp_tok, x_tok, (size_t)total_x * 4, NWP_GUARD * 4));
  HIPCHK(hipMemset(B.tmp_tok.as<int>() + total_x, 0xff, NWP_GUARD * 4));
  AMGCHK(probe_up(B.tmp_off, x_off, np1 * 8));
  AMGCHK(probe_up(B.new_len, new_len.data(), (size_t)n_pairs * 4));
  AMGCHK(probe_up(B.final_cls, cls.data(), (size_t)n_pairs));
  if (read_len) AMGCHK(probe_up(B.read_len, read_len, (size_t)n_pairs * 8));
  AMGCHK(probe_up(B.glist, glist.data(), (size_t)n_pairs * 4));
  AMGCHK(B.sizes.ensure((n_pairs + 2) * 2 * sizeof(long long)));
  AMGCHK(B.places.ensure((n_pairs + 2) * 3 * sizeof(long long)));
  AMGCHK(B.route.ensure((size_t)n_pairs + 16));
  HIPCHK(hipMemset(B.route.p, 0, (size_t)n_pairs));
  // ---- the positions of the original genes: the caller's pool, or the pool of produced positions with NWP_GUARD_PRE
  // guard words behind them; that pool is allocated for what it holds and no more, so that this call's products have
  // grow_keep move it (state[4] says whether it did)
  const long long used = (pooled ? total_y : 0) + NWP_GUARD_PRE;
  {
    std::vector<long long> ps((size_t)used, -1ll), pe((size_t)used, -1ll);
    if (pooled) {
      memcpy(ps.data(), y_start, (size_t)total_y * 8);
      memcpy(pe.data(), y_end, (size_t)total_y * 8);
      const long long filler[NWP_N0_POOLED] = {-1, -1, -1, -1, -1};
      std::vector<long long> off((size_t)n_pairs);
      for (int64_t p = 0; p < n_pairs; ++p) off[p] = NWP_N0_POOLED + y_off[p];
      AMGCHK(probe_up(c->gene_start, filler, sizeof(filler)));
      AMGCHK(probe_up(c->gene_end, filler, sizeof(filler)));
      AMGCHK(probe_up(c->pos_off, off.data(), (size_t)n_pairs * 8));
    } else {
      AMGCHK(probe_up(c->gene_start, y_start, (size_t)total_y * 8));
      AMGCHK(probe_up(c->gene_end, y_end, (size_t)total_y * 8));
    }
    AMGCHK(c->pos1_s.ensure((size_t)used * 8));
    AMGCHK(c->pos1_e.ensure((size_t)used * 8));
    HIPCHK(hipMemcpy(c->pos1_s.p, ps.data(), (size_t)used * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->pos1_e.p, pe.data(), (size_t)used * 8, hipMemcpyHostToDevice));
  }
  c->have_pos = true;
  c->pos_identity = !pooled;
  c->pos_n0 = pooled ? NWP_N0_POOLED : total_y;
  c->pos1_used = used;
  HIPCHK(hipDeviceSynchronize());

  CorrScratch S;
  S.per_read = (size_t)n_pairs + 2;
  S.final_cls = B.final_cls.as<unsigned char>();
  S.nw_size = B.sizes.as<long long>();
  S.nw_off = S.nw_size + (n_pairs + 2);
  S.new_len = B.new_len.as<unsigned int>();
  S.tmp_off = B.tmp_off.as<long long>();
  S.tmp_tok = B.tmp_tok.as<int>();
  S.plen = B.places.as<long long>();
  S.poffs = S.plen + (n_pairs + 2);
  S.pos_new = S.poffs + (n_pairs + 2);
  S.n_general = c->status.as<unsigned long long>() + ST_MISC;
  S.glist = &B.glist;
  CorrArgs a;
  memset(&a, 0, sizeof(a));
  a.tokens = B.tokens.as<int>();
  a.read_off = B.read_off.as<long long>();
  fill_pos_args(c, a);
  a.read_len = read_len ? B.read_len.as<long long>() : nullptr;
  a.n_reads = n_pairs;
  a.have_pos = 1;
  a.cls_final = S.final_cls;
  a.tmp_off = S.tmp_off;
  a.new_len = S.new_len;
  a.tmp_tok = S.tmp_tok;
  // ---- the shape step's part, the pools, the kernels: the calls amg_correct_reads makes
  CorrCounts n;
  n.n_gapped = n_pairs;
  n.carry = true;
  FetchList shape;
  AMGCHK(corr_nw_sizes(c, sw, S, a, n_pairs, shape));
  unsigned long long v[3] = {0, 0, 0};
  AMGCHK(fetch(c, shape, v));
  n.big_total = (long long)v[0];
  n.pos_total = (long long)v[1];
  n.n_general = v[2];
  const void* pool_before = c->pos1_s.p;
  AMGCHK(corr_grow_pos_pools(c, n));
  fill_pos_args(c, a);
  const long long span = n.pos_total + NWP_GUARD;  // corr_grow_pos_pools leaves 64 entries behind the products
  HIPCHK(hipMemsetAsync(c->pos1_s.as<long long>() + used, 0xff, (size_t)span * 8, c->stream));
  HIPCHK(hipMemsetAsync(c->pos1_e.as<long long>() + used, 0xff, (size_t)span * 8, c->stream));
  AMGCHK(corr_positions(c, sw, S, a, n, B.route.as<unsigned char>()));
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));

  // ---- what came of it
  std::vector<long long> gs((size_t)(used + span)), ge((size_t)(used + span)), nw_size((size_t)n_pairs);
  std::vector<NwRec> rec((size_t)n_pairs);
  std::vector<int> tail(NWP_GUARD);
  HIPCHK(hipMemcpy(gs.data(), c->pos1_s.p, gs.size() * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(ge.data(), c->pos1_e.p, ge.size() * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(nw_size.data(), S.nw_size, (size_t)n_pairs * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(rec.data(), c->nw_rec.p, (size_t)n_pairs * sizeof(NwRec), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(route, B.route.p, (size_t)n_pairs, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(tail.data(), B.tmp_tok.as<int>() + total_x, NWP_GUARD * 4, hipMemcpyDeviceToHost));
  bool intact = true;
  for (long long i = 0; i < used; ++i) {
    const bool orig = pooled && i < total_y;
    if (gs[i] != (orig ? y_start[i] : -1ll) || ge[i] != (orig ? y_end[i] : -1ll)) intact = false;
  }
  for (long long i = used + n.pos_total; i < used + span; ++i)
    if (gs[i] != -1ll || ge[i] != -1ll) intact = false;
  for (int i = 0; i < NWP_GUARD; ++i)
    if (tail[i] != -1) intact = false;
  const long long take = n.pos_total < want_pos ? n.pos_total : want_pos;
  if (take > 0) {
    memcpy(out_start, gs.data() + used, (size_t)take * 8);
    memcpy(out_end, ge.data() + used, (size_t)take * 8);
  }
  for (int64_t p = 0; p < n_pairs; ++p)  // the general kernel's pairs: by the record and the size k_nw_sizes made
    if (cls[p] != RC_KEEP_ORIG && rec[p].N == 0) route[p] = nw_size[p] > 0 ? NW_ROUTE_GLOBAL : NW_ROUTE_LDS;
  state[0] = n.big_total;
  state[1] = n.pos_total;
  state[2] = (int64_t)n.n_general;
  state[3] = intact ? 1 : 0;
  state[4] = c->pos1_s.p != pool_before ? 1 : 0;
  return AMG_OK;
}
