// amg_correct_gapped.hip — re-threading of the reads with None runs (stage correct_gapped of amg_correct_reads;
// reference construct_graph.py:1166-1203, 1297-1310, 1331-1386, 2292-2342): the list of the gapped reads and the host
// function that runs the stage.  (Pipeline: amg_correct.hip.)  Its parts live with their kernels:
//   amg_gap_memo.hip      k_gap_queries, k_gap_dfs, k_gap_dfs_lanes   the path memo: every distinct question of the
//                                                                     None runs answered once
//   amg_gap_lean.hip      k_corr_gapped_lean   sixteen lanes per read: the reads whose every question has one answer
//   amg_gap_fast.hip      gf_* steps, gapped_fast_read, k_corr_gapped_fast   a wave per read, staged in LDS (GfLds)
//   amg_gap_general.hip   dfs_paths, k_corr_gapped   the general kernel: a thread per read, its search stack in
//                                                    private arrays
// (The None runs of a live-window mask: gap_run_ends / gap_run_terminals in amg_correct.h.)
// (dfs_paths_wave — the re-threading's visitor on the wave-cooperative search —, oriented_tok, cand_better and the
// memo's question key: amg_gap_search.h.)
#include "amg_correct.h"

// list of the gapped reads (in read order) and, per gapped read, the record the gapped kernels start from
__global__ void k_scatter_gapped(const unsigned int* __restrict__ flag, const long long* __restrict__ pos,
                                 long long n_reads, int* __restrict__ out, const long long* __restrict__ read_off,
                                 const int* __restrict__ r_start, const int* __restrict__ r_end,
                                 const long long* __restrict__ tmp_off, const unsigned long long* __restrict__ lmask,
                                 GapRec* __restrict__ rec) {
  long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_reads || !flag[r]) return;
  const long long gi = pos[r];
  out[gi] = (int)r;
  GapRec q;
  q.r = (int)r;
  q.t0 = read_off[r];
  const long long len = read_off[r + 1] - q.t0;
  q.L0 = (int)(len > 0x7fffffff ? 0x7fffffff : len);
  q.start = r_start[r];
  q.end = r_end[r];
  q.dst = tmp_off[r];
  q.mask = lmask[r];
  q.pad = 0;
  rec[gi] = q;
}

// ------------------------------------------------------------------ stage correct_gapped
// THE place where the gapped kernels' arguments are made (gq: the memo's question slots, nullptr without memo)
static GapArgs gap_args(amg_ctx* c, const CorrScratch& S, const CorrArgs& a, const CorrCounts& n, const int* gq,
                        const GeneralRoom& room) {
  GapArgs G;
  G.a = a;
  G.g = make_view(c);
  G.rec = c->gap_rec.as<GapRec>();
  G.gapped_reads = S.glist->as<int>();
  G.n_gapped = n.n_gapped;
  G.pool = S.pool->as<int>();
  G.pool_cap = room.pool_cap;
  G.pool_used = c->status.as<unsigned long long>() + ST_COMPACT_A;
  G.status = c->status.as<unsigned long long>();
  G.cand = S.cand->as<int>();
  G.cand_stride = room.cand_stride;
  G.final_cls = S.final_cls;
  G.need_slow = S.need_slow->as<unsigned char>();
  G.gq = gq;
  G.qres = c->gm_res.as<int4>();
  G.qpool = c->gm_pool.as<int>();
  return G;
}

// Who hands what to whom: k_corr_gapped_lean (sixteen lanes per read) does the reads whose every question has one
// answer and flags the others in gm_fail; k_corr_gapped_fast (a wave per read, LDS staging) does those — or, without
// memo or lean kernel, every read — and flags in need_slow what exceeds its capacities; k_corr_gapped (a thread per
// read, global pool and candidate scratch) does the flagged rest and is the one that may ask for a larger pool.
int corr_gapped(amg_ctx* c, const CorrSwitches& sw, const CorrScratch& S, const CorrArgs& a, CorrCounts& n) {
  const long long R = c->n_reads, n_gapped = n.n_gapped;
  AMGCHK(S.glist->ensure((size_t)(n_gapped + 1) * sizeof(int)));
  AMGCHK(c->gap_rec.ensure((size_t)(n_gapped + 1) * sizeof(GapRec)));
  hipLaunchKernelGGL(k_scatter_gapped, dim3(nblk(R, 256)), dim3(256), 0, c->stream, S.flag, S.new_idx, R,
                     S.glist->as<int>(), a.read_off, S.r_start, S.r_end, S.tmp_off, a.lmask, c->gap_rec.as<GapRec>());
  const int* gq = nullptr;
  if (n.total_runs > 0 && sw.gap_memo) AMGCHK(corr_gap_memo(c, sw, a, n, &gq));
  GeneralRoom room;
  AMGCHK(corr_general_room(c, sw, S, n, room));
  GapArgs G = gap_args(c, S, a, n, gq, room);
  {
    ClearList gcl;
    gcl.add(c->status.p, ST_WORDS * sizeof(unsigned long long));
    gcl.add(G.need_slow, ((size_t)n_gapped + 4) & ~(size_t)3, sw.fast_gapped ? 0u : 0x01010101u);  // (the buffer has 64 spare bytes)
    AMGCHK(clear_many(c, gcl));
  }
  if (sw.fast_gapped && gq && sw.lean_gapped) {
    // (no count of the flagged reads comes back to the host; AMG_CORR_ROUTES tallies them for tests)
    n.lean_ran = true;
    AMGCHK(c->gm_fail.ensure((size_t)n_gapped + 64));
    corr_gapped_lean_launch(c, G, c->gm_gene.as<int>(), c->gm_fail.as<unsigned char>());
    corr_gapped_fast_launch(c, G, c->gm_fail.as<unsigned char>());
  } else if (sw.fast_gapped) {
    corr_gapped_fast_launch(c, G, nullptr);
  }
  AMGCHK(corr_gapped_general(c, S, G, n));
  if (sw.routes) AMGCHK(routes_gapped(c, S, n, G.need_slow, gq));  // (need_slow is a borrowed output buffer: now)
  return AMG_OK;
}
