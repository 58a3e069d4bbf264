// amg_gap_lean.hip — re-threading, the common case (stage correct_gapped; who hands what to whom:
// amg_correct_gapped.hip): k_corr_gapped_lean, sixteen lanes per read, for the reads whose every question the path
// memo (amg_gap_memo.hip) answered with one path.  The others are flagged for k_corr_gapped_fast (amg_gap_fast.hip).
#include "amg_correct.h"

// ---- re-threading, the common case: SIXTEEN LANES per read.
// k_corr_gapped_fast gives a read a whole wave and spends ~900 instructions on it, most of them with a handful of
// useful lanes, and its waves wait two thirds of their time on a chain of five dependent loads (rocprofv3 counters,
// profiles/r5_*): the kernel is bound by instruction issue and by that chain, not by bytes.  Nearly every read asks
// questions the path memo answered with exactly ONE path (after filter_graph the error bubbles are gone: between two
// terminals of a read there is the genome's path and nothing else).  Then nothing has to be chosen — no cartesian
// product, no shared-gene count, no mean coverage — and the corrected read is the original one with, for every None
// run (ps, pe), the genes k + ps .. k + pe - 1 replaced by the last genes of the path's nodes 1 .. len - 1:
//   * a live window w of the read spells the read's own genes w .. w + k - 1, so every gene that comes from a live
//     window is a token of the read itself (no node-token gather);
//   * the path's first node is window ps; its last node is window pe's NODE in whatever direction the path arrives
//     (new_find_paths_between_nodes :2292-2342 accepts any), so its gene comes from the memo like the interior ones —
//     unless the next run starts at pe: then the later replacement overwrites the shared terminal (insert_elements
//     :1166-1203) and the gene is the read's own again.
// A group of 16 lanes takes one read: lane q owns None run q (k_gap_queries entered at most 16 per read), the group's
// prefix sums run over DPP row shifts (a DPP row IS 16 lanes), and the output genes are written 16 at a time.  Four
// reads per wave share every instruction and keep four chains of loads in flight.  A read that does not qualify (no
// memo entry, a question with no or several answers, an answer beyond the inline stretch, a path of one node) is
// flagged for k_corr_gapped_fast: same results by construction, checked against the oracle through the whole sweep at
// full size and by the fuzzers.
#define GL_GROUP 16
#define GL_THREADS 256
__global__ __launch_bounds__(GL_THREADS) void k_corr_gapped_lean(GapArgs A, const int* __restrict__ qgene,
                                                                  unsigned char* __restrict__ left) {
  // per read and run: {first output index of the run's genes, their number, output - token shift behind them, where
  // the path's genes are in qgene}
  __shared__ int4 s_run[GL_THREADS / GL_GROUP][GL_GROUP];
  __shared__ int s_tk[GL_THREADS / GL_GROUP][64 + AMG_MAX_K];  // the read's own genes (a qualifying read has <= 64 windows)
  const CorrArgs& a = A.a;
  const int k = A.g.k;
  const int lane = threadIdx.x & 63, l16 = threadIdx.x & (GL_GROUP - 1), grp = threadIdx.x / GL_GROUP;
  const int sh = lane & ~(GL_GROUP - 1);  // first lane of this group inside its wave
  const long long gi = (long long)blockIdx.x * (GL_THREADS / GL_GROUP) + grp;
  const bool have = gi < A.n_gapped;
  GapRec rec;
  rec.r = 0; rec.L0 = 0; rec.start = 0; rec.end = -1; rec.t0 = 0; rec.dst = 0; rec.mask = 0ull; rec.pad = 0;
  // the chain of dependent loads is what a read costs here: the record and the read's question slots leave together
  // (the slots of runs the read does not have are not initialised and not looked at), the read's genes and the
  // answers' headers follow, the answers' genes last
  int slot = have ? A.gq[gi * GF_MAXGAP + l16] : -1;
  if (have) rec = A.rec[gi];
  const unsigned long long lv = rec.mask;
  const int nwin = rec.L0 - k + 1;
  bool ok = have && nwin <= 64 && lv != 0ull;
  // the read's None runs as k_gap_queries numbered them: run q ends at the q-th set bit of gap_run_ends
  const int first = rec.start, last = rec.end;
  unsigned long long ends = ok ? gap_run_ends(lv, first, last) : 0ull;
  const int n_gaps = __popcll(ends);
  ok = ok && n_gaps >= 1 && n_gaps <= GF_MAXGAP;
  // (k_gap_queries left gq[0] = -1 on a read it did not enter)
  const bool mine = ok && l16 < n_gaps;
  if (!mine) slot = -1;
  int4 res = make_int4(0, -1, 0, 0);
  if (mine && slot >= 0) res = A.qres[slot];
  if (ok) {  // genes first .. last + k - 1 of the read, staged while the answers' headers are on their way
    const int span = last + k - first;
    for (int i = l16; i < span; i += GL_GROUP) s_tk[grp][i] = a.tokens[rec.t0 + first + i];
  }
  int ps = 0, pe = 0;
  if (mine) {
    unsigned long long e = ends;
    for (int j = 0; j < l16; ++j) e &= e - 1ull;
    gap_run_terminals(lv, __ffsll((long long)e) - 1, ps, pe);
  }
  const int len = (mine && res.y >= 4) ? (res.y - 2) >> 1 : 0;  // one record [run, len, nodes, dirs]
  const bool good = !mine || (slot >= 0 && res.z == 1 && res.y >= 6 && res.y <= GM_INLINE && len >= 2);
  // every run of the read has to qualify: the group's 16 bits of the wave's ballot
  const unsigned int bad16 = (unsigned int)((__ballot(!good) >> sh) & 0xffffull);
  // why the read is left (GL_*): the weightiest reason among its runs
  const bool multi = !good && slot >= 0 && res.z != 1;
  const bool toolong = !good && slot >= 0 && res.z == 1 && res.y > GM_INLINE;
  const unsigned int multi16 = (unsigned int)((__ballot(multi) >> sh) & 0xffffull);
  const unsigned int long16 = (unsigned int)((__ballot(toolong) >> sh) & 0xffffull);
  const int why = !ok ? GL_NO_SLOTS : multi16 ? GL_ANSWERS : long16 ? GL_LONG : GL_OTHER;  // (looked at when bad16 != 0)
  ok = ok && bad16 == 0u;
  // does the next run start where this one ends?  (its ps from the neighbouring lane: row_shl:1)
  const int ps_next = __builtin_amdgcn_update_dpp(-1, ps, 0x101, 0xf, 0xf, false);
  const int shared = (mine && l16 + 1 < n_gaps && ps_next == pe) ? 1 : 0;
  const int c = mine ? len - 1 - shared : 0;            // genes the run brings
  const int rep = mine ? pe - ps - shared : 0;          // genes of the read they replace: k + ps .. k + pe - 1 - shared
  const int incl = row_scan_incl(c - rep);
  const int d_before = incl - (c - rep);
  if (mine) s_run[grp][l16] = make_int4(ps + k - first + d_before, c, incl, res.x + 3);  // (path node 1 sits at res.x + 2 + 1)
  const int total_delta = __shfl(incl, sh + (n_gaps > 0 ? n_gaps - 1 : 0), 64);
  __syncthreads();
  const int ng = ok ? (last + k - first) + total_delta : 0;
  if (ok) {
    for (int o = l16; o < ng; o += GL_GROUP) {
      int tok_shift = 0, src = -1;
      for (int q = 0; q < n_gaps; ++q) {
        const int4 rq = s_run[grp][q];
        if (o >= rq.x) {
          src = o < rq.x + rq.y ? rq.w + (o - rq.x) : -1;
          tok_shift = rq.z;
        }
      }
      const int v = src >= 0 ? qgene[src] : s_tk[grp][o - tok_shift];
      a.tmp_tok[rec.dst + o] = v;
    }
    if (l16 == 0) a.new_len[rec.r] = (unsigned int)ng;
  }
  // the reads left to the wave-per-read kernel: a flag per read (a list would need a counter, and one counter word
  // takes ~100 returning atomics per microsecond: 30 k waves with a read to hand over were 0.3 ms of this kernel)
  if (have && l16 == 0) left[gi] = (unsigned char)(ok ? 0 : why);
}

void corr_gapped_lean_launch(amg_ctx* c, const GapArgs& G, const int* qgene, unsigned char* left) {
  hipLaunchKernelGGL(k_corr_gapped_lean, dim3(nblk(G.n_gapped, GL_THREADS / GL_GROUP)), dim3(GL_THREADS), 0, c->stream,
                     G, qgene, left);
}
