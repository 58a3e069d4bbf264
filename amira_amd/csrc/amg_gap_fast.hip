// amg_gap_fast.hip — re-threading, a wave per read (stage correct_gapped; who hands what to whom:
// amg_correct_gapped.hip): k_corr_gapped_fast with its staging (GfLds) and the gf_* steps of gapped_fast_read.
#include "amg_correct.h"
#include "amg_gap_search.h"

// ---- fast path of the gapped-read kernel: one wave per read, everything staged in LDS.
// Reads that exceed any of its fixed capacities are flagged (need_slow) and left to the
// general one-thread-per-read kernel (amg_gap_general.hip); results are identical by construction (same
// DFS order, same product order, same comparisons).  (Capacities: GF_* in amg_correct.h.)

// GF_WPB reads (waves) per workgroup.  The LDS of a workgroup is held until its LAST wave is done
// and reads differ a lot in work (runs, paths): with four waves per workgroup the kernel ran at
// half its occupancy limit waiting for stragglers (2.05 ms; 1.83 ms with two, 1.80 ms with one).
#define GF_WPB 1
struct GfLds {  // one read's staging
  int node[GF_MAXW];
  signed char dir[GF_MAXW];
  int tok[GF_MAXW + AMG_MAX_K];
  int gap[GF_MAXGAP * 3];  // ps, pe, n_paths
  int pool[GF_POOL];
  int used;
  int cnode[GF_CAND];
  signed char cdir[GF_CAND];
  int gene[GF_CAND + AMG_MAX_K];
  int best[GF_CAND + AMG_MAX_K];
};

// ---- the steps of gapped_fast_read, each done by the whole wave on the read's staging S
// the read's windows (nodes, directions) and genes
__device__ __forceinline__ void gf_stage(const CorrArgs& a, const GapRec& rec, int nwin, int lane, GfLds& S) {
  for (int i = lane; i < nwin; i += 64) {
    S.node[i] = a.tok_node[rec.t0 + i];
    S.dir[i] = a.tok_dir[rec.t0 + i];
  }
  for (int i = lane; i < rec.L0; i += 64) S.tok[i] = a.tokens[rec.t0 + i];
  if (lane == 0) S.used = 0;
  wave_sync();
}

// None runs in [start, end] (identify_path_terminals), in read order: S.gap of the first GF_MAXGAP; returns how many
__device__ __forceinline__ int gf_list_runs(int start, int end, int lane, GfLds& S) {
  int n_gaps = 0;
  for (int c0 = start; c0 <= end; c0 += 64) {
    const int i = c0 + lane;
    const bool is_end = i <= end && S.node[i] < 0 && S.node[i + 1] >= 0;  // i < end whenever node[i] < 0
    const unsigned long long m = __ballot(is_end);
    if (is_end) {
      int q = n_gaps + __popcll(m & ((1ull << lane) - 1ull));
      if (q < GF_MAXGAP) {
        int ps = i - 1;
        while (S.node[ps] < 0) --ps;
        S.gap[3 * q] = ps;
        S.gap[3 * q + 1] = i + 1;
        S.gap[3 * q + 2] = 0;
      }
    }
    n_gaps += __popcll(m);
  }
  return n_gaps;
}

// the runs' paths copied from the memo (k_gap_queries entered the read's questions): lane q looks run q up, then all
// copies are in flight together.  Returns 0, or why the read is handed down.
__device__ __forceinline__ int gf_paths_from_memo(const GapArgs& A, int myslot, int n_gaps, int lane, GfLds& S) {
  int4 res = make_int4(0, 0, 0, 0);
  if (lane < n_gaps) res = A.qres[myslot];
  const int len = res.y > 0 ? res.y : 0;
  int at = len;  // inclusive prefix over the runs (lanes < n_gaps <= 16)
#pragma unroll
  for (int d = 1; d < GF_MAXGAP; d <<= 1) {
    const int o = __shfl_up(at, d, 64);
    if (lane >= d) at += o;
  }
  const int total = __shfl(at, n_gaps - 1, 64);
  at -= len;
  if (__any(res.y < 0)) return GS_MEMO_UNFIT;
  if (total > GF_POOL) return GS_RECORDS;
  for (int q = 0; q < n_gaps; ++q) {
    const int src = __shfl(res.x, q, 64), ln = __shfl(len, q, 64), dst0 = __shfl(at, q, 64);
    for (int i = lane; i < ln; i += 64) S.pool[dst0 + i] = A.qpool[src + i];
  }
  wave_sync();
  if (lane < n_gaps) {
    for (int o = at; o < at + len; o += 2 + 2 * S.pool[o + 1]) S.pool[o] = lane;  // the records' run field
    S.gap[3 * lane + 2] = res.z;
  }
  if (lane == 0) S.used = total;
  wave_sync();
  return 0;
}

// without memo: one wave-cooperative search per run, runs in read order
__device__ __forceinline__ int gf_paths_by_search(const GView& g, int n_gaps, int lane, GfLds& S) {
  for (int q = 0; q < n_gaps; ++q) {
    const int ps = S.gap[3 * q], pe = S.gap[3 * q + 1];
    const int np = dfs_paths_wave(g, S.node[ps], S.dir[ps], S.node[pe], 2 * g.k, q, S.pool, &S.used, lane);
    if (lane == 0) S.gap[3 * q + 2] = np < 0 ? 0 : np;
    if (np < 0) return GS_RECORDS;
  }
  return 0;
}

// candidates = the product of the runs' path counts (counted up to the first product beyond GF_MAXCOMBO)
__device__ __forceinline__ unsigned long long gf_count_combos(const GfLds& S, int n_gaps, bool& dead_end) {
  unsigned long long n_combo = 1;
  dead_end = false;
  for (int q = 0; q < n_gaps; ++q) {
    const int np = S.gap[3 * q + 2];
    dead_end = dead_end || np == 0;
    n_combo *= (unsigned long long)np;
    if (n_combo > GF_MAXCOMBO) break;
  }
  return n_combo;
}

__device__ __forceinline__ void gf_copy_windows(GfLds& S, int n, int i, int cnt, int lane) {
  for (int j = lane; j < cnt; j += 64) {
    S.cnode[n + j] = S.node[i + j];
    S.cdir[n + j] = S.dir[i + j];
  }
}

// candidate `combo` (mixed radix over the runs' paths, the LAST run varies fastest: itertools.product): the live
// windows and the chosen path of every run into S.cnode / S.cdir.  Control flow is wave-uniform (one step per run, not
// per window), the copies are lane-parallel.  Returns the candidate's nodes, -1 beyond GF_CAND.
__device__ __forceinline__ int gf_build_candidate(GfLds& S, int start, int end, int n_gaps, int used,
                                                  unsigned long long combo, int lane) {
  int n = 0, i = start, prev_pe = -1;
  for (int q = 0; q < n_gaps; ++q) {
    const int ps = S.gap[3 * q], pe = S.gap[3 * q + 1], np = S.gap[3 * q + 2];
    // windows [i, ps) are live (a None run is maximal): copied as they are
    const int cnt = ps - i;
    if (cnt > 0) {
      if (n + cnt > GF_CAND) return -1;
      gf_copy_windows(S, n, i, cnt, lane);
      n += cnt;
    }
    unsigned long long div = 1;
    for (int j = q + 1; j < n_gaps; ++j) div *= (unsigned long long)S.gap[3 * j + 2];
    int pick = (int)((combo / div) % (unsigned long long)np);
    int off = 0;
    while (off < used) {  // records of run q appear in DFS order
      if (S.pool[off] == q) {
        if (pick == 0) break;
        --pick;
      }
      off += 2 + 2 * S.pool[off + 1];
    }
    const int L = S.pool[off + 1];
    if (prev_pe == ps && n > 0) --n;  // consecutive runs share their terminal node
    if (n + L > GF_CAND) return -1;
    for (int j = lane; j < L; j += 64) {
      S.cnode[n + j] = S.pool[off + 2 + j];
      S.cdir[n + j] = (signed char)S.pool[off + 2 + L + j];
    }
    n += L;
    prev_pe = pe;
    i = (q + 1 < n_gaps && S.gap[3 * (q + 1)] == pe) ? pe : pe + 1;
  }
  const int cnt = end - i + 1;
  if (cnt > 0) {
    if (n + cnt > GF_CAND) return -1;
    gf_copy_windows(S, n, i, cnt, lane);
    n += cnt;
  }
  return n;
}

// the candidate's ng = n + k - 1 genes (get_annotation_for_read) into S.gene and, when candidates are ranked against
// each other, its coverage sum and len(set(genes) & set(original genes)); lane-parallel
__device__ __forceinline__ void gf_spell_and_score(const GView& g, GfLds& S, int n, int L0, bool rank, int lane,
                                                   int& shared, unsigned long long& csum) {
  const int ng = n + g.k - 1;
  shared = 0;
  csum = 0;
  for (int q = lane; q < ng; q += 64) {
    const int idx = q < g.k - 1 ? 0 : q - (g.k - 1);
    const int j = q < g.k - 1 ? q : g.k - 1;
    S.gene[q] = oriented_tok(g, S.cnode[idx], S.cdir[idx], j);
  }
  if (rank) {
    for (int q = lane; q < n; q += 64) csum += g.n_cov[S.cnode[q]];
    for (int d = 32; d > 0; d >>= 1) csum += __shfl_xor(csum, d, 64);
  }
  wave_sync();
  if (rank) {
    for (int q = lane; q < ng; q += 64) {
      const int tk = S.gene[q];
      bool dup = false;
      for (int w = 0; w < q && !dup; ++w) dup = (S.gene[w] == tk);
      bool hit = false;
      if (!dup)
        for (int w = 0; w < L0 && !hit; ++w) hit = (S.tok[w] == tk);
      shared += hit ? 1 : 0;
    }
    for (int d = 32; d > 0; d >>= 1) shared += __shfl_xor(shared, d, 64);
  }
}

__device__ __forceinline__ void gf_hand_down(const GapArgs& A, long long gi, int lane, int why) {
  if (lane == 0) A.need_slow[gi] = (unsigned char)why;
}

// One read, re-threaded by one wave.  The first limit exceeded hands the read to the general kernel (GS_*).
__device__ __forceinline__ void gapped_fast_read(const GapArgs& A, long long gi, int lane, GfLds& S) {
  const CorrArgs& a = A.a;
  const GView& g = A.g;
  const GapRec rec = A.rec[gi];
  const int nwin = rec.L0 - g.k + 1;
  if (nwin > GF_MAXW) return gf_hand_down(A, gi, lane, GS_WINDOWS);
  // the read's question slots in the path memo ([0] < 0: none; entries past its runs are not initialised)
  const int myslot = (A.gq && lane < GF_MAXGAP) ? A.gq[gi * GF_MAXGAP + lane] : -1;
  gf_stage(a, rec, nwin, lane, S);
  const int n_gaps = gf_list_runs(rec.start, rec.end, lane, S);
  if (n_gaps > GF_MAXGAP) return gf_hand_down(A, gi, lane, GS_RUNS);
  wave_sync();
  const int unfit = __builtin_amdgcn_readfirstlane(myslot) >= 0 ? gf_paths_from_memo(A, myslot, n_gaps, lane, S)
                                                                : gf_paths_by_search(g, n_gaps, lane, S);
  if (unfit) return gf_hand_down(A, gi, lane, unfit);
  wave_sync();
  bool dead_end;
  const unsigned long long n_combo = gf_count_combos(S, n_gaps, dead_end);
  if (dead_end) {
    // possible_paths == []: the original genes (and positions) are kept (:1292-1293); the pack step copies them
    if (lane == 0) {
      a.new_len[rec.r] = (unsigned int)rec.L0;
      A.final_cls[rec.r] = RC_KEEP_ORIG;
    }
    return;
  }
  if (n_combo > GF_MAXCOMBO) return gf_hand_down(A, gi, lane, GS_COMBOS);
  const int used = S.used;
  int best_shared = 0, best_ng = -1;
  unsigned long long best_sum = 0, best_len = 1;
  for (unsigned long long combo = 0; combo < n_combo; ++combo) {
    const int n = gf_build_candidate(S, rec.start, rec.end, n_gaps, used, combo, lane);
    wave_sync();
    if (n < 0) return gf_hand_down(A, gi, lane, GS_CAND);
    int shared;
    unsigned long long csum;
    gf_spell_and_score(g, S, n, rec.L0, n_combo > 1, lane, shared, csum);  // (a lone candidate is not ranked)
    if (n_combo == 1 || cand_better(shared, csum, n, best_shared, best_sum, best_len)) {
      best_shared = shared;
      best_sum = csum;
      best_len = (unsigned long long)n;
      best_ng = n + g.k - 1;
      for (int q = lane; q < best_ng; q += 64) S.best[q] = S.gene[q];
    }
    wave_sync();
  }
  for (int q = lane; q < best_ng; q += 64) a.tmp_tok[rec.dst + q] = S.best[q];
  if (lane == 0) a.new_len[rec.r] = (unsigned int)best_ng;
}

// left == nullptr: every re-threaded read, one per workgroup; else the reads k_corr_gapped_lean flagged: a workgroup
// takes LEAN_CHUNK consecutive reads, lane l looks at read l's flag and the wave works through the flagged ones
__global__ __launch_bounds__(64 * GF_WPB, 8) void k_corr_gapped_fast(GapArgs A, const unsigned char* __restrict__ left) {
  __shared__ GfLds s_lds;
  const int lane = (int)threadIdx.x;
  if (!left) {
    if ((long long)blockIdx.x < A.n_gapped) gapped_fast_read(A, (long long)blockIdx.x, lane, s_lds);
    return;
  }
  const long long base = (long long)blockIdx.x * LEAN_CHUNK;
  const bool mine = lane < LEAN_CHUNK && base + lane < A.n_gapped && left[base + lane] != 0;
  unsigned long long todo = __ballot(mine);
  while (todo) {
    const int b = __ffsll((long long)todo) - 1;
    todo &= todo - 1ull;
    gapped_fast_read(A, base + b, lane, s_lds);
    wave_sync();  // the next read reuses the staging
  }
}

void corr_gapped_fast_launch(amg_ctx* c, const GapArgs& G, const unsigned char* left) {
  const unsigned int blocks = left ? nblk(G.n_gapped, LEAN_CHUNK) : (unsigned int)G.n_gapped;
  hipLaunchKernelGGL(k_corr_gapped_fast, dim3(blocks), dim3(64 * GF_WPB), 0, c->stream, G, left);
}
