// amg_gap_search.h — what the units of the re-threading's path search share: the question key of the path memo, the
// visitor that writes the paths of one None run on the wave-cooperative search (amg_wave_dfs.h), and the gene a node
// spells in a direction, and the rule that ranks a read's candidates.  Users: amg_gap_memo.hip (k_gap_queries,
// k_gap_dfs, k_gap_dfs_lanes), amg_gap_general.hip (k_corr_gapped) and amg_gap_fast.hip (k_corr_gapped_fast).
#pragma once
#include "amg_correct.h"
#include "amg_wave_dfs.h"

// last gene of node n taken in direction d (get_gene_mer_genes / get_reverse_gene_mer_genes)
__device__ __forceinline__ int oriented_tok(const GView& g, int n, int d, int j) {
  const int* nt = g.n_tok + (long long)n * g.k;
  return d == 1 ? nt[j] : g.flip - nt[g.k - 1 - j];
}

// The paths of one None run, found by the whole wave (wave_dfs, amg_wave_dfs.h): a path is accepted when it reaches
// `e` with <= distance nodes and written to the LDS pool by lanes 0..len-1 at once, as a [run, len, nodes, dirs] record.
struct GapVisit {
  int e, distance, run, lane;
  int *pool, *used;
  int n_paths;
  bool overflow;
  __device__ __forceinline__ int enter(int, int L, int cur_node, int, int my_node, int my_dir) {
    if (cur_node == e && L <= distance) {
      const int off = *used;
      if (off + 2 + 2 * L <= GF_POOL) {
        if (lane == 0) {
          pool[off] = run;
          pool[off + 1] = L;
        }
        if (lane < L) {
          pool[off + 2 + lane] = my_node;
          pool[off + 2 + L + lane] = my_dir;
        }
      } else {
        overflow = true;
      }
      wave_sync();
      if (lane == 0) *used = off + 2 + 2 * L;
      wave_sync();
      ++n_paths;
      return WD_RETREAT;
    }
    return L - 1 > distance ? WD_RETREAT : WD_EXPAND;
  }
};

// returns the number of paths, -1 on pool overflow
__device__ __forceinline__ int dfs_paths_wave(const GView& g, int s, int sdir, int e, int distance, int run, int* pool,
                                              int* used, int lane) {
  GapVisit v{e, distance, run, lane, pool, used, 0, false};
  wave_dfs(g, s, sdir, lane, v);
  return v.overflow ? -1 : v.n_paths;
}

// a question of the path memo: (start node, start direction, end node) in one non-zero word
__device__ __forceinline__ unsigned long long gap_query_key(int s, int sdir, int e) {
  return (1ull << 63) | ((unsigned long long)(unsigned int)s << 32) | ((unsigned long long)(unsigned int)e << 1) |
         (sdir == 1 ? 1ull : 0ull);
}

// the rule that ranks candidates: strictly more shared genes, or equal and strictly higher mean coverage (:1301-1308;
// csum / n against best_sum / best_len by exact cross-multiplication = the order of statistics.mean)
__device__ __forceinline__ bool cand_better(int shared, unsigned long long csum, int n, int best_shared,
                                            unsigned long long best_sum, unsigned long long best_len) {
  return shared > best_shared || (shared == best_shared && csum * best_len > best_sum * (unsigned long long)n);
}
