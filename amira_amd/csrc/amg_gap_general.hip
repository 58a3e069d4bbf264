// amg_gap_general.hip — re-threading, the general kernel (stage correct_gapped; who hands what to whom:
// amg_correct_gapped.hip): k_corr_gapped, a thread per read, its search stack in private arrays, its paths in a global
// pool and its candidates in global scratch.  It does the reads the wave-per-read kernel flagged in need_slow — what
// exceeds that kernel's LDS capacities — and is the one that may ask for a larger pool.  The host side here is the
// kernel's alone: its room (candidate scratch, the flags, the first pool) and the attempt loop that grows the pool.
#include "amg_correct.h"
#include "amg_gap_search.h"

#define DFS_MAX (2 * AMG_MAX_K + 4)
#define GG_BLOCKS 2048u  // the grid's upper limit: the candidate scratch is sized for 64 threads of as many workgroups

struct PathSink {
  int* buf;        // nullptr => count only
  long long used;  // ints
  int n_paths;
};

// new_find_paths_between_nodes(start, end, distance, direction): simple paths following the
// forward list when the current direction is +1, the backward list when -1, in list order;
// a path is accepted when it reaches `end` with <= distance nodes.  Emits [len, node*len, dir*len].
__device__ void dfs_paths(const GView& g, int s, int sdir, int e, int distance, PathSink* sink) {
  int node[DFS_MAX], dir[DFS_MAX];
  long long cur[DFS_MAX], lim[DFS_MAX];
  int depth = 0;
  node[0] = s;
  dir[0] = sdir;
  bool entering = true;
  while (depth >= 0) {
    if (entering) {
      int L = depth + 1;
      if (node[depth] == e && L <= distance) {
        if (sink->buf) {
          int* o = sink->buf + sink->used;
          o[0] = L;
          for (int j = 0; j < L; ++j) {
            o[1 + j] = node[j];
            o[1 + L + j] = dir[j];
          }
        }
        sink->used += 1 + 2 * L;
        sink->n_paths += 1;
        --depth;
        entering = false;
        continue;
      }
      if (L - 1 > distance) {
        --depth;
        entering = false;
        continue;
      }
      long long row = 2ll * node[depth] + (dir[depth] == 1 ? 0 : 1);
      const int4 rw = g.lrows[row];
      cur[depth] = rw.x;
      lim[depth] = rw.x + rw.y;
      entering = false;
    }
    bool pushed = false;
    while (cur[depth] < lim[depth]) {
      const int2 ent = g.lent[cur[depth]++];
      int t = ent.x;
      bool seen = false;
      for (int j = 0; j <= depth; ++j) seen = seen || (node[j] == t);
      if (seen) continue;
      node[depth + 1] = t;
      dir[depth + 1] = ent.y;
      ++depth;
      entering = true;
      pushed = true;
      break;
    }
    if (!pushed) --depth;
  }
}

struct GapIter {
  long long t0;
  const int* tok_node;
  int start, end, i;
  int ps, pe;
  __device__ bool next() {
    // identify_path_terminals: for i in [start, end] with a None at i: path_start = i-1 if live,
    // pair emitted when i+1 is live
    while (i <= end) {
      int idx = i++;
      if (tok_node[t0 + idx] < 0) {
        if (tok_node[t0 + idx - 1] >= 0) ps = idx - 1;
        if (tok_node[t0 + idx + 1] >= 0) {
          pe = idx + 1;
          return true;
        }
      }
    }
    return false;
  }
};

// build candidate `combo` (mixed radix over the gaps' path choices) into (out_node, out_dir);
// returns its node count.  paths of gap q start at pool[gap_off[q]] as [len, nodes, dirs] records.
__device__ int build_candidate(const GapArgs& A, long long t0, int start, int end, const int* rec,
                               int n_gaps, unsigned long long combo, int* out_node, signed char* out_dir) {
  // rec layout: for each gap q: [ps, pe, n_paths, first_record_offset] (4 ints)
  // product(*lists): the LAST gap varies fastest
  int n = 0;
  int q = 0;
  int i = start;
  int prev_pe = -1;
  // choice for gap q = (combo / prod_{j>q} n_j) % n_q
  while (i <= end) {
    if (q < n_gaps && rec[4 * q] == i) {
      int ps = rec[4 * q], pe = rec[4 * q + 1], np = rec[4 * q + 2];
      unsigned long long div = 1;
      for (int j = q + 1; j < n_gaps; ++j) div *= (unsigned long long)rec[4 * j + 2];
      int pick = (int)((combo / div) % (unsigned long long)np);
      const int* p = A.pool + rec[4 * q + 3];
      for (int s = 0; s < pick; ++s) p += 1 + 2 * p[0];
      int L = p[0];
      if (prev_pe == ps && n > 0) --n;  // shared endpoint: the later replacement overwrites it
      for (int j = 0; j < L; ++j) {
        out_node[n] = p[1 + j];
        out_dir[n] = (signed char)p[1 + L + j];
        ++n;
      }
      prev_pe = pe;
      i = pe;
      ++q;
      if (!(q < n_gaps && rec[4 * q] == pe)) i = pe + 1;
    } else {
      out_node[n] = A.a.tok_node[t0 + i];
      out_dir[n] = A.a.tok_dir[t0 + i];
      ++n;
      ++i;
    }
  }
  return n;
}

__global__ __launch_bounds__(64) void k_corr_gapped(GapArgs A) {
  const CorrArgs& a = A.a;
  const GView& g = A.g;
  const long long gtid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long gstride = (long long)gridDim.x * blockDim.x;
  int* my = A.cand + gtid * (long long)A.cand_stride;
  for (long long gi = gtid; gi < A.n_gapped; gi += gstride) {
    if (!A.need_slow[gi]) continue;
    const long long r = A.gapped_reads[gi];
    const long long t0 = a.read_off[r];
    const int L0 = (int)(a.read_off[r + 1] - t0);
    const int start = a.r_start[r], end = a.r_end[r];
    const long long dst = a.tmp_off[r];
    // ---- pass 1: count paths per None run
    int n_gaps = 0;
    long long need = 0;
    bool dead_end = false;
    {
      GapIter it{t0, a.tok_node, start, end, start, -1, -1};
      while (it.next()) {
        PathSink sink{nullptr, 0, 0};
        dfs_paths(g, a.tok_node[t0 + it.ps], a.tok_dir[t0 + it.ps], a.tok_node[t0 + it.pe], 2 * g.k, &sink);
        if (sink.n_paths == 0) dead_end = true;
        need += sink.used;
        ++n_gaps;
      }
    }
    bool keep_orig = dead_end;  // product over an empty list: possible_paths == [] (:1292-1293)
    int* rec = nullptr;
    if (!keep_orig) {
      // ---- reserve pool space: 4 ints per gap + the path records
      unsigned long long want = (unsigned long long)need + 4ull * n_gaps;
      unsigned long long base = atomicAdd(A.pool_used, want);
      if (base + want > A.pool_cap) {
        A.status[ST_OVERFLOW] = 3;  // host grows the pool and re-runs
        a.new_len[r] = 0;
        continue;
      }
      rec = A.pool + base;
      int* wr = rec + 4 * n_gaps;
      GapIter it{t0, a.tok_node, start, end, start, -1, -1};
      int q = 0;
      while (it.next()) {
        PathSink sink{wr, 0, 0};
        dfs_paths(g, a.tok_node[t0 + it.ps], a.tok_dir[t0 + it.ps], a.tok_node[t0 + it.pe], 2 * g.k, &sink);
        rec[4 * q] = it.ps;
        rec[4 * q + 1] = it.pe;
        rec[4 * q + 2] = sink.n_paths;
        rec[4 * q + 3] = (int)(wr - A.pool);
        wr += sink.used;
        ++q;
      }
    }
    if (keep_orig) {  // the pack step copies the original genes and positions
      a.new_len[r] = (unsigned int)L0;
      A.final_cls[r] = RC_KEEP_ORIG;
      continue;
    }
    // ---- enumerate the cartesian product in itertools.product order
    unsigned long long n_combo = 1;
    for (int q = 0; q < n_gaps; ++q) {
      n_combo *= (unsigned long long)rec[4 * q + 2];
      if (n_combo > (1ull << 40)) n_combo = 1ull << 40;  // unreachable in practice; bounds the loop
    }
    const int cap_nodes = (int)a.bound[r];
    int* c_node = my;                                         // [cap_nodes]
    signed char* c_dir = reinterpret_cast<signed char*>(my + cap_nodes);  // [cap_nodes]
    int* c_gene = my + cap_nodes + (cap_nodes + 3) / 4;       // [cap_nodes + k]
    int best_shared = 0;
    unsigned long long best_sum = 0, best_len = 1;  // mean coverage 0
    int best_n = -1;
    for (unsigned long long combo = 0; combo < n_combo; ++combo) {
      int n = build_candidate(A, t0, start, end, rec, n_gaps, combo, c_node, c_dir);
      // genes (get_annotation_for_read): k-1 genes of the first node + last gene of every node
      int ng = 0;
      for (int j = 0; j < g.k - 1; ++j) c_gene[ng++] = oriented_tok(g, c_node[0], c_dir[0], j);
      unsigned long long csum = 0;
      for (int j = 0; j < n; ++j) {
        c_gene[ng++] = oriented_tok(g, c_node[j], c_dir[j], g.k - 1);
        csum += g.n_cov[c_node[j]];
      }
      // len(set(genes) & set(original genes))
      int shared = 0;
      for (int j = 0; j < ng; ++j) {
        int tk = c_gene[j];
        bool dup = false;
        for (int q = 0; q < j && !dup; ++q) dup = (c_gene[q] == tk);
        if (dup) continue;
        bool hit = false;
        for (int q = 0; q < L0 && !hit; ++q) hit = (a.tokens[t0 + q] == tk);
        shared += hit ? 1 : 0;
      }
      if (cand_better(shared, csum, n, best_shared, best_sum, best_len)) {
        best_shared = shared;
        best_sum = csum;
        best_len = (unsigned long long)n;
        best_n = ng;
        for (int j = 0; j < ng; ++j) a.tmp_tok[dst + j] = c_gene[j];
      }
    }
    a.new_len[r] = (unsigned int)best_n;
  }
}

// ------------------------------------------------------------------ host side
int corr_general_room(amg_ctx* c, const CorrSwitches& sw, const CorrScratch& S, const CorrCounts& n, GeneralRoom& room) {
  const unsigned int threads_total = 64u * GG_BLOCKS;
  room.cand_stride = (unsigned int)(2 * n.max_bound + (n.max_bound + 3) / 4 + c->k + 16);
  AMGCHK(S.cand->ensure((size_t)threads_total * room.cand_stride * sizeof(int)));
  // the general kernel only sees what the fast kernel hands over: start small, grow on demand
  room.pool_cap = 1ull << 22;
  if (sw.gap_pool) {  // test hook: a first pool that the reads of a small input overflow (never a larger one)
    const unsigned long long lo = strtoull(sw.gap_pool, nullptr, 10);
    room.pool_cap = lo < room.pool_cap ? lo : room.pool_cap;
  }
  AMGCHK(S.need_slow->ensure((size_t)n.n_gapped + 64));
  AMGCHK(S.pool->ensure((size_t)room.pool_cap * sizeof(int)));
  return AMG_OK;
}

int corr_gapped_general(amg_ctx* c, const CorrScratch& S, GapArgs& G, CorrCounts& n) {
  for (int attempt = 0;; ++attempt) {
    if (attempt > 0) {  // a larger pool, the status words clear again
      AMGCHK(S.pool->ensure((size_t)G.pool_cap * sizeof(int)));
      G.pool = S.pool->as<int>();
      ClearList gcl;
      gcl.add(c->status.p, ST_WORDS * sizeof(unsigned long long));
      AMGCHK(clear_many(c, gcl));
    }
    unsigned int blocks = (unsigned int)((G.n_gapped + 63) / 64);
    if (blocks > GG_BLOCKS) blocks = GG_BLOCKS;
    hipLaunchKernelGGL(k_corr_gapped, dim3(blocks), dim3(64), 0, c->stream, G);
    unsigned long long hs[ST_WORDS];
    AMGCHK(fetch_status(c, hs));
    if (!hs[ST_OVERFLOW]) break;
    if (attempt >= 8) return amg_fail(AMG_E_OVERFLOW, "correct_reads: path pool overflow");
    G.pool_cap = hs[ST_COMPACT_A] * 2 + (1ull << 20);
    n.pool_retries = attempt + 1;
  }
  return AMG_OK;
}
