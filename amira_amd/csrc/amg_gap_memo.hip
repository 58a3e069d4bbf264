// amg_gap_memo.hip — the path memo's search with ONE LANE per question (k_gap_dfs_lanes), for k <= 7.
// (The memo itself — k_gap_queries, the wave-per-question k_gap_dfs and the host's gap_memo — is in
// amg_correct_gapped.hip; this kernel has a unit of its own because kernels compiled next to k_corr_classify change
// that kernel's code, see there.)
//
// After filter_graph nearly every question is a walk along one chain: a path of about k + 2 nodes, each node one
// dependent 16-byte load of its row record.  A wave per question (k_gap_dfs) has one useful lane in every step and at
// most 32 waves x 256 CUs questions in flight: ~100 k questions take a dozen rounds of a chain's latency.  A lane per
// question puts every chain in flight at once.
//   phase A  lane qi answers question qlist[qi] by the scalar search dfs_paths spells (forward list in direction +1,
//            backward in -1, list order, no node twice, accepted at `end` with L <= 2k nodes, retreat when L - 1 > 2k),
//            its stack in LDS, one column per lane, and writes the records [0, len, nodes, dirs] straight into the
//            question's inline stretch of the pool.  A lane whose answer would not fit the stretch, whose search would
//            leave the stack or the step budget, stops and flags its question;
//   phase B  the wave answers its flagged questions one after the other exactly as k_gap_dfs does (dfs_paths_wave
//            into LDS, then the spill behind the inline stretches): an answer beyond GM_INLINE ints takes the code it
//            always took.
#include "amg_gap_search.h"

#define GDL_THREADS 256
#define GDL_DEPTH 16     // stack levels: a search enters at most 2k + 2 nodes deep (the last one only to retreat)
#define GDL_STEPS 4096   // loop iterations of one lane's search (a chain takes ~3 per node); beyond: the wave's turn
#define GDL_DIR_BIT 0x80000000u  // a level's node word: the node (< 2^31) and, in the top bit, direction +1

__global__ __launch_bounds__(GDL_THREADS) void k_gap_dfs_lanes(GView g, const int* __restrict__ qlist, long long n_queries,
                                                                const unsigned long long* __restrict__ qtab,
                                                                unsigned long long* pool_used, unsigned long long pool_cap,
                                                                int* __restrict__ qpool, int4* __restrict__ qres,
                                                                int* __restrict__ qgene) {
  __shared__ unsigned int s_node[GDL_DEPTH][GDL_THREADS];  // node | direction bit
  __shared__ int s_cur[GDL_DEPTH][GDL_THREADS];            // next entry of the level's row (index into lent)
  __shared__ int s_lim[GDL_DEPTH][GDL_THREADS];            // one past the row's last entry
  __shared__ int s_pool[GDL_THREADS / 64][GF_POOL];        // phase B: the searching wave's staging
  __shared__ int s_used[GDL_THREADS / 64];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const long long qi = (long long)blockIdx.x * GDL_THREADS + t;
  if (qi - lane >= n_queries) return;  // (wave-uniform: no lane of this wave has a question)
  const bool have = qi < n_queries;
  const int distance = 2 * g.k;
  int slot = 0, s = 0, sdir = 1, e = 0;
  if (have) {
    slot = qlist[qi];
    const unsigned long long key = qtab[slot];
    s = (int)((key >> 32) & 0x7fffffffull);
    e = (int)((key >> 1) & 0x7fffffffull);
    sdir = (key & 1ull) ? 1 : -1;
  }
  // ---- phase A
  const long long off = qi * GM_INLINE;
  // (the host sizes the pool for every inline stretch; a lane whose stretch were not there leaves it to phase B's check)
  bool flagged = have && (unsigned long long)(off + GM_INLINE) > pool_cap;
  int used = 0, n_paths = 0;
  if (have && !flagged) {
    int depth = 0, cur = 0, lim = 0;
    int2 first_ent = make_int2(-1, 0);  // the row record's embedded first entry, while the row is fresh (as wave_dfs)
    bool entering = true;
    s_node[0][t] = (unsigned int)s | (sdir == 1 ? GDL_DIR_BIT : 0u);
    int step = 0;
    for (; step < GDL_STEPS && depth >= 0; ++step) {
      if (entering) {
        entering = false;
        const unsigned int nw = s_node[depth][t];
        const int node = (int)(nw & ~GDL_DIR_BIT);
        const int L = depth + 1;
        if (node == e && L <= distance) {
          if (used + 2 + 2 * L > GM_INLINE) {
            flagged = true;
            break;
          }
          // the path is levels 0 .. L - 1 of the stack.  With it, for the FIRST path, the last gene of every node taken
          // in the path's direction: what k_corr_gapped_lean writes out for a question with one answer (a second path
          // leaves those words unread, as k_gap_dfs leaves them unwritten).  Unrolled: the gathers leave together
          int* o = qpool + off + used;
          unsigned int pw[GDL_DEPTH];
          int gene[GDL_DEPTH];
#pragma unroll
          for (int j = 0; j < GDL_DEPTH; ++j) {
            pw[j] = j < L ? s_node[j][t] : 0u;
            gene[j] = 0;
            if (j < L && n_paths == 0)
              gene[j] = oriented_tok(g, (int)(pw[j] & ~GDL_DIR_BIT), (pw[j] & GDL_DIR_BIT) ? 1 : -1, g.k - 1);
          }
          o[0] = 0;
          o[1] = L;
#pragma unroll
          for (int j = 0; j < GDL_DEPTH; ++j)
            if (j < L) {
              o[2 + j] = (int)(pw[j] & ~GDL_DIR_BIT);
              o[2 + L + j] = (pw[j] & GDL_DIR_BIT) ? 1 : -1;
              if (n_paths == 0) qgene[off + 2 + j] = gene[j];
            }
          used += 2 + 2 * L;
          ++n_paths;
        } else if (L - 1 <= distance) {
          const int4 rw = g.lrows[2ll * node + ((nw & GDL_DIR_BIT) ? 0 : 1)];
          cur = rw.x;
          lim = rw.x + rw.y;
          first_ent = make_int2(rw.z, rw.w);
          continue;
        }
        // accepted or too long: back to the level before
        --depth;
        if (depth >= 0) {
          cur = s_cur[depth][t];
          lim = s_lim[depth][t];
        }
        first_ent.x = -1;
      } else if (cur < lim) {
        int2 ent = first_ent;
        if (first_ent.x < 0) ent = g.lent[cur];
        first_ent.x = -1;
        ++cur;
        bool seen = false;  // no node twice on a path (:2327)
#pragma unroll
        for (int j = 0; j < GDL_DEPTH; ++j) seen = seen || (j <= depth && (int)(s_node[j][t] & ~GDL_DIR_BIT) == ent.x);
        if (seen) continue;
        if (depth + 1 >= GDL_DEPTH) {  // never with 2k + 2 <= GDL_DEPTH (the host's rule); the wave has no such limit
          flagged = true;
          break;
        }
        s_cur[depth][t] = cur;
        s_lim[depth][t] = lim;
        ++depth;
        s_node[depth][t] = (unsigned int)ent.x | (ent.y == 1 ? GDL_DIR_BIT : 0u);
        entering = true;
      } else {
        --depth;
        if (depth >= 0) {
          cur = s_cur[depth][t];
          lim = s_lim[depth][t];
        }
        first_ent.x = -1;  // back in an older row: its first entry was consumed long ago
      }
    }
    if (depth >= 0) flagged = true;  // out of steps (or stopped above)
    if (!flagged) qres[slot] = make_int4((int)off, used, n_paths, 0);
  }
  // ---- phase B: the wave's turn, k_gap_dfs's body for each flagged question
  unsigned long long todo = __ballot(flagged);
  for (int turn = 0; turn < 64 && todo; ++turn) {
    const int b = __ffsll((long long)todo) - 1;
    todo &= todo - 1ull;
    const int bs = __builtin_amdgcn_readlane(s, b), be = __builtin_amdgcn_readlane(e, b);
    const int bdir = __builtin_amdgcn_readlane(sdir, b), bslot = __builtin_amdgcn_readlane(slot, b);
    const long long bqi = qi - lane + b;
    if (lane == 0) s_used[w] = 0;
    wave_sync();
    const int np = dfs_paths_wave(g, bs, bdir, be, distance, 0, s_pool[w], &s_used[w], lane);
    wave_sync();
    const int bused = s_used[w];
    int4 res = make_int4(0, -1, 0, 0);
    if (np >= 0) {
      unsigned long long boff = (unsigned long long)bqi * GM_INLINE;
      if (bused > GM_INLINE) {
        if (lane == 0) boff = (unsigned long long)n_queries * GM_INLINE + atomicAdd(pool_used, (unsigned long long)bused);
        boff = (unsigned long long)bcast_i64((long long)boff, 0);
      }
      if (boff + (unsigned long long)bused <= pool_cap) {
        for (int i = lane; i < bused; i += 64) qpool[boff + i] = s_pool[w][i];
        res = make_int4((int)boff, bused, np, 0);
        if (np == 1 && bused <= GM_INLINE) {
          const int len = s_pool[w][1];
          if (lane < len) qgene[boff + 2 + lane] = oriented_tok(g, s_pool[w][2 + lane], s_pool[w][2 + len + lane], g.k - 1);
        }
      }
    }
    if (lane == 0) qres[bslot] = res;
    wave_sync();  // the next question reuses the staging
  }
}

bool gap_dfs_lanes_fits(int k) { return 2 * k + 2 <= GDL_DEPTH; }

void gap_dfs_lanes_launch(amg_ctx* c, const int* qlist, long long n_queries, const unsigned long long* qtab,
                          unsigned long long* pool_used, unsigned long long pool_cap, int* qpool, int4* qres,
                          int* qgene) {
  hipLaunchKernelGGL(k_gap_dfs_lanes, dim3(nblk(n_queries, GDL_THREADS)), dim3(GDL_THREADS), 0, c->stream,
                     make_view(c), qlist, n_queries, qtab, pool_used, pool_cap, qpool, qres, qgene);
}
