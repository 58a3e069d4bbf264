// amg_gap_memo.hip — the path memo of the re-threading (stage correct_gapped; who hands what to whom:
// amg_correct_gapped.hip): every distinct question of the None runs answered once.
//
// k_gap_queries: one LANE per re-threaded read walks the read's None runs on its live-window mask
// (k_corr_classify kept it), looks up the three node words of each run and enters the question (start node, start
// direction, end node) into an open-addressing table; the slot index is the question's id, the lane that created
// the slot lists it.  k_gap_dfs answers every listed question once (the wave-cooperative search, dfs_paths_wave; result copied
// to a global pool) for k >= 8 and under AMG_GAP_DFS_WAVE=1; otherwise k_gap_dfs_lanes does (a lane per
// question); k_corr_gapped_fast copies answers instead of searching.  Reads with more than 64 windows or more than
// GF_MAXGAP runs take no part (gq[0] = -1: they search for themselves, as before).
//
// k_gap_dfs_lanes, ONE LANE per question, for k <= 7.
// After filter_graph nearly every question is a walk along one chain: a path of about k + 2 nodes, each node one
// dependent 16-byte load of its row record.  A wave per question (k_gap_dfs) has one useful lane in every step and at
// most 32 waves x 256 CUs questions in flight: ~100 k questions take a dozen rounds of a chain's latency.  A lane per
// question puts every chain in flight at once.
//   phase A  lane qi answers question qlist[qi] by the scalar search dfs_paths spells (amg_gap_general.hip: forward
//            list in direction +1, backward in -1, list order, no node twice, accepted at `end` with L <= 2k nodes,
//            retreat when L - 1 > 2k), its stack in LDS, one column per lane, and writes the records
//            [0, len, nodes, dirs] straight into the question's inline stretch of the pool.  A lane whose answer would
//            not fit the stretch, whose search would leave the stack or the step budget, stops and flags its question;
//   phase B  the wave answers its flagged questions one after the other exactly as k_gap_dfs does (gap_answer_wave:
//            dfs_paths_wave into LDS, then the spill behind the inline stretches): an answer beyond GM_INLINE ints
//            takes the code it always took.
#include "amg_gap_search.h"

__global__ __launch_bounds__(256) void k_gap_queries(const GapRec* __restrict__ rec, long long n_gapped, int k,
                                                      const int* __restrict__ tok_node,
                                                      const signed char* __restrict__ tok_dir,
                                                      unsigned long long* qtab, unsigned int qmask,
                                                      unsigned long long* ctr /*[0] questions listed*/,
                                                      int* __restrict__ qlist, int* __restrict__ gq,
                                                      unsigned long long* status) {
  // the questions this workgroup creates are collected in LDS and listed with ONE atomicAdd (a counter word takes
  // ~90 returning atomics per microsecond; there are ~100 k questions)
  __shared__ int s_list[256 * GF_MAXGAP];
  __shared__ unsigned int s_n;
  __shared__ unsigned long long s_base;
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  const long long gi = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gi < n_gapped) {
    const GapRec q = rec[gi];
    int* my = gq + gi * GF_MAXGAP;
    const int nwin = q.L0 - k + 1;
    const unsigned long long lv = q.mask;
    unsigned long long ends = gap_run_ends(lv, q.start, q.end);
    if (nwin > 64 || lv == 0ull || __popcll(ends) > GF_MAXGAP) {
      my[0] = -1;
    } else {
      int j = 0;
      while (ends) {
        int ps, pe;
        gap_run_terminals(lv, __ffsll((long long)ends) - 1, ps, pe);
        ends &= ends - 1ull;
        const unsigned long long key = gap_query_key(tok_node[q.t0 + ps], (int)tok_dir[q.t0 + ps], tok_node[q.t0 + pe]);
        unsigned int idx = (unsigned int)mix64(key) & qmask;
        int slot = -1;
        for (unsigned int probes = 0; probes <= qmask; ++probes) {
          unsigned long long cur = qtab[idx];  // plain: a stale view can only show "empty", which the CAS settles
          if (cur == 0ull) {
            cur = atomicCAS(qtab + idx, 0ull, key);
            if (cur == 0ull) {
              s_list[atomicAdd(&s_n, 1u)] = (int)idx;
              cur = key;
            }
          }
          if (cur == key) {
            slot = (int)idx;
            break;
          }
          idx = (idx + 1) & qmask;
        }
        if (slot < 0) status[ST_OVERFLOW] = 7;  // the table holds two slots per run: cannot fill up
        my[j++] = slot;
      }
    }
  }
  __syncthreads();
  const unsigned int n = s_n;
  if (n == 0) return;
  if (threadIdx.x == 0) s_base = atomicAdd(ctr, (unsigned long long)n);
  __syncthreads();
  for (unsigned int i = threadIdx.x; i < n; i += 256) qlist[s_base + i] = s_list[i];
}

// One question (s, sdir, e), number qi of the list and slot `slot` of the table, answered by the whole wave: the
// search into the wave's staging s_pool / s_used, then the answer into the pool and its header into qres[slot].
__device__ __forceinline__ void gap_answer_wave(const GView& g, int s, int sdir, int e, int slot, long long qi,
                                                long long n_queries, unsigned long long* pool_used,
                                                unsigned long long pool_cap, int* __restrict__ qpool,
                                                int4* __restrict__ qres, int* __restrict__ qgene, int* s_pool,
                                                int* s_used, int lane) {
  if (lane == 0) *s_used = 0;
  wave_sync();
  const int np = dfs_paths_wave(g, s, sdir, e, 2 * g.k, 0, s_pool, s_used, lane);
  wave_sync();
  const int used = *s_used;
  int4 res = make_int4(0, -1, 0, 0);
  if (np >= 0) {
    // an answer of up to GM_INLINE ints lives in the question's own stretch of the pool (a few paths of ~7 nodes: nearly
    // all of them); longer ones take space behind those stretches, one atomicAdd each
    unsigned long long off = (unsigned long long)qi * GM_INLINE;
    if (used > GM_INLINE) {
      if (lane == 0) off = (unsigned long long)n_queries * GM_INLINE + atomicAdd(pool_used, (unsigned long long)used);
      off = (unsigned long long)bcast_i64((long long)off, 0);
    }
    if (off + (unsigned long long)used <= pool_cap) {
      for (int i = lane; i < used; i += 64) qpool[off + i] = s_pool[i];
      res = make_int4((int)off, used, np, 0);
      // a question with ONE answer (nearly all of them) also keeps the last gene of every node of its path, taken in the
      // path's direction (get_gene_mer_genes / get_reverse_gene_mer_genes :588-598): what k_corr_gapped_lean writes out
      if (np == 1 && used <= GM_INLINE) {
        const int len = s_pool[1];
        if (lane < len) qgene[off + 2 + lane] = oriented_tok(g, s_pool[2 + lane], s_pool[2 + len + lane], g.k - 1);
      }
    }
  }
  if (lane == 0) qres[slot] = res;
}

__global__ __launch_bounds__(64, 8) void k_gap_dfs(GView g, const int* __restrict__ qlist, long long n_queries,
                                                    const unsigned long long* __restrict__ qtab,
                                                    unsigned long long* pool_used, unsigned long long pool_cap,
                                                    int* __restrict__ qpool, int4* __restrict__ qres,
                                                    int* __restrict__ qgene) {
  __shared__ int s_pool[GF_POOL];
  __shared__ int s_used;
  const long long qi = blockIdx.x;
  if (qi >= n_queries) return;
  const int lane = threadIdx.x;
  const int slot = qlist[qi];
  const unsigned long long key = qtab[slot];
  const int s = (int)((key >> 32) & 0x7fffffffull), e = (int)((key >> 1) & 0x7fffffffull);
  const int sdir = (key & 1ull) ? 1 : -1;
  gap_answer_wave(g, s, sdir, e, slot, qi, n_queries, pool_used, pool_cap, qpool, qres, qgene, s_pool, &s_used, lane);
}

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
  // ---- phase B: the wave's turn for each flagged question
  unsigned long long todo = __ballot(flagged);
  for (int turn = 0; turn < 64 && todo; ++turn) {
    const int b = __ffsll((long long)todo) - 1;
    todo &= todo - 1ull;
    const int bs = __builtin_amdgcn_readlane(s, b), be = __builtin_amdgcn_readlane(e, b);
    const int bdir = __builtin_amdgcn_readlane(sdir, b), bslot = __builtin_amdgcn_readlane(slot, b);
    gap_answer_wave(g, bs, bdir, be, bslot, qi - lane + b, n_queries, pool_used, pool_cap, qpool, qres, qgene,
                    s_pool[w], &s_used[w], lane);
    wave_sync();  // the next question reuses the staging
  }
}

// ------------------------------------------------------------------ host side
// Path memo: every distinct (start, direction, end) question of the None runs is answered once.  Returns in *gq the
// per-read question slots, nullptr when there is no memo (offsets beyond an int; switched off or no runs: not called).
int corr_gap_memo(amg_ctx* c, const CorrSwitches& sw, const CorrArgs& a, CorrCounts& n, const int** gq) {
  hipStream_t st = c->stream;
  const long long n_gapped = n.n_gapped, total_runs = n.total_runs;
  *gq = nullptr;
  const uint64_t qslots = pow2_at_least((uint64_t)total_runs * 2 + 16);
  AMGCHK(c->gm_tab.ensure((size_t)qslots * sizeof(unsigned long long)));
  AMGCHK(c->gm_res.ensure((size_t)qslots * sizeof(int4)));
  AMGCHK(c->gm_list.ensure((size_t)(total_runs + 1) * sizeof(int)));
  AMGCHK(c->gm_q.ensure((size_t)(n_gapped + 1) * GF_MAXGAP * sizeof(int)));
  {
    ClearList cl;
    cl.add(c->gm_tab.p, (size_t)qslots * sizeof(unsigned long long));
    cl.add(c->gm_ctr.p, 16 * sizeof(unsigned long long));
    cl.add(c->status.as<unsigned long long>() + ST_OVERFLOW, sizeof(unsigned long long));
    AMGCHK(clear_many(c, cl));
  }
  hipLaunchKernelGGL(k_gap_queries, dim3(nblk(n_gapped, 256)), dim3(256), 0, st, c->gap_rec.as<GapRec>(), n_gapped,
                     c->k, a.tok_node, a.tok_dir, c->gm_tab.as<unsigned long long>(), (unsigned int)(qslots - 1),
                     c->gm_ctr.as<unsigned long long>(), c->gm_list.as<int>(), c->gm_q.as<int>(),
                     c->status.as<unsigned long long>());
  unsigned long long v[2] = {0, 0};
  {
    FetchList l;
    l.add(c->gm_ctr.p);
    l.add(c->status.as<unsigned long long>() + ST_OVERFLOW);
    AMGCHK(fetch(c, l, v));
  }
  if (v[1]) return amg_fail(AMG_E_HIP, "correct_reads: path memo table full");
  const long long n_queries = (long long)v[0];
  // answers average ~20 ints; one that does not find room sends its reads to the general kernel
  unsigned long long qcap = (unsigned long long)n_queries * (GM_INLINE + 32ull) + 4096ull;
  if (sw.memo_spill) {  // test hook: less room behind the inline stretches (never more)
    const unsigned long long lo = (unsigned long long)n_queries * GM_INLINE + strtoull(sw.memo_spill, nullptr, 10);
    qcap = lo < qcap ? lo : qcap;
  }
  if (qcap > 0x7fffffffull) return AMG_OK;  // (pool offsets are ints)
  AMGCHK(c->gm_pool.ensure((size_t)qcap * sizeof(int)));
  AMGCHK(c->gm_gene.ensure((size_t)qcap * sizeof(int)));
  // a lane per question for the k whose search fits its stack, else a wave per question
  const bool lanes = !sw.gap_dfs_wave && 2 * c->k + 2 <= GDL_DEPTH;
  if (n_queries > 0 && lanes)
    hipLaunchKernelGGL(k_gap_dfs_lanes, dim3(nblk(n_queries, GDL_THREADS)), dim3(GDL_THREADS), 0, st, make_view(c),
                       c->gm_list.as<int>(), n_queries, c->gm_tab.as<unsigned long long>(),
                       c->gm_ctr.as<unsigned long long>() + 1, qcap, c->gm_pool.as<int>(), c->gm_res.as<int4>(),
                       c->gm_gene.as<int>());
  else if (n_queries > 0)
    hipLaunchKernelGGL(k_gap_dfs, dim3((unsigned int)n_queries), dim3(64), 0, st, make_view(c), c->gm_list.as<int>(),
                       n_queries, c->gm_tab.as<unsigned long long>(), c->gm_ctr.as<unsigned long long>() + 1, qcap,
                       c->gm_pool.as<int>(), c->gm_res.as<int4>(), c->gm_gene.as<int>());
  *gq = c->gm_q.as<int>();
  n.n_queries = n_queries;
  return AMG_OK;
}
