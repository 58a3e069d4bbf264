// amg_correct_gapped.hip — re-threading of the reads with None runs (stage correct_gapped of amg_correct_reads;
// reference construct_graph.py:1166-1203, 1297-1310, 1331-1386, 2292-2342): the bounded path search, the path memo
// and the three gapped kernels, with the host function that runs them.  (Pipeline: amg_correct.hip.)
//   k_corr_classify                      (amg_correct.hip's classify step: see below why it is compiled here)
//   dfs_paths, k_corr_gapped             the general kernel: a thread per read, its search stack in private arrays
//   k_gap_queries, k_gap_dfs             the path memo: every distinct question of the None runs answered once (a wave
//                                        per question; a lane per question, k_gap_dfs_lanes, is amg_gap_memo.hip's)
//   k_corr_gapped_lean                   sixteen lanes per read: the reads whose every question has one answer
//   gf_* steps, gapped_fast_read, k_corr_gapped_fast   a wave per read, staged in LDS (GfLds)
//   gap_memo, corr_gapped                the host side
// (The None runs of a live-window mask: gap_run_ends / gap_run_terminals in amg_correct.h.)
// (dfs_paths_wave — the re-threading's visitor on the wave-cooperative search —, oriented_tok and the memo's question
// key: amg_gap_search.h, shared with amg_gap_memo.hip.)
#include "amg_correct.h"
#include "amg_gap_search.h"

// ---- classification.  The kernel belongs to amg_correct.hip's classify step and is launched from here only because
// of what the compiler does with it: the device library's 64-bit count-leading-zeros helper is optimised differently
// in a unit where k_corr_classify is its only caller (k_gap_queries and k_corr_gapped_lean are the others here), and
// the kernel's code is to stay what it was.
// One wave classifies 64 consecutive reads.  Lane l owns read l: its offsets, fix flag and results are loaded and
// stored coalesced, one read per lane.  What needs the read's windows — which are live — is a 64-bit mask per read:
// the wave loads the windows of one flagged read at a time (lanes = windows, four reads in flight), ballots, and
// hands the mask to the owning lane; everything else is bit arithmetic on that mask.  (A wave per four reads
// stored every result with its own one-lane instruction: ~8 vector-memory instructions per read.)
__global__ __launch_bounds__(256) void k_corr_classify(CorrArgs a) {
  const long long rbase = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * CLS_READS;
  if (rbase >= a.n_reads) return;
  const int lane = threadIdx.x & 63;
  const long long r = rbase + lane;
  const bool have = r < a.n_reads;
  const long long t0 = have ? a.read_off[r] : 0;
  const long long n = have ? (a.read_off[r + 1] - t0) - a.k + 1 : 0;  // windows; L = n + k - 1
  const bool look = have && n > 0 && a.read_fix[r] != 0;
  // live-window masks of the flagged reads with <= 64 windows
  unsigned long long lv = 0;
  unsigned long long todo = __ballot(look && n <= 64);
  while (todo) {
    int who[4];
    long long tj[4];
    int nj[4], v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      who[q] = todo ? __ffsll((long long)todo) - 1 : -1;
      if (todo) todo &= todo - 1ull;
      tj[q] = who[q] >= 0 ? bcast_i64(t0, who[q]) : 0;
      nj[q] = who[q] >= 0 ? __builtin_amdgcn_readlane((int)n, who[q]) : 0;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) v[q] = lane < nj[q] ? a.tok_node[tj[q] + lane] : -1;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const unsigned long long m = __ballot(v[q] >= 0);  // lanes >= n hold -1
      if (lane == who[q]) lv = m;
    }
  }
  long long first = n, last = -1;
  unsigned int runs = 0, live = 0;
  if (look && n <= 64) {
    first = lv ? (long long)__ffsll((long long)lv) - 1 : n;
    last = lv ? 63 - (long long)__clzll((long long)lv) : -1;
    live = (unsigned int)__popcll(lv);
    // a None run ends where the next window is live (windows past `last` are not live)
    const unsigned long long inside =
        lv ? ((last == 63 ? ~0ull : ((1ull << (last + 1)) - 1ull)) & ~((1ull << first) - 1ull)) : 0ull;
    runs = (unsigned int)__popcll(~lv & inside & (lv >> 1));
  }
  // flagged reads longer than one wave: the wave walks each of them
  unsigned long long big = __ballot(look && n > 64);
  while (big) {
    const int w = __ffsll((long long)big) - 1;
    big &= big - 1ull;
    const long long tw = bcast_i64(t0, w), nw = bcast_i64(n, w);
    long long f = nw, l = -1;
    for (long long i = lane; i < nw; i += 64)
      if (a.tok_node[tw + i] >= 0) {
        f = f < i ? f : i;
        l = l > i ? l : i;
      }
    for (int d = 32; d > 0; d >>= 1) {
      const long long f2 = __shfl_xor(f, d, 64), l2 = __shfl_xor(l, d, 64);
      f = f < f2 ? f : f2;
      l = l > l2 ? l : l2;
    }
    unsigned int ru = 0, li = 0;
    if (l >= 0) {
      for (long long i = f + lane; i <= l; i += 64) {
        const bool none = a.tok_node[tw + i] < 0;
        li += none ? 0u : 1u;
        if (none && a.tok_node[tw + i + 1] >= 0) ++ru;
      }
      for (int d = 32; d > 0; d >>= 1) {
        ru += __shfl_xor(ru, d, 64);
        li += __shfl_xor(li, d, 64);
      }
    }
    if (lane == w) {
      first = f;
      last = l;
      runs = ru;
      live = li;
    }
  }
  const long long L = n + a.k - 1;
  unsigned char cls;
  int start = 0, end = -1;
  unsigned int bound = 0;
  unsigned int len_out = 0;  // genes of the corrected read, known here unless it has None runs
  if (n <= 0) {
    cls = RC_SKIP;  // no entry in _readNodes: correct_reads never sees the read (:1128)
  } else if (!look) {
    cls = RC_COPY;
    len_out = (unsigned int)L;
  } else if (last < 0) {
    cls = RC_DROP;  // every node filtered: the read is dropped (:1141,:1150)
  } else {
    start = (int)first;
    end = (int)last;
    if (runs == 0) {
      cls = RC_TRIM;
      len_out = (unsigned int)(end - start + a.k);
    } else {
      cls = RC_GAPPED;
      const unsigned int b1 = live + runs * (unsigned int)(2 * a.k) + (unsigned int)a.k;
      bound = b1 > (unsigned int)L ? b1 : (unsigned int)L;  // may fall back to the original genes
    }
  }
  if (have) {
    a.cls[r] = cls;
    a.cls_final[r] = cls;
    a.r_start[r] = start;
    a.r_end[r] = end;
    a.bound[r] = bound;    // temp space: only re-threaded reads are staged
    a.new_len[r] = len_out;
    a.gflag[r] = cls == RC_GAPPED ? 1u : 0u;  // list of re-threaded reads (scan input)
    a.lmask[r] = (cls == RC_GAPPED && n <= 64) ? lv : 0ull;
  }
  // largest staging bound of a re-threaded read and the number of None runs: one atomic per wave each (the maximum
  // only when it raises a plain — possibly stale, never too large — read of it); lanes past the last read hold zeros
  unsigned int mb = (have && cls == RC_GAPPED) ? bound : 0u;
  unsigned int nr = (have && cls == RC_GAPPED) ? runs : 0u;
  for (int d = 32; d > 0; d >>= 1) {
    const unsigned int o = (unsigned int)__shfl_xor((int)mb, d, 64);
    mb = mb > o ? mb : o;
    nr += (unsigned int)__shfl_xor((int)nr, d, 64);
  }
  if (lane == 0 && (unsigned long long)mb > *a.max_bound) atomicMax(a.max_bound, (unsigned long long)mb);
  // (16 counter words 128 bytes apart: one word takes ~90 atomics per microsecond, a wave per 64 reads asks more)
  if (lane == 0 && nr) atomicAdd(a.n_runs + 16 * (blockIdx.x & 15), (unsigned long long)nr);
}

void corr_classify_launch(amg_ctx* c, const CorrArgs& a) {
  hipLaunchKernelGGL(k_corr_classify, dim3(nblk(a.n_reads, 4 * CLS_READS)), dim3(256), 0, c->stream, a);  // also new_len, flag, max
}

// ---- gapped reads
#define DFS_MAX (2 * AMG_MAX_K + 4)

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

// the rule that ranks candidates: strictly more shared genes, or equal and strictly higher mean coverage (:1301-1308;
// csum / n against best_sum / best_len by exact cross-multiplication = the order of statistics.mean)
__device__ __forceinline__ bool cand_better(int shared, unsigned long long csum, int n, int best_shared,
                                            unsigned long long best_sum, unsigned long long best_len) {
  return shared > best_shared || (shared == best_shared && csum * best_len > best_sum * (unsigned long long)n);
}

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

// ---- fast path of the gapped-read kernel: one wave per read, everything staged in LDS.
// Reads that exceed any of its fixed capacities are flagged (need_slow) and left to the
// general one-thread-per-read kernel above; results are identical by construction (same
// DFS order, same product order, same comparisons).  (Capacities: GF_* in amg_correct.h.)

// ---- path memo.  k_gap_queries: one LANE per re-threaded read walks the read's None runs on its live-window mask
// (k_corr_classify kept it), looks up the three node words of each run and enters the question (start node, start
// direction, end node) into an open-addressing table; the slot index is the question's id, the lane that created
// the slot lists it.  k_gap_dfs answers every listed question once (the wave-cooperative search, dfs_paths_wave; result copied
// to a global pool) for k >= 8 and under AMG_GAP_DFS_WAVE=1; otherwise k_gap_dfs_lanes does (amg_gap_memo.hip, a lane per
// question); k_corr_gapped_fast copies answers instead of searching.  Reads with more than 64 windows or more than
// GF_MAXGAP runs take no part (gq[0] = -1: they search for themselves, as before).
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
  if (lane == 0) s_used = 0;
  wave_sync();
  const int np = dfs_paths_wave(g, s, sdir, e, 2 * g.k, 0, s_pool, &s_used, lane);
  wave_sync();
  const int used = s_used;
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
// Path memo: every distinct (start, direction, end) question of the None runs is answered once.  Returns in *gq the
// per-read question slots, nullptr when there is no memo (switched off, no runs, or offsets beyond an int).
static int gap_memo(amg_ctx* c, const CorrSwitches& sw, const CorrArgs& a, CorrCounts& n, const int** gq) {
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
  if (n_queries > 0 && !sw.gap_dfs_wave && gap_dfs_lanes_fits(c->k))
    gap_dfs_lanes_launch(c, c->gm_list.as<int>(), n_queries, c->gm_tab.as<unsigned long long>(),
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

// Who hands what to whom: k_corr_gapped_lean (sixteen lanes per read) does the reads whose every question has one
// answer and flags the others in gm_fail; k_corr_gapped_fast (a wave per read, LDS staging) does those — or, without
// memo or lean kernel, every read — and flags in need_slow what exceeds its capacities; k_corr_gapped (a thread per
// read, global pool and candidate scratch) does the flagged rest and is the one that may ask for a larger pool.
int corr_gapped(amg_ctx* c, const CorrSwitches& sw, const CorrScratch& S, const CorrArgs& a, CorrCounts& n) {
  hipStream_t st = c->stream;
  const long long R = c->n_reads, n_gapped = n.n_gapped;
  AMGCHK(S.glist->ensure((size_t)(n_gapped + 1) * sizeof(int)));
  AMGCHK(c->gap_rec.ensure((size_t)(n_gapped + 1) * sizeof(GapRec)));
  hipLaunchKernelGGL(k_scatter_gapped, dim3(nblk(R, 256)), dim3(256), 0, st, S.flag, S.new_idx, R,
                     S.glist->as<int>(), a.read_off, S.r_start, S.r_end, S.tmp_off, a.lmask, c->gap_rec.as<GapRec>());
  const int* gq = nullptr;
  if (n.total_runs > 0 && sw.gap_memo) AMGCHK(gap_memo(c, sw, a, n, &gq));
  const unsigned int threads_total = 64u * 2048u;
  unsigned int cand_stride = (unsigned int)(2 * n.max_bound + (n.max_bound + 3) / 4 + c->k + 16);
  AMGCHK(S.cand->ensure((size_t)threads_total * cand_stride * sizeof(int)));
  // the general kernel only sees what the fast kernel hands over: start small, grow on demand
  unsigned long long pool_cap = 1ull << 22;
  if (sw.gap_pool) {  // test hook: a first pool that the reads of a small input overflow (never a larger one)
    const unsigned long long lo = strtoull(sw.gap_pool, nullptr, 10);
    pool_cap = lo < pool_cap ? lo : pool_cap;
  }
  AMGCHK(S.need_slow->ensure((size_t)n_gapped + 64));
  unsigned char* need_slow = S.need_slow->as<unsigned char>();
  for (int attempt = 0;; ++attempt) {
    AMGCHK(S.pool->ensure((size_t)pool_cap * sizeof(int)));
    unsigned long long* used = c->status.as<unsigned long long>() + ST_COMPACT_A;
    ClearList gcl;
    gcl.add(c->status.p, ST_WORDS * sizeof(unsigned long long));
    GapArgs G;
    G.a = a;
    G.g = make_view(c);
    G.rec = c->gap_rec.as<GapRec>();
    G.gapped_reads = S.glist->as<int>();
    G.n_gapped = n_gapped;
    G.pool = S.pool->as<int>();
    G.pool_cap = pool_cap;
    G.pool_used = used;
    G.status = c->status.as<unsigned long long>();
    G.cand = S.cand->as<int>();
    G.cand_stride = cand_stride;
    G.final_cls = S.final_cls;
    G.need_slow = need_slow;
    G.gq = gq;
    G.qres = c->gm_res.as<int4>();
    G.qpool = c->gm_pool.as<int>();
    if (attempt == 0) {
      gcl.add(need_slow, ((size_t)n_gapped + 4) & ~(size_t)3, sw.fast_gapped ? 0u : 0x01010101u);  // (the buffer has 64 spare bytes)
      AMGCHK(clear_many(c, gcl));
      if (sw.fast_gapped && gq && sw.lean_gapped) {
        // (no count of the flagged reads comes back to the host; AMG_CORR_ROUTES tallies them for tests)
        n.lean_ran = true;
        AMGCHK(c->gm_fail.ensure((size_t)n_gapped + 64));
        hipLaunchKernelGGL(k_corr_gapped_lean, dim3(nblk(n_gapped, GL_THREADS / GL_GROUP)), dim3(GL_THREADS), 0, st, G,
                           c->gm_gene.as<int>(), c->gm_fail.as<unsigned char>());
        hipLaunchKernelGGL(k_corr_gapped_fast, dim3(nblk(n_gapped, LEAN_CHUNK)), dim3(64 * GF_WPB), 0, st, G,
                           c->gm_fail.as<unsigned char>());
      } else if (sw.fast_gapped) {
        hipLaunchKernelGGL(k_corr_gapped_fast, dim3((unsigned int)n_gapped), dim3(64 * GF_WPB), 0, st, G,
                           (const unsigned char*)nullptr);
      }
    } else {
      AMGCHK(clear_many(c, gcl));  // (the status words alone)
    }
    unsigned int blocks = (unsigned int)((n_gapped + 63) / 64);
    if (blocks > 2048u) blocks = 2048u;
    hipLaunchKernelGGL(k_corr_gapped, dim3(blocks), dim3(64), 0, st, G);
    unsigned long long hs[ST_WORDS];
    AMGCHK(fetch_status(c, hs));
    if (!hs[ST_OVERFLOW]) break;
    if (attempt >= 8) return amg_fail(AMG_E_OVERFLOW, "correct_reads: path pool overflow");
    pool_cap = hs[ST_COMPACT_A] * 2 + (1ull << 20);
    n.pool_retries = attempt + 1;
  }
  if (sw.routes) AMGCHK(routes_gapped(c, S, n, need_slow, gq));  // (need_slow is a borrowed output buffer: now)
  return AMG_OK;
}
