// amg_correct.hip — per-read correction on the device (reference construct_graph.py:1123-1396): amg_correct_reads and
// the steps that belong to no other unit (classify, shape, pack).
//
// Pipeline (all device; the host reads a few words back between the steps to size what comes next):
//   classify   k_corr_classify: a wave per 64 reads, a read per lane.  Flagged reads with <= 64 windows are judged on
//              a live-window mask (kept in gm_mask for the steps below), longer ones are walked by the wave.  The mask
//              comes from win_mask, where the read walk of the last removal (k_mask_reads, amg_filter.hip) left one for
//              every read, while those masks are current (WindowMasks, amg_state.h); after anything else has written
//              tok_node or read_fix — a filtered build's own flags — it is balloted from the read's windows.  Class,
//              [start, end] (find_read_boundaries :1153-1164), None runs inside (identify_path_terminals :1375-1386);
//              unmarked reads are copies, reads that only lost their ends are slices ([start : end + k], :1277-1285);
//              reads with None runs are RC_GAPPED and get a staging bound.  One scan pair: staging offsets, gapped list.
//   gapped     (amg_correct_gapped.hip with the amg_gap_* units, after the live adjacency is up to date)
//              k_scatter_gapped lists the gapped reads with a start record each.  Path memo (amg_gap_memo.hip):
//              k_gap_queries enters every None run's (start, direction, end) question into a table, k_gap_dfs_lanes or
//              k_gap_dfs answers each once (new_find_paths_between_nodes :2292-2342, a lane or a wave per question).
//              Then per read the cartesian product of the replacements (insert_elements :1166-1203),
//              best candidate by shared genes, then mean coverage (:1297-1310), genes via get_annotation_for_read
//              (:1331-1373): k_corr_gapped_lean, sixteen lanes per read, for reads whose questions have one answer
//              each -> k_corr_gapped_fast, a wave per read in LDS, for what that left -> k_corr_gapped, a thread per
//              read with a global path pool, for what exceeds the LDS capacities (the pool grows and the step repeats).
//   shape      scan of the kept reads and their lengths: the corrected CSR's offsets.  With positions: k_nw_sizes
//              (per gapped read the carry-over's record, scratch bytes, new positions) and its scan pair.
//   positions  (amg_correct_nw.hip, only with gene positions and gapped reads)  k_nw_place, then needleman_wunsch
//              (:1433-1480), traceback, position carry-over (:1314-1325) and replace_invalid_gene_positions
//              (:1669-1691): k_corr_nw_fast, a wave per read in registers / LDS with shortcuts for alignments that
//              are plain, and k_corr_nw by anti-diagonals for reads beyond its limits.
//   pack       k_corr_pack: a wave per 64 reads compacts genes and per-read records into the corrected CSR; positions
//              stay in their pools (CorrArgs).  The last fetch brings the node bound for the next build.
#include "amg_correct.h"

// live nodes of the graph the reads were corrected against (with PackArgs::dead_kept: an upper bound for the nodes of
// the graph the corrected reads will make)
#define COUNT_PER 16
__global__ __launch_bounds__(256) void k_count_alive(const unsigned char* __restrict__ alive, long long n,
                                                     unsigned long long* out) {
  // a grid sized to the array, COUNT_PER bytes a thread in one 16-byte load: 128 grid-stride workgroups had ten loads of
  // four bytes a thread in a row and waited for each (18 us for 5.4 MB)
  __shared__ unsigned int s_part[4];
  unsigned int c = 0;
  const long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * COUNT_PER;
  if (i + COUNT_PER <= n) {
    const uint4 w = *reinterpret_cast<const uint4*>(alive + i);  // (flags are 0 / 1 bytes)
    c = __popc(w.x & 0x01010101u) + __popc(w.y & 0x01010101u) + __popc(w.z & 0x01010101u) + __popc(w.w & 0x01010101u);
  } else {
    for (long long j = i; j < n; ++j) c += alive[j] ? 1u : 0u;
  }
  for (int d = 32; d > 0; d >>= 1) c += (unsigned int)__shfl_xor((int)c, d, 64);
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0 && (s_part[0] | s_part[1] | s_part[2] | s_part[3]))
    atomicAdd(out, (unsigned long long)s_part[0] + s_part[1] + s_part[2] + s_part[3]);
}

// ---- classification.
// One wave classifies 64 consecutive reads.  Lane l owns read l: its offsets, fix flag and results are loaded and
// stored coalesced, one read per lane.  What needs the read's windows — which are live — is a 64-bit mask per read:
// the wave loads the windows of one flagged read at a time (lanes = windows, four reads in flight), ballots, and
// hands the mask to the owning lane; everything else is bit arithmetic on that mask.  (A wave per four reads
// stored every result with its own one-lane instruction: ~8 vector-memory instructions per read.)
__global__ __launch_bounds__(256) void k_corr_classify(CorrArgs a) {
  const long long rbase = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * CLS_READS;
  const int lane = threadIdx.x & 63;  // (a wave past the last read stays, with no read in any lane: the barrier below)
  const long long r = rbase + lane;
  const bool have = r < a.n_reads;
  const long long t0 = have ? a.read_off[r] : 0;
  const long long n = have ? (a.read_off[r + 1] - t0) - a.k + 1 : 0;  // windows; L = n + k - 1
  const bool look = have && n > 0 && a.read_fix[r] != 0;
  // live-window masks of the flagged reads with <= 64 windows
  unsigned long long lv = 0;
  // ... as the removal's read walk left them (win_mask: current masks of tok_node as it stands, one per lane like the
  // read's other inputs; bits from the window count on are masked off, whatever the tokens behind the last window hold)
  if (a.win_mask && look && n <= 64) lv = a.win_mask[r] & (n == 64 ? ~0ull : (1ull << n) - 1ull);
  // ... or, without current masks (flags of a filtered build), from the windows themselves
  unsigned long long todo = a.win_mask ? 0ull : __ballot(look && n <= 64);
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
  // largest staging bound of a re-threaded read and the number of None runs: one atomic per WORKGROUP each, on 16
  // words 128 bytes apart (one word takes ~90 atomics per microsecond).  With the masks at hand the waves of a million
  // reads get here within a few microseconds of each other: a maximum on ONE word, guarded by a plain read of it that
  // every wave made before any atomic had landed, queued 15 000 atomics there (160 us).  Lanes past the last read hold
  // zeros.
  __shared__ unsigned int s_mb[4], s_nr[4];
  unsigned int mb = (have && cls == RC_GAPPED) ? bound : 0u;
  unsigned int nr = (have && cls == RC_GAPPED) ? runs : 0u;
  for (int d = 32; d > 0; d >>= 1) {
    const unsigned int o = (unsigned int)__shfl_xor((int)mb, d, 64);
    mb = mb > o ? mb : o;
    nr += (unsigned int)__shfl_xor((int)nr, d, 64);
  }
  if (lane == 0) {
    s_mb[threadIdx.x >> 6] = mb;
    s_nr[threadIdx.x >> 6] = nr;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned int m01 = s_mb[0] > s_mb[1] ? s_mb[0] : s_mb[1], m23 = s_mb[2] > s_mb[3] ? s_mb[2] : s_mb[3];
    const unsigned int m = m01 > m23 ? m01 : m23, s = s_nr[0] + s_nr[1] + s_nr[2] + s_nr[3];
    if (m) atomicMax(a.max_bound + 16 * (blockIdx.x & 15), (unsigned long long)m);
    if (s) atomicAdd(a.n_runs + 16 * (blockIdx.x & 15), (unsigned long long)s);
  }
}

// One wave packs 64 consecutive reads.  Lane l owns read l's record: where its genes come from (the read itself,
// a slice of it, or the temp area of a re-threaded read), where they go, how many, and its entry of the corrected
// CSR — all of it loaded and stored coalesced, one read per lane.  Then the 64 lanes copy the reads' genes one read
// at a time (source / destination / length broadcast with v_readlane), four reads in flight.  (A wave per four
// reads issued ~20 small vector-memory instructions per read and was bound by their issue, not by bytes: 0.6 ms for
// 0.56 GB.)  Gene positions stay where they are: the corrected read only records where its positions begin
// (CorrArgs).
__global__ __launch_bounds__(256) void k_corr_pack(PackArgs A) {
  const CorrArgs& a = A.a;
  const int lane = threadIdx.x & 63;
  const long long r = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * PACK_READS + lane;
  if (blockIdx.x == 0 && threadIdx.x == 0) A.o_off[A.out_reads] = A.out_tokens;
  long long dst = 0, src = 0;  // src: token index; bit 62 set = in the temp area
  int n = 0;
  unsigned int dead = 0;  // windows of removed nodes this read brings back (see amg_correct_reads: the next build's table)
  if (r < a.n_reads && a.new_len[r] > 0) {
    dst = A.new_off[r];
    n = (int)a.new_len[r];
    const unsigned char fc = A.final_cls[r];
    if (fc == RC_KEEP_ORIG) {
      const long long nw = a.read_off[r + 1] - a.read_off[r] - a.k + 1;
      dead = nw <= 64 ? (unsigned int)(nw - __popcll(a.lmask[r])) : (unsigned int)nw;
    }
    long long poff = 0;
    if (fc == RC_GAPPED) {  // re-threaded read: genes staged in the temp area, positions written to the pool by
      src = a.tmp_off[r] | (1ll << 62);  // the carry-over kernels
      if (a.have_pos) poff = A.pos_new[r];
    } else {  // untouched read, kept original, or a slice [start : end + k] of it (:1277-1285)
      const long long cut = fc == RC_TRIM ? a.r_start[r] : 0;
      src = a.read_off[r] + cut;
      if (a.have_pos) poff = (a.pos_off ? a.pos_off[r] : a.read_off[r]) + cut;
    }
    const long long q = A.new_idx[r];
    A.o_off[q] = dst;
    A.o_orig[q] = (int)r;
    A.o_changed[q] = (fc == RC_TRIM || fc == RC_GAPPED) ? 1 : 0;
    A.o_src[q] = fc == RC_GAPPED ? -1ll : src;
    if (a.have_pos) A.o_posoff[q] = poff;
    if (a.read_len) A.o_rl[q] = a.read_len[r];
  }
  if (__ballot(dead != 0u) != 0ull) {
    for (int d = 32; d > 0; d >>= 1) dead += (unsigned int)__shfl_xor((int)dead, d, 64);
    if (lane == 0) atomicAdd(A.dead_kept + 16 * (blockIdx.x & 15), (unsigned long long)dead);
  }
  if (__ballot(n > 0) == 0ull) return;
  for (int j0 = 0; j0 < PACK_READS; j0 += 4) {
    const int* sp[4];
    long long d[4];
    int nn[4], vt[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      nn[j] = __builtin_amdgcn_readlane(n, j0 + j);
      const long long sj = bcast_i64(src, j0 + j);
      d[j] = bcast_i64(dst, j0 + j);
      sp[j] = ((sj >> 62) & 1 ? a.tmp_tok : a.tokens) + (sj & ~(1ll << 62));
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (lane < nn[j]) vt[j] = sp[j][lane];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (lane < nn[j]) A.o_tok[d[j] + lane] = vt[j];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      for (int i = 64 + lane; i < nn[j]; i += 64)  // reads longer than one wave
        A.o_tok[d[j] + i] = sp[j][i];
  }
}

// ------------------------------------------------------------------ the host's view of one call
static CorrSwitches read_switches() {
  auto is_one = [](const char* name) {
    const char* v = getenv(name);
    return v && v[0] == '1';
  };
  CorrSwitches sw;
  sw.gap_memo = !is_one("AMG_NO_GAP_MEMO");
  sw.gap_dfs_wave = is_one("AMG_GAP_DFS_WAVE");
  sw.fast_gapped = !is_one("AMG_NO_FAST_GAPPED");
  sw.lean_gapped = !is_one("AMG_NO_LEAN_GAPPED");
  sw.fast_nw = !is_one("AMG_NO_FAST_NW");
  sw.nw_shortcuts = !is_one("AMG_NW_NO_SHORTCUT");
  sw.node_bound = getenv("AMG_TEST_NODE_BOUND");
  sw.routes = is_one("AMG_CORR_ROUTES");  // (the one switch that turns something ON)
  sw.gap_pool = getenv("AMG_TEST_GAP_POOL");
  sw.memo_spill = getenv("AMG_TEST_MEMO_SPILL");
  return sw;
}

// The scratch plan (CorrScratch), in three parts because two sizes are only known after a fetch.  The order of the
// ensure calls is part of the behaviour (one that grows frees and allocates).
static int plan_per_read(amg_ctx* c, CorrScratch& S) {
  const size_t per_read = (size_t)(c->n_reads + 2);
  AMGCHK(c->s0.ensure(per_read * (1 + 1) + 64));                 // cls, final_cls
  AMGCHK(c->s1.ensure(per_read * sizeof(int) * 2 + per_read * sizeof(long long) * 2 + 64));  // r_start, r_end, nw sizes/offsets
  AMGCHK(c->s2.ensure(per_read * sizeof(unsigned int) * 3));     // bound, new_len, keep/flag
  AMGCHK(c->s3.ensure(per_read * sizeof(long long) * 3));        // tmp_off, new_idx, new_off
  AMGCHK(c->gm_mask.ensure(per_read * sizeof(unsigned long long)));
  AMGCHK(c->gm_ctr.ensure((16 + 256 + 256 + 16) * sizeof(unsigned long long)));
  S.per_read = per_read;
  S.cls = c->s0.as<unsigned char>();
  S.final_cls = S.cls + per_read;
  S.r_start = c->s1.as<int>();
  S.r_end = S.r_start + per_read;
  S.nw_size = reinterpret_cast<long long*>(((uintptr_t)(S.r_end + per_read) + 15) & ~(uintptr_t)15);
  S.nw_off = S.nw_size + per_read;
  S.bound = c->s2.as<unsigned int>();
  S.new_len = S.bound + per_read;
  S.flag = S.new_len + per_read;
  S.tmp_off = c->s3.as<long long>();
  S.new_idx = S.tmp_off + per_read;
  S.new_off = S.new_idx + per_read;
  S.n_general = c->status.as<unsigned long long>() + ST_MISC;
  S.n_runs = c->gm_ctr.as<unsigned long long>() + 16;
  S.max_bound = S.n_runs + 8;  // (the other half of each partial sum's 128 bytes)
  S.dead_kept = S.n_runs + 256;
  S.count_alive = c->n_nodes >= (1ll << 20);
  S.glist = &c->c_orig;
  S.cand = &c->c_gstart;
  S.pool = &c->c_gend;
  S.need_slow = &c->c_changed;
  return AMG_OK;
}

static int plan_staging(amg_ctx* c, CorrScratch& S, long long tmp_total) {
  AMGCHK(c->c_tokens_buf.ensure((size_t)(tmp_total + 4) * sizeof(int)));  // (the output, early: the order of allocations is kept)
  AMGCHK(c->s4.ensure((size_t)(tmp_total + 4) * sizeof(int)));
  S.tmp_tok = c->s4.as<int>();
  return AMG_OK;
}

static int plan_positions(amg_ctx* c, CorrScratch& S, long long n_gapped) {
  AMGCHK(c->s5.ensure((size_t)(2 * (n_gapped + 2) + c->n_reads + 2) * sizeof(long long)));
  S.plen = c->s5.as<long long>();
  S.poffs = S.plen + (n_gapped + 2);
  S.pos_new = S.poffs + (n_gapped + 2);
  return AMG_OK;
}

// THE place where the kernels' common arguments are made: everything the context and the plan know at the moment
// of the call.  amg_correct_reads calls it again where a pointer appears or may have moved (tmp_tok, the pools).
static void corr_args(amg_ctx* c, const CorrScratch& S, CorrArgs& a) {
  a.tokens = c->tokens.as<int>();
  a.read_off = c->read_off.as<long long>();
  a.tok_node = c->tok_node.as<int>();
  a.tok_dir = c->tok_dir.as<signed char>();
  a.read_fix = c->read_fix.as<unsigned char>();
  a.win_mask = c->win_masks == WindowMasks::Current ? c->win_mask.as<unsigned long long>() : nullptr;
  fill_pos_args(c, a);
  a.read_len = c->have_read_len ? c->read_len.as<long long>() : nullptr;
  a.n_reads = c->n_reads;
  a.k = c->k;
  a.flip = c->two_v - 1;
  a.have_pos = c->have_pos ? 1 : 0;
  a.gflag = S.flag;
  a.max_bound = S.max_bound;
  a.lmask = c->gm_mask.as<unsigned long long>();
  a.n_runs = S.n_runs;
  a.cls = S.cls;
  a.cls_final = S.final_cls;
  a.r_start = S.r_start;
  a.r_end = S.r_end;
  a.bound = S.bound;
  a.tmp_off = S.tmp_off;
  a.new_len = S.new_len;
  a.tmp_tok = S.tmp_tok;
}

// ------------------------------------------------------------------ the steps of this unit
// classes, boundaries, lengths of the reads that are not re-threaded; where the others are staged and listed
static int corr_classify(amg_ctx* c, const CorrScratch& S, const CorrArgs& a, CorrCounts& n) {
  hipStream_t st = c->stream;
  const long long R = c->n_reads;
  {
    ClearList cl;
    cl.add(S.bound, S.per_read * sizeof(unsigned int) * 3);
    cl.add(S.n_runs, (256 + 256 + 16) * sizeof(unsigned long long));  // (the partial maxima lie between the sums)
    AMGCHK(clear_many(c, cl));
  }
  if (R > 0) hipLaunchKernelGGL(k_corr_classify, dim3(nblk(R, 4 * CLS_READS)), dim3(256), 0, st, a);  // also new_len, flag, max
  // (for the next build's table: how many nodes are alive; rides along, read back with the pack step's words)
  if (S.count_alive)
    hipLaunchKernelGGL(k_count_alive, dim3(nblk(c->n_nodes, 256 * COUNT_PER)), dim3(256), 0, st, c->node_alive.as<unsigned char>(), c->n_nodes,
                       S.dead_kept + 256);
  // where the re-threaded reads' genes are staged, and the list of gapped reads: two scans, one launch
  AMGCHK(prim_exscan_u32_pair(c, S.bound, S.tmp_off, S.flag, S.new_idx, (size_t)R));
  FetchList l;
  l.add(S.tmp_off + R);
  l.add(S.new_idx + R);
  for (int i = 0; i < 16; ++i) l.add(S.n_runs + 16 * i);
  for (int i = 0; i < 16; ++i) l.add(S.max_bound + 16 * i);
  unsigned long long v[2 + 16 + 16];
  AMGCHK(fetch(c, l, v));
  n.tmp_total = (long long)v[0];
  n.n_gapped = (long long)v[1];
  for (int i = 0; i < 16; ++i) n.total_runs += (long long)v[2 + i];
  for (int i = 0; i < 16; ++i) n.max_bound = n.max_bound > v[18 + i] ? n.max_bound : v[18 + i];
  n.carry = n.n_gapped > 0 && c->have_pos;
  return AMG_OK;
}

// shape of the corrected set: which reads stay and where their genes go (both scans in one launch, straight from
// the lengths) — before the position carry-over, which needs its own sizes from the same fetch
static int corr_shape(amg_ctx* c, const CorrSwitches& sw, CorrScratch& S, const CorrArgs& a, CorrCounts& n) {
  const long long R = c->n_reads;
  AMGCHK(prim_exscan_keep_and_len(c, S.new_len, S.new_idx, S.new_off, (size_t)R));
  FetchList shape;
  shape.add(S.new_idx + R);
  shape.add(S.new_off + R);
  if (n.carry) {
    AMGCHK(plan_positions(c, S, n.n_gapped));
    AMGCHK(corr_nw_sizes(c, sw, S, a, n.n_gapped, shape));
  }
  unsigned long long v[5] = {0, 0, 0, 0, 0};
  AMGCHK(fetch(c, shape, v));
  n.out_reads = (long long)v[0];
  n.out_tokens = (long long)v[1];
  n.big_total = (long long)v[2];
  n.pos_total = (long long)v[3];
  n.n_general = v[4];
  return AMG_OK;
}

// the output buffers in their own role (CorrScratch: their scratch names are void from here on)
static int ensure_outputs(amg_ctx* c, const CorrCounts& n) {
  AMGCHK(c->c_tokens_buf.ensure((size_t)(n.out_tokens + 64) * sizeof(int)));
  AMGCHK(c->c_read_off.ensure((size_t)(n.out_reads + 2) * sizeof(long long)));
  AMGCHK(c->c_orig.ensure((size_t)(n.out_reads + 2) * sizeof(int)));
  AMGCHK(c->c_changed.ensure((size_t)(n.out_reads + 2)));
  AMGCHK(c->c_src.ensure((size_t)(n.out_reads + 2) * sizeof(long long)));
  if (c->have_pos) AMGCHK(c->c_pos_off.ensure((size_t)(n.out_reads + 2) * sizeof(long long)));
  if (c->have_read_len) AMGCHK(c->c_read_len.ensure((size_t)(n.out_reads + 2) * sizeof(long long)));
  return AMG_OK;
}

static int corr_pack(amg_ctx* c, const CorrScratch& S, const CorrArgs& a, const CorrCounts& n) {
  PackArgs Pk;
  Pk.a = a;
  Pk.new_idx = S.new_idx;
  Pk.new_off = S.new_off;
  Pk.final_cls = S.final_cls;
  Pk.o_tok = c->c_tokens_buf.as<int>();
  Pk.o_off = c->c_read_off.as<long long>();
  Pk.o_orig = c->c_orig.as<int>();
  Pk.o_changed = c->c_changed.as<unsigned char>();
  Pk.o_src = c->c_src.as<long long>();
  Pk.pos_new = S.pos_new;
  Pk.o_posoff = c->have_pos ? c->c_pos_off.as<long long>() : nullptr;
  Pk.o_rl = c->have_read_len ? c->c_read_len.as<long long>() : nullptr;
  Pk.out_reads = n.out_reads;
  Pk.out_tokens = n.out_tokens;
  Pk.dead_kept = S.dead_kept;
  if (c->n_reads > 0)
    hipLaunchKernelGGL(k_corr_pack, dim3(nblk(c->n_reads, 4 * PACK_READS)), dim3(256), 0, c->stream, Pk);
  else
    HIPCHK(hipMemcpyAsync(c->c_read_off.as<long long>() + n.out_reads, &n.out_tokens, sizeof(long long),
                          hipMemcpyHostToDevice, c->stream));
  return AMG_OK;
}

// The call's last synchronisation; with it an upper bound for the nodes of the graph these reads will make (same k):
// every window of a corrected read is a live node of this graph — untouched reads, slices, re-threaded paths —
// except the dead windows of the reads that fell back to their original genes.
// *only_drops_and_trims: no read was re-threaded or kept its genes around a dead window — reads were dropped or cut to their
// live windows, so the graph they make is this graph's live part (amg_derive.hip) unless an edge died on its own
static int corr_node_bound(amg_ctx* c, const CorrScratch& S, const CorrCounts& n, int64_t* bound_out, bool* only_drops_and_trims) {
  FetchList l;
  for (int i = 0; i < 16; ++i) l.add(S.dead_kept + 16 * i);
  l.add(S.dead_kept + 256);
  unsigned long long v[17];
  AMGCHK(fetch(c, l, v));
  unsigned long long bound = S.count_alive ? v[16] : (unsigned long long)c->n_nodes;
  unsigned long long dead_kept = 0;
  for (int i = 0; i < 16; ++i) dead_kept += v[i];
  *bound_out = (int64_t)(bound + dead_kept);
  *only_drops_and_trims = n.n_gapped == 0 && dead_kept == 0;
  return AMG_OK;
}

// classify -> [live adjacency -> gapped] -> shape -> [positions] -> pack -> bound.  Every step ends in at most one
// fetch (the gapped step: one for the memo, one per pool attempt), and `a` is remade where the plan or the pools
// have changed, so the copy a step takes into its kernels' arguments is the one of the line above it.
extern "C" int amg_correct_reads(amg_ctx* c, int64_t* n_out_reads, int64_t* n_out_tokens) {
  NEED_BUILT(c);
  const CorrSwitches sw = read_switches();
  stages_reset(c);
  ctx_corrected_begun(c);
  CorrScratch S;
  CorrCounts n;
  CorrArgs a;
  AMGCHK(plan_per_read(c, S));
  corr_args(c, S, a);  // (no tmp_tok yet)
  c->have_routes = false;
  if (sw.routes) AMGCHK(routes_begin(c));

  stage_begin(c, "correct_classify");
  AMGCHK(corr_classify(c, S, a, n));
  stage_end(c);
  AMGCHK(plan_staging(c, S, n.tmp_total));
  corr_args(c, S, a);  // + tmp_tok

  if (n.n_gapped > 0) {
    stage_begin(c, "live_adjacency");
    AMGCHK(ensure_live_adj(c));
    stage_end(c);
    stage_begin(c, "correct_gapped");
    AMGCHK(corr_gapped(c, sw, S, a, n));
    stage_end(c);
  }

  stage_begin(c, "correct_pack");  // first interval of that name: the SHAPE of the corrected set
  AMGCHK(corr_shape(c, sw, S, a, n));
  stage_end(c);
  AMGCHK(ensure_outputs(c, n));

  if (n.carry) {
    stage_begin(c, "correct_positions");
    AMGCHK(corr_grow_pos_pools(c, n));
    corr_args(c, S, a);  // the pools of produced positions where they are now
    AMGCHK(corr_positions(c, sw, S, a, n));
    if (sw.routes) AMGCHK(routes_nw(c, S, n));
    stage_end(c);
  }

  stage_begin(c, "correct_pack");  // second interval: the pack itself
  AMGCHK(corr_pack(c, S, a, n));
  int64_t bound = 0;
  bool only_drops_and_trims = false;
  AMGCHK(corr_node_bound(c, S, n, &bound, &only_drops_and_trims));
  stage_end(c);
  if (sw.routes) AMGCHK(routes_end(c, n));
  ctx_corrected_made(c, n.out_reads, n.out_tokens, c->pos1_used + (n.carry ? n.pos_total : 0), only_drops_and_trims, bound,
                     sw.node_bound);
  if (n_out_reads) *n_out_reads = n.out_reads;
  if (n_out_tokens) *n_out_tokens = n.out_tokens;
  return AMG_OK;
}
