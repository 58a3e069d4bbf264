// amg_select.hip — selections of whole reads on the device: amg_select_reads (get_valid_reads_only, reference
// construct_graph.py:1422-1427; remove_junk_reads, :1398-1420).
//
// A selection of whole reads is a corrected set in which nothing changed, so that is what the call leaves: the c_*
// arrays of the ctx as an amg_correct_reads that changed no read would fill them, for the getters and the adopt of
// amg_corrected.hip to work on.
//   classify   k_sel_classify: a wave per 64 reads, a read per lane.  Masked windows (tok_node < 0) of every read with
//              a window: reads of at most 64 windows by ballot (lanes = windows, four reads in flight), longer ones
//              walked by the wave.  Verdict, keep flag and length per read; the masked windows of the reads IN THE SET
//              summed for the next build's node bound, the most windows of a read for the verdict on n_allowed.
//   shape      one scan pair (amg_scan.hip): the set's rows from the keep flags, its offsets from the lengths.  A read
//              in the set stays even without a gene (get_valid_reads_only returns {r: []} for it), so the scan takes
//              the keep flag, not "length > 0" as the correction's pack does.
//   pack       k_sel_pack: a wave per 64 reads, a lane per read for the record, the 64 lanes copy the genes one read at
//              a time, four reads in flight.  Gene positions stay where they are: a read records where they begin.
// The outputs are sized by the current read set (a selection never grows it), so nothing is read back between the
// steps: ONE fetch at the end carries the set's sizes, the bound's counters and the longest read's windows.
// Two things an amg_correct_reads also guards: c_derivable stays false (rejected reads take live coverage away and kept
// ones bring their masked windows back as nodes: the set does not make the live part of the graph at hand), and the
// node bound of the next build counts the masked windows of the reads in the set.
#include "amg_correct.h"
#include "amg_select_args.h"

#define SEL_READS 64  // reads per wave of both kernels

struct SelArgs {
  const int* tokens;
  const long long* read_off;
  const int* tok_node;
  const unsigned char* read_fix;
  const long long* pos_off;   // nullptr: a read's positions begin at its token offset
  const long long* read_len;  // nullptr: no read lengths were set
  const long long* allowed;   // device copy of the caller's table (JUNK)
  long long n_allowed;
  long long n_reads;
  int k, mode, invert, have_pos;
  // per read
  unsigned char* verdict;
  unsigned int* keep;  // 1: the read is in the set (scan input)
  unsigned int* len;   // its genes when it is, else 0 (scan input)
  // counters
  unsigned long long* masked_in;  // masked windows of the reads in the set: 16 partial sums, 16 words apart
  unsigned long long* max_win;    // most windows of a read
};

struct SelPack {
  SelArgs a;
  const long long* new_idx;  // exscan(keep): new_idx[n_reads] = reads of the set
  const long long* new_off;  // exscan(len):  new_off[n_reads] = its genes
  int* o_tok;
  long long* o_off;
  int* o_orig;
  unsigned char* o_changed;
  long long* o_src;
  long long* o_posoff;
  long long* o_rl;
};

// alive nodes, for the node bound (flags are 0 / 1 bytes)
__global__ __launch_bounds__(256) void k_sel_count_alive(const unsigned char* __restrict__ alive, long long n,
                                                         unsigned long long* out) {
  unsigned int c = 0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    c += alive[i] ? 1u : 0u;
  for (int d = 32; d > 0; d >>= 1) c += (unsigned int)__shfl_xor((int)c, d, 64);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(out, (unsigned long long)c);
}

// One wave judges 64 consecutive reads.  Lane l owns read l: offsets, fix flag, verdict, keep flag and length are
// loaded and stored coalesced.  The masked windows of a read of at most 64 windows are a popcount of one ballot (the
// wave loads the windows of one read at a time, four reads in flight); a longer read is walked by the wave.
__global__ __launch_bounds__(256) void k_sel_classify(SelArgs a) {
  const long long rbase = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * SEL_READS;
  if (rbase >= a.n_reads) return;
  const int lane = threadIdx.x & 63;
  const long long r = rbase + lane;
  const bool have = r < a.n_reads;
  const long long t0 = have ? a.read_off[r] : 0;
  const long long L = have ? a.read_off[r + 1] - t0 : 0;
  const long long n = L - a.k + 1 > 0 ? L - a.k + 1 : 0;  // windows
  const bool look = have && n > 0;
  unsigned int m = 0;  // masked windows
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
    for (int q = 0; q < 4; ++q) v[q] = lane < nj[q] ? a.tok_node[tj[q] + lane] : 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const unsigned long long mk = __ballot(v[q] < 0);  // lanes >= n hold 0
      if (lane == who[q]) m = (unsigned int)__popcll(mk);
    }
  }
  unsigned long long big = __ballot(look && n > 64);
  while (big) {
    const int w = __ffsll((long long)big) - 1;
    big &= big - 1ull;
    const long long tw = bcast_i64(t0, w), nw = bcast_i64(n, w);
    unsigned int mm = 0;
    for (long long i = lane; i < nw; i += 64) mm += a.tok_node[tw + i] < 0 ? 1u : 0u;
    for (int d = 32; d > 0; d >>= 1) mm += (unsigned int)__shfl_xor((int)mm, d, 64);
    if (lane == w) m = mm;
  }
  unsigned char verdict = AMG_SEL_UNLISTED;
  if (have && a.mode == AMG_SELECT_VALID) {
    verdict = a.read_fix[r] != 0 ? AMG_SEL_REJECTED : AMG_SEL_KEPT;
  } else if (look) {
    // (a read beyond the table is rejected here and the call refused once the host has seen max_win)
    verdict = (n < a.n_allowed && (long long)m <= a.allowed[n]) ? AMG_SEL_KEPT : AMG_SEL_REJECTED;
  }
  const bool in_set = have && verdict == (a.invert ? AMG_SEL_REJECTED : AMG_SEL_KEPT);
  if (have) {
    a.verdict[r] = verdict;
    a.keep[r] = in_set ? 1u : 0u;
    a.len[r] = in_set ? (unsigned int)L : 0u;
  }
  // one atomic per wave each, the maximum only when it raises a plain — possibly stale, never too large — read of it
  unsigned int ms = in_set ? m : 0u;
  long long mw = n;
  for (int d = 32; d > 0; d >>= 1) {
    ms += (unsigned int)__shfl_xor((int)ms, d, 64);
    const long long o = __shfl_xor(mw, d, 64);
    mw = mw > o ? mw : o;
  }
  if (lane == 0 && ms) atomicAdd(a.masked_in + 16 * (blockIdx.x & 15), (unsigned long long)ms);
  if (lane == 0 && (unsigned long long)mw > *a.max_win) atomicMax(a.max_win, (unsigned long long)mw);
}

// One wave packs 64 consecutive reads.  Lane l owns read l's record of the corrected CSR (a read of the set has one
// even when it has no gene); then the 64 lanes copy the reads' genes one read at a time, four reads in flight, with a
// tail loop for reads of more than 64 genes.
__global__ __launch_bounds__(256) void k_sel_pack(SelPack A) {
  const SelArgs& a = A.a;
  const int lane = threadIdx.x & 63;
  const long long r = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * SEL_READS + lane;
  if (blockIdx.x == 0 && threadIdx.x == 0) A.o_off[A.new_idx[a.n_reads]] = A.new_off[a.n_reads];
  long long dst = 0, src = 0;
  int n = 0;
  if (r < a.n_reads && a.keep[r] != 0u) {
    dst = A.new_off[r];
    n = (int)a.len[r];
    src = a.read_off[r];
    const long long q = A.new_idx[r];
    A.o_off[q] = dst;
    A.o_orig[q] = (int)r;
    A.o_changed[q] = 0;
    A.o_src[q] = src;
    if (a.have_pos) A.o_posoff[q] = a.pos_off ? a.pos_off[r] : src;
    if (a.read_len) A.o_rl[q] = a.read_len[r];
  }
  if (__ballot(n > 0) == 0ull) return;
  for (int j0 = 0; j0 < SEL_READS; j0 += 4) {
    const int* sp[4];
    long long d[4];
    int nn[4], vt[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      nn[j] = __builtin_amdgcn_readlane(n, j0 + j);
      sp[j] = a.tokens + bcast_i64(src, j0 + j);
      d[j] = bcast_i64(dst, j0 + j);
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

extern "C" int amg_select_reads(amg_ctx* c, int32_t mode, int32_t invert, const int64_t* allowed, int64_t n_allowed,
                                uint8_t* verdict, int64_t* n_out_reads, int64_t* n_out_tokens) {
  NEED_BUILT(c);
  char why[192];
  if (sel_check_args(mode, allowed != nullptr, n_allowed, why, sizeof why))
    return amg_fail(AMG_E_ARG, "amg_select_reads: %s", why);
  hipStream_t st = c->stream;
  const long long R = c->n_reads, T = c->n_tokens;
  stages_reset(c);
  ctx_corrected_begun(c);

  // scratch: verdicts; keep flags and lengths; the two scans; the table; the counters [16 x 16 words], alive nodes
  // and the most windows behind them
  const size_t per_read = (size_t)(R + 2);
  AMGCHK(c->s0.ensure(per_read + 64));
  AMGCHK(c->s2.ensure(per_read * sizeof(unsigned int) * 2));
  AMGCHK(c->s3.ensure(per_read * sizeof(long long) * 2));
  AMGCHK(c->s4.ensure((256 + 2) * sizeof(unsigned long long)));
  if (mode == AMG_SELECT_JUNK) AMGCHK(c->s1.ensure((size_t)n_allowed * sizeof(long long)));
  // the set is no larger than the current reads: the outputs in their full size, nothing read back to size them
  AMGCHK(c->c_tokens_buf.ensure((size_t)(T + 64) * sizeof(int)));
  AMGCHK(c->c_read_off.ensure((size_t)(R + 2) * sizeof(long long)));
  AMGCHK(c->c_orig.ensure((size_t)(R + 2) * sizeof(int)));
  AMGCHK(c->c_changed.ensure((size_t)(R + 2)));
  AMGCHK(c->c_src.ensure((size_t)(R + 2) * sizeof(long long)));
  if (c->have_pos) AMGCHK(c->c_pos_off.ensure((size_t)(R + 2) * sizeof(long long)));
  if (c->have_read_len) AMGCHK(c->c_read_len.ensure((size_t)(R + 2) * sizeof(long long)));

  SelArgs a;
  a.tokens = c->tokens.as<int>();
  a.read_off = c->read_off.as<long long>();
  a.tok_node = c->tok_node.as<int>();
  a.read_fix = c->read_fix.as<unsigned char>();
  a.pos_off = (c->have_pos && !c->pos_identity) ? c->pos_off.as<long long>() : nullptr;
  a.read_len = c->have_read_len ? c->read_len.as<long long>() : nullptr;
  a.allowed = mode == AMG_SELECT_JUNK ? c->s1.as<long long>() : nullptr;
  a.n_allowed = mode == AMG_SELECT_JUNK ? n_allowed : 0;
  a.n_reads = R;
  a.k = c->k;
  a.mode = mode;
  a.invert = invert != 0 ? 1 : 0;
  a.have_pos = c->have_pos ? 1 : 0;
  a.verdict = c->s0.as<unsigned char>();
  a.keep = c->s2.as<unsigned int>();
  a.len = a.keep + per_read;
  a.masked_in = c->s4.as<unsigned long long>();
  unsigned long long* n_alive = a.masked_in + 256;
  a.max_win = a.masked_in + 257;
  long long* new_idx = c->s3.as<long long>();
  long long* new_off = new_idx + per_read;

  stage_begin(c, "select_classify");
  if (mode == AMG_SELECT_JUNK)
    HIPCHK(hipMemcpyAsync(c->s1.p, allowed, (size_t)n_allowed * sizeof(long long), hipMemcpyHostToDevice, st));
  {
    ClearList cl;
    cl.add(a.masked_in, (256 + 2) * sizeof(unsigned long long));
    AMGCHK(clear_many(c, cl));
  }
  if (R > 0) hipLaunchKernelGGL(k_sel_classify, dim3(nblk(R, 4 * SEL_READS)), dim3(256), 0, st, a);
  if (c->n_nodes > 0)
    hipLaunchKernelGGL(k_sel_count_alive, dim3(nblk(c->n_nodes, 256 * 16) < 1024u ? nblk(c->n_nodes, 256 * 16) : 1024u),
                       dim3(256), 0, st, c->node_alive.as<unsigned char>(), (long long)c->n_nodes, n_alive);
  stage_end(c);

  stage_begin(c, "select_pack");
  AMGCHK(prim_exscan_u32_pair(c, a.keep, new_idx, a.len, new_off, (size_t)R));
  SelPack Pk;
  Pk.a = a;
  Pk.new_idx = new_idx;
  Pk.new_off = new_off;
  Pk.o_tok = c->c_tokens_buf.as<int>();
  Pk.o_off = c->c_read_off.as<long long>();
  Pk.o_orig = c->c_orig.as<int>();
  Pk.o_changed = c->c_changed.as<unsigned char>();
  Pk.o_src = c->c_src.as<long long>();
  Pk.o_posoff = c->have_pos ? c->c_pos_off.as<long long>() : nullptr;
  Pk.o_rl = c->have_read_len ? c->c_read_len.as<long long>() : nullptr;
  if (R > 0)
    hipLaunchKernelGGL(k_sel_pack, dim3(nblk(R, 4 * SEL_READS)), dim3(256), 0, st, Pk);
  else
    HIPCHK(hipMemsetAsync(c->c_read_off.p, 0, sizeof(long long), st));
  // the call's one synchronisation
  FetchList l;
  l.add(new_idx + R);
  l.add(new_off + R);
  for (int i = 0; i < 16; ++i) l.add(a.masked_in + 16 * i);
  l.add(n_alive);
  l.add(a.max_win);
  unsigned long long v[20];
  AMGCHK(fetch(c, l, v));
  stage_end(c);

  if (sel_check_table(mode, (int64_t)v[19], n_allowed, why, sizeof why))
    return amg_fail(AMG_E_ARG, "amg_select_reads: %s", why);
  if (verdict && R > 0) {  // (only when asked for)
    HIPCHK(hipMemcpyAsync(verdict, a.verdict, (size_t)R, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  // the next build's node table: every window of a read in the set is an alive node of this graph or one of the set's
  // masked windows (an upper bound: masked windows may share a node)
  unsigned long long bound = v[18];
  for (int i = 0; i < 16; ++i) bound += v[2 + i];
  ctx_corrected_made(c, (int64_t)v[0], (int64_t)v[1], c->pos1_used, false, (int64_t)bound, getenv("AMG_TEST_NODE_BOUND"));
  if (n_out_reads) *n_out_reads = c->c_reads;
  if (n_out_tokens) *n_out_tokens = c->c_tokens;
  return AMG_OK;
}
