// amg_correct_nw.hip — position carry-over of the re-threaded reads (stage correct_positions of amg_correct_reads;
// reference construct_graph.py:1314-1325, 1433-1480, 1669-1691): sizes and places of what the carry-over produces,
// the general and the register-resident Needleman-Wunsch kernel with their named steps, and the host functions
// that run them.  (Pipeline: amg_correct.hip.  The kernels' limits: amg_correct.h.  Test entry: amg_nw_probe.hip.)
#include "amg_correct.h"
static constexpr long long NW_NONE = (long long)0x8000000000000000ull;  // a position that is None

// ---- the general kernel (any N, M): one wave per read, its steps
// needleman_wunsch's matrix (:1433-1456) by anti-diagonals, 64 cells at a time: pointers into P, scores in three
// rolling diagonals of N + 1 ints at dg
__device__ __forceinline__ void nw_fill_antidiagonals(const int* x, const int* y, int N, int M, int lane, int* dg,
                                                      unsigned char* P) {
  int* d0 = dg;            // anti-diagonal d-2, entry i+1 holds F[i, d-2-i]
  int* d1 = d0 + (N + 1);  // anti-diagonal d-1
  int* d2 = d1 + (N + 1);  // anti-diagonal d
  // borders (:1439-1445): F[-1,-1] = 0, F[i,-1] = -i, F[-1,j] = -j
  for (int d = 0; d <= N + M - 2; ++d) {
    int ilo = d - (M - 1) > 0 ? d - (M - 1) : 0;
    int ihi = d < N - 1 ? d : N - 1;
    for (int i = ilo + lane; i <= ihi; i += 64) {
      int j = d - i;
      int f_dd = (i == 0 && j == 0) ? 0 : (i == 0 ? -(j - 1) : (j == 0 ? -(i - 1) : d0[i]));
      int f_im1 = (i == 0) ? -j : d1[i];      // F[i-1, j]
      int f_jm1 = (j == 0) ? -i : d1[i + 1];  // F[i, j-1]
      int s_diag_ = f_dd + (x[i] == y[j] ? 1 : 0);
      int s_left = f_im1 - 1;  // pointer LEFT = (-1, 0)
      int s_up = f_jm1 - 1;    // pointer UP   = (0, -1)
      // max over (score, pointer) tuples: on ties UP (0,-1) > LEFT (-1,0) > DIAG (-1,-1)
      int best = s_diag_;
      unsigned char ptr = 0;
      if (s_left >= best) { best = s_left; ptr = 1; }
      if (s_up >= best) { best = s_up; ptr = 2; }
      d2[i + 1] = best;
      P[(long long)i * M + j] = ptr;
    }
    __syncthreads();
    int* t = d0; d0 = d1; d1 = d2; d2 = t;
  }
}

// traceback (:1458-1480), one lane; ops are collected back to front.  Returns their number.
__device__ __forceinline__ int nw_traceback(const unsigned char* P, int N, int M, unsigned char* ops) {
  int n_ops = 0, i = N - 1, j = M - 1;
  while (i >= 0 && j >= 0) {
    unsigned char p = P[(long long)i * M + j];
    ops[n_ops++] = p;
    if (p == 0) { --i; --j; }
    else if (p == 1) --i;
    else --j;
  }
  while (i >= 0) { ops[n_ops++] = 1; --i; }
  while (j >= 0) { ops[n_ops++] = 2; --j; }
  return n_ops;
}

// carry positions over (:1314-1325), alignment walked front to back by one lane.  A mismatching diagonal column yields
// (None, None) WITHOUT consuming an original position.  (nwf_positions_from_ops' rule, serial: two on purpose.)
__device__ __forceinline__ void nw_carry_over(const unsigned char* ops, int n_ops, const int* x, const int* y,
                                              const long long* ogs, const long long* oge, long long* o_gs,
                                              long long* o_ge) {
  int xi = 0, yj = 0, cur = 0, out = 0;
  for (int o = n_ops - 1; o >= 0; --o) {
    unsigned char p = ops[o];
    if (p == 0) {
      if (x[xi] == y[yj]) {
        o_gs[out] = ogs[cur];
        o_ge[out] = oge[cur];
        ++cur;
      } else {
        o_gs[out] = NW_NONE;
        o_ge[out] = NW_NONE;
      }
      ++out; ++xi; ++yj;
    } else if (p == 1) {
      o_gs[out] = NW_NONE;
      o_ge[out] = NW_NONE;
      ++out; ++xi;
    } else {
      ++cur; ++yj;
    }
  }
}

// replace_invalid_gene_positions (:1669-1691), one lane, in place: prev_end is the end of the last entry that was
// valid BEFORE repair; the look-ahead only sees entries that are still unrepaired.  (The same rule as nwf_repair,
// serial: two algorithms on purpose, the tests hold them equal.)
__device__ __forceinline__ void nw_repair(long long* o_gs, long long* o_ge, int N, long long rl) {
  long long prev_end = 0;
  for (int q = 0; q < N; ++q) {
    long long sv = o_gs[q], ev = o_ge[q];
    if (ev != NW_NONE) prev_end = ev;
    if (sv == NW_NONE && ev == NW_NONE) {
      long long nxt = NW_NONE;
      for (int w = q + 1; w < N; ++w)
        if (o_gs[w] != NW_NONE) { nxt = o_gs[w]; break; }
      o_gs[q] = prev_end;
      o_ge[q] = (nxt != NW_NONE) ? nxt : rl - 1;
    }
  }
}

__global__ __launch_bounds__(64) void k_corr_nw(NwArgs A) {
  __shared__ unsigned char s_ptr[NW_LDS_CELLS];
  __shared__ int s_diag[3 * (NW_LDS_N + 1)];
  __shared__ unsigned char s_ops[2 * NW_LDS_N];
  const CorrArgs& a = A.a;
  const long long gi = blockIdx.x;
  if (gi >= A.n_gapped) return;
  const long long r = A.rec[gi].r, pdst = A.rec[gi].pdst;
  if (a.cls_final[r] == RC_KEEP_ORIG) return;  // original genes kept: positions untouched
  const int lane = threadIdx.x;
  const long long t0 = a.read_off[r];
  const int M = (int)(a.read_off[r + 1] - t0);  // y = original genes
  const int N = (int)a.new_len[r];              // x = corrected genes
  if (A.allow_fast && nw_fast_ok(N, M)) return;  // k_corr_nw_fast handles it
  const int* x = a.tmp_tok + a.tmp_off[r];
  const int* y = a.tokens + t0;
  const long long *ogs, *oge;
  pos_base(a, A.rec[gi].poff, ogs, oge);
  unsigned char *P = s_ptr, *ops = s_ops;
  int* dg = s_diag;
  if (!nw_in_lds(N, M)) {  // the scratch k_nw_sizes sized
    unsigned char* base = A.big_buf + A.big_off[gi];
    P = base;
    ops = base + nw_scratch_ops_at(N, M);
    dg = reinterpret_cast<int*>(base + nw_scratch_diag_at(N, M));
  }
  nw_fill_antidiagonals(x, y, N, M, lane, dg, P);
  if (lane != 0) return;
  const int n_ops = nw_traceback(P, N, M, ops);
  nw_carry_over(ops, n_ops, x, y, ogs, oge, A.o_gs + pdst, A.o_ge + pdst);
  nw_repair(A.o_gs + pdst, A.o_ge + pdst, N, a.read_len ? a.read_len[r] : 0);
}

// ---- fast path: M <= 64 original genes, N <= 128 corrected genes.  One wave per read, no workgroup barriers: lane j
// owns column j of the DP matrix and the wave computes one row per step — F[i-1,j] stays in the lane's own register,
// F[i-1,j-1] arrives from lane j-1 by a DPP shift, the dependency along the row is a prefix maximum (DPP scan).
// Pointers are packed 2 bits per cell (16 rows per word per lane).
struct NwfLds {  // one read's staging
  int x[NWF_MAX_N];
  unsigned int opw[(NWF_MAX_N + NWF_MAX_M) / 16 + 1];  // alignment ops, 2 bits each
  long long gs[NWF_MAX_N];
  long long ge[NWF_MAX_N];
  long long ogs[NWF_MAX_M];  // positions of the original genes
  long long oge[NWF_MAX_M];
};
// alignment ops, 2 bits each, 16 per word of NwfLds::opw: wave-uniform, lane 0 stores a word when it is full
struct NwfOps {
  unsigned int pack = 0;  // the word being filled
  int n = 0;              // ops so far
  __device__ __forceinline__ void push(unsigned int p, int lane, unsigned int* opw) {
    pack |= p << ((n & 15) * 2);
    if ((n & 15) == 15) {
      if (lane == 0) opw[n >> 4] = pack;
      pack = 0;
    }
    ++n;
  }
  __device__ __forceinline__ void flush(int lane, unsigned int* opw) const {
    if ((n & 15) != 0 && lane == 0) opw[n >> 4] = pack;
  }
};

// ---- the steps of nw_fast_read, each done by the whole wave on the read's staging S
// Equal-length rule, m == 3 or 4 mismatches (mm; eq_a: x[i] == y[i+1], eq_b: x[i+1] == y[i]): is the diagonal the
// unique optimum?  The diagonal scores N - m >= N - 4, any alignment with two or more gaps per list at most N - 5, so
// only the alignments with ONE gap in each list can reach it.  Such an alignment runs on the diagonal up to its first
// gap at u, one place off it (x[i] against y[i+1], or the mirror image) up to its second gap at l, and on the diagonal
// again; it scores its matches - 2, + 1 when the first gap is a leading one (u = 0: the first gap of a leading run is
// free).  With the match indicators as bit masks (D diagonal, S shifted) its matches are prefD(u) - prefS(u) +
// prefS(l) + sufD(l): the best over u <= l is a prefix maximum over the lanes.  If even the best such alignment stays
// BELOW N - m the diagonal is the unique optimum (a tie would not do: the traceback prefers gaps).  Checked
// exhaustively against the reference's alignment in tests/test_nw_shortcut_cpu.py.
__device__ __forceinline__ bool nwf_one_gap_stays_below(int N, int m, unsigned long long mm, unsigned long long eq_a,
                                                        unsigned long long eq_b, int lane) {
  const unsigned long long dmask = ~mm & (N == 64 ? ~0ull : ((1ull << N) - 1ull));
  const unsigned long long below = (1ull << lane) - 1ull;
  const int prefD = __popcll(dmask & below);
  const int sufD = lane >= 63 ? 0 : __popcll(dmask >> (lane + 1));
  const int ID = (int)0x80000000 / 2;
  int best = ID;
#pragma unroll
  for (int side = 0; side < 2; ++side) {
    const int prefS = __popcll((side == 0 ? eq_a : eq_b) & below);
    const int g = wave_prefix_max(lane < N ? prefD - prefS + (lane == 0 ? 1 : 0) : ID, ID);
    int h = lane < N ? g + prefS + sufD - 2 : ID;
    for (int d = 32; d > 0; d >>= 1) h = max(h, __shfl_xor(h, d, 64));
    best = max(best, h);
  }
  return best < N - m;
}

// Place along a diagonal (both shortcuts; N <= 64): a matched column q takes original position number
// start + (matched columns before q), anything else is (None, None)
__device__ __forceinline__ void nwf_place_diagonal(NwfLds& S, int N, unsigned long long matched, int start, int lane) {
  if (lane >= N) return;
  const bool match = ((matched >> lane) & 1ull) != 0ull;
  const int cur = start + __popcll(matched & ((1ull << lane) - 1ull));
  S.gs[lane] = match ? S.ogs[cur] : NW_NONE;
  S.ge[lane] = match ? S.oge[cur] : NW_NONE;
}

// Fill, one matrix ROW per step (N steps instead of the N + M - 1 anti-diagonals of a systolic sweep, which also
// idles half the lanes while it ramps up and down).  Lane j owns column j and keeps F[i-1, j].  With c_j =
// max(F[i-1,j-1] + match, F[i-1,j] - 1) the row is
//   F[i, j] = max(c_j, F[i, j-1] - 1) = max_{k <= j} (c_k + k) - j   (F[i,-1] = -i enters as k = -1)
// i.e. a prefix maximum over the lanes: six DPP steps.  The pointer follows from the three candidates with the
// reference's tie order UP (0,-1) > LEFT (-1,0) > DIAG.  Pointers stay in registers: 2 bits per cell, word b of lane
// j = rows 16b .. 16b+15 of column j.
__device__ __forceinline__ void nwf_fill(int N, int x0, int x1, int yj, int lane,
                                         unsigned int (&ptrs)[NWF_MAX_N / 16]) {
  int Fp = -lane;  // F[-1, j] = -j
#pragma unroll
  for (int blk = 0; blk < NWF_MAX_N / 16; ++blk) {
    unsigned int acc = 0;
    const int iend = N < blk * 16 + 16 ? N : blk * 16 + 16;
    for (int i = blk * 16; i < iend; ++i) {
      const int xi = blk < 4 ? __builtin_amdgcn_readlane(x0, i) : __builtin_amdgcn_readlane(x1, i - 64);
      // F[i-1, j-1]; lane 0 takes the border F[i-1, -1] = -(i-1), F[-1,-1] = 0
      const int fd = __builtin_amdgcn_update_dpp(i == 0 ? 0 : 1 - i, Fp, 0x138, 0xf, 0xf, false);
      const int s_d = fd + (xi == yj ? 1 : 0);
      const int s_l = Fp - 1;  // from F[i-1, j]: pointer LEFT = (-1, 0)
      const int c = s_d > s_l ? s_d : s_l;
      const int Fc = max(wave_prefix_max(c + lane, (int)0x80000000), -i - 1) - lane;  // F[i, j]
      // F[i, j-1] - 1: pointer UP = (0, -1); lane 0 takes the border F[i, -1] = -i
      const int s_u = __builtin_amdgcn_update_dpp(-i, Fc, 0x138, 0xf, 0xf, false) - 1;
      const unsigned int ptr = s_u >= c ? 2u : (s_l >= s_d ? 1u : 0u);
      acc |= ptr << ((i & 15) * 2);
      Fp = Fc;
    }
    ptrs[blk] = acc;
  }
}

// Traceback on the scalar unit: i, j and the ops are wave-uniform, a pointer is one
// v_readlane away (no LDS round trip per step).  Ops are collected back to front into S.opw; returns their number.
__device__ __forceinline__ int nwf_traceback(int N, int M, const unsigned int (&ptrs)[NWF_MAX_N / 16], int lane,
                                             NwfLds& S) {
  NwfOps ops;
  int i = N - 1, j = M - 1;
#pragma unroll
  for (int blk = NWF_MAX_N / 16 - 1; blk >= 0; --blk) {
    while (i >= blk * 16 && j >= 0) {
      const unsigned int w = (unsigned int)__builtin_amdgcn_readlane((int)ptrs[blk], j);
      const unsigned int p = (w >> ((i & 15) * 2)) & 3u;
      ops.push(p, lane, S.opw);
      if (p == 0) { --i; --j; }
      else if (p == 1) --i;
      else --j;
    }
  }
  for (; i >= 0; --i) ops.push(1u, lane, S.opw);  // leading corrected genes: LEFT
  for (; j >= 0; --j) ops.push(2u, lane, S.opw);  // leading original genes: UP
  ops.flush(lane, S.opw);
  return ops.n;
}

// Positions from the ops, in parallel over the alignment columns (front to back, 64 per step): nw_carry_over's rule
// with ballots and popcounts for its counters (two algorithms on purpose, the tests hold them equal)
__device__ __forceinline__ void nwf_positions_from_ops(int n_ops, int yj, int lane, NwfLds& S) {
  int base_x = 0, base_y = 0, base_cur = 0;
  for (int c0 = 0; c0 < n_ops; c0 += 64) {
    const int f = c0 + lane;
    const bool in = f < n_ops;
    const int g = in ? n_ops - 1 - f : 0;
    const unsigned int op = in ? (S.opw[g >> 4] >> ((g & 15) * 2)) & 3u : 3u;
    const bool isx = in && (op == 0 || op == 1), isy = in && (op == 0 || op == 2);
    const unsigned long long lt = (1ull << lane) - 1ull;
    const unsigned long long bx = __ballot(isx), by = __ballot(isy);
    const int xi = base_x + __popcll(bx & lt), yy = base_y + __popcll(by & lt);
    const int ysel = __shfl(yj, yy < 64 ? yy : 0, 64);  // all lanes take part in the shuffle
    const bool match = in && op == 0 && S.x[xi < NWF_MAX_N ? xi : 0] == ysel;
    const bool inc = in && (op == 2 || match);
    const unsigned long long bc = __ballot(inc);
    const int cur = base_cur + __popcll(bc & lt);
    if (isx) {
      S.gs[xi] = match ? S.ogs[cur < NWF_MAX_M ? cur : 0] : NW_NONE;
      S.ge[xi] = match ? S.oge[cur < NWF_MAX_M ? cur : 0] : NW_NONE;
    }
    base_x += __popcll(bx);
    base_y += __popcll(by);
    base_cur += __popcll(bc);
  }
}

// Repair and store: replace_invalid_gene_positions (:1669-1691), each lane repairs its own entries from the
// UNREPAIRED staging (the rule of nw_repair, parallel: two algorithms on purpose, the tests hold them equal)
__device__ __forceinline__ void nwf_repair(const NwArgs& A, int N, long long pdst, long long rl, int lane,
                                           const NwfLds& S) {
  for (int q = lane; q < N; q += 64) {
    long long sv = S.gs[q], ev = S.ge[q];
    if (sv == NW_NONE && ev == NW_NONE) {
      long long prev_end = 0;
      for (int w = q - 1; w >= 0; --w)
        if (S.ge[w] != NW_NONE) { prev_end = S.ge[w]; break; }
      long long nxt = NW_NONE;
      for (int w = q + 1; w < N; ++w)
        if (S.gs[w] != NW_NONE) { nxt = S.gs[w]; break; }
      sv = prev_end;
      ev = (nxt != NW_NONE) ? nxt : rl - 1;
    }
    A.o_gs[pdst + q] = sv;
    A.o_ge[pdst + q] = ev;
  }
}

// One read, carried over by one wave.  The staging, the two shortcuts' verdicts and their placement are one body (the
// rules stated where they stand): cut into steps of their own they compiled to a kernel 2 - 3 % slower on its chain of
// dependent loads (profiles/carry_over_steps_NOTES.md).  Fill, traceback, positions and repair are steps.
__device__ __forceinline__ void nw_fast_read(const NwArgs& A, long long gi, int lane, NwfLds& S) {
  const CorrArgs& a = A.a;
  // ---- stage.  The kernel is bound by its chain of dependent global loads (one wave per read, ~15 us per wave at full
  // occupancy), not by the fill: one record load, then every per-gene load of the read in one batch (the original
  // positions included: the carry-over reads them from LDS), then only stores.
  const NwRec q = A.rec[gi];
  // wave-uniform by construction; tell the compiler so that loop control stays scalar
  const int N = __builtin_amdgcn_readfirstlane(q.N);
  if (N == 0) return;  // original genes kept, or a read for k_corr_nw
  const int M = __builtin_amdgcn_readfirstlane(q.M);
  const long long r = q.r, t0 = q.t0, dst = q.dst, pdst = q.pdst;
  const int x0 = lane < N ? a.tmp_tok[dst + lane] : -2;            // corrected genes 0..63
  const int x1 = lane + 64 < N ? a.tmp_tok[dst + lane + 64] : -2;  // and 64..127, one per lane
  const int yj = lane < M ? a.tokens[t0 + lane] : -1;
  const long long *pgs, *pge;
  pos_base(a, q.poff, pgs, pge);
  const long long ogs = lane < M ? pgs[lane] : 0;
  const long long oge = lane < M ? pge[lane] : 0;
  const long long rl = a.read_len ? a.read_len[r] : 0;  // (with the batch: not a third dependent round trip)
  if (lane < N) S.x[lane] = x0;
  if (lane + 64 < N) S.x[lane + 64] = x1;
  S.ogs[lane] = ogs;
  S.oge[lane] = oge;
  // ---- shortcut: equally long gene lists that differ in a few places.
  // With the reference's scores (match +1, mismatch 0, gap -1, and borders F[i,-1] = -i, F[-1,j] = -j that make the
  // first gap of a LEADING run free) an alignment of two lists of the same length N with p >= 1 gaps in each scores at
  // most (N - p) - 2p + 1 <= N - 2, the pure diagonal N - m for m mismatching places.  m <= 1: the diagonal is the only
  // optimum.  m == 2 (mismatches at a < b): N - 2 is reached only by "one free leading gap, N - 1 matches, one gap of
  // the other kind somewhere": y[0] skipped, x[i] == y[i+1] up to the gap that skips x[j], plain matches after it —
  // which needs j >= b (no mismatch may follow the gap) and therefore x[i] == y[i+1] for all i < b; or the mirror image
  // with x[i+1] == y[i].  If neither holds the diagonal is again the only optimum.  A unique optimum is what the
  // traceback returns whatever the tie order, so the matrix is not needed: columns are (x[q], y[q]), a mismatching
  // column gives (None, None) and does not consume an original position (:1314-1325).  (Tandem gene arrays do produce
  // the tie: found by tools/fuzz_sweep.py, kept as tests/golden/data/nw_tie_case.json.xz.)  m == 3, 4: the function above.
  bool diagonal = false;
  int route = NW_ROUTE_FILL;  // what settles this read (wave-uniform; only amg_nw_probe asks)
  if (N == M) {
    const unsigned long long mm = __ballot(lane < N && x0 != yj);
    const int m = __popcll(mm);
    diagonal = m <= 1;
    const int x_next = __shfl_down(x0, 1, 64), y_next = __shfl_down(yj, 1, 64);  // every lane shuffles
    const unsigned long long eq_a = __ballot(lane < N - 1 && x0 == y_next);  // x[i] == y[i+1]
    const unsigned long long eq_b = __ballot(lane < N - 1 && x_next == yj);  // x[i+1] == y[i]
    if (m == 2) {
      const int b = 63 - __clzll((long long)mm);               // the later mismatch, b >= 1
      const unsigned long long upto_b = (1ull << b) - 1ull;    // places 0 .. b-1
      diagonal = (eq_a & upto_b) != upto_b && (eq_b & upto_b) != upto_b;
    } else if (m == 3 || m == 4) {
      diagonal = nwf_one_gap_stays_below(N, m, mm, eq_a, eq_b, lane);
    }
    diagonal = diagonal && A.shortcuts != 0;
    if (diagonal) route = NW_ROUTE_EQUAL;
    if (diagonal) nwf_place_diagonal(S, N, ~mm, 0, lane);
  }
  // ---- second shortcut: the OFFSET-DIAGONAL CERTIFICATE, for a corrected list that is the original one with an end
  // trimmed off and a few genes replaced (one re-threaded read in four of the cleaning sweep, and every one of them
  // filled a matrix: ~3 000 instructions).  If every gene of x occurs in y at most once, and where it does at i + s for
  // ONE offset s in [0, M - N], and at least two genes match, then: nothing off diagonal s scores, a detour from it
  // costs two gaps, so every optimal alignment runs along diagonal s from the first to the last match; the ties that
  // remain (where the s leading and M - N - s trailing gaps sit among the unmatched genes at either end) never move a
  // matched column.  What the reference carries over (:1314-1325) is then: matched x[q] -> original position number
  // s + (matches before q) — a gap column and a match consume an original position, a mismatching column does not —
  // unmatched -> (None, None).  Checked against the reference's alignment exhaustively on short lists and on random
  // trimmed / substituted / repeated ones in tests/test_nw_shortcut_cpu.py.
  if (!diagonal && A.shortcuts != 0 && N <= M && N >= 2) {  // (M <= 64 here: lane j holds y[j])
    int s_off = 0x7fffffff;
    bool ok = true;
    unsigned long long matched = 0ull;
    for (int i = 0; i < N && ok; ++i) {  // wave-uniform: one gene of x against all of y per step
      const int g = __builtin_amdgcn_readlane(x0, i);
      const unsigned long long at = __ballot(lane < M && yj == g);
      if (at != 0ull) {
        const int si = __ffsll((long long)at) - 1 - i;
        ok = (at & (at - 1ull)) == 0ull && (s_off == 0x7fffffff || si == s_off);
        s_off = si;
        matched |= 1ull << i;
      }
    }
    ok = ok && s_off != 0x7fffffff && s_off >= 0 && s_off <= M - N && __popcll(matched) >= 2;
    if (ok) {
      diagonal = true;
      route = NW_ROUTE_CERT;
      nwf_place_diagonal(S, N, matched, s_off, lane);
    }
  }
  if (!diagonal) {
    unsigned int ptrs[NWF_MAX_N / 16];
    nwf_fill(N, x0, x1, yj, lane, ptrs);
    const int n_ops = nwf_traceback(N, M, ptrs, lane, S);
    wave_sync();
    nwf_positions_from_ops(n_ops, yj, lane, S);
  }
  wave_sync();
  if (A.route && lane == 0) A.route[gi] = (unsigned char)route;
  nwf_repair(A, N, pdst, rl, lane, S);
}

// One read, one wave, one workgroup (as GF_WPB: most reads take a shortcut, some fill a matrix, and a workgroup's LDS is
// held for its last wave: 0.94 ms with four reads per workgroup, 0.87 with two, 0.71 with one).  (Sixteen lanes per read
// for the reads whose alignment is provably the diagonal, three in four, were measured in round 5: 0.27 ms for them plus
// 0.56 ms for the others against 0.575 ms for everybody here: the diagonal ones ride along for nothing.)
__global__ __launch_bounds__(64) void k_corr_nw_fast(NwArgs A) {
  __shared__ NwfLds s_lds;
  if ((long long)blockIdx.x < A.n_gapped) nw_fast_read(A, (long long)blockIdx.x, (int)threadIdx.x, s_lds);
}

// per gapped read: the record k_corr_nw_fast starts from, its new positions, and the bytes of global scratch
// k_corr_nw needs for it (0 when its matrix stays in LDS)
__global__ void k_nw_sizes(const int* __restrict__ gapped, long long n_gapped,
                           const long long* __restrict__ read_off, const unsigned int* __restrict__ new_len,
                           const long long* __restrict__ tmp_off, const long long* __restrict__ new_off,
                           const unsigned char* __restrict__ final_cls, long long* __restrict__ size,
                           int allow_fast, unsigned long long* n_general, NwRec* __restrict__ rec,
                           const long long* __restrict__ pos_off, long long* __restrict__ plen) {
  long long gi = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gi >= n_gapped) return;
  long long r = gapped[gi];
  long long N = new_len[r], M = read_off[r + 1] - read_off[r];
  const bool carried = final_cls[r] != RC_KEEP_ORIG;                // else: original genes and positions kept
  const bool fast = carried && allow_fast && nw_fast_ok(N, M);      // k_corr_nw_fast's, else k_corr_nw's
  // the record: one 32-byte load instead of a chain of dependent per-read loads at the head of a latency-bound kernel
  NwRec q;
  q.r = (int)r;
  q.M = (int)(M > 0x7fffffff ? 0x7fffffff : M);
  q.N = fast ? (int)N : 0;  // 0: not for the fast kernel
  q.pad = 0;
  q.t0 = read_off[r];
  q.dst = tmp_off[r];
  q.pdst = 0;  // k_nw_place
  q.poff = pos_off ? pos_off[r] : read_off[r];
  rec[gi] = q;
  plen[gi] = carried ? N : 0;  // new positions of this read
  size[gi] = (carried && !nw_in_lds(N, M)) ? nw_scratch_bytes(N, M) : 0;
  if (carried && !fast) atomicAdd(n_general, 1ull);
}

// where the new positions of gapped read gi go (pool of produced positions, after `base`)
__global__ void k_nw_place(long long n_gapped, const long long* __restrict__ poffs, long long base, long long n0,
                           NwRec* __restrict__ rec, long long* __restrict__ pos_new) {
  long long gi = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (gi >= n_gapped) return;
  const long long at = base + poffs[gi];
  rec[gi].pdst = at;
  pos_new[rec[gi].r] = n0 + at;
}

// device allocation that keeps its first `used` bytes when it has to grow
static int grow_keep(amg_ctx* c, DevBuf& b, size_t need, size_t used) {
  if (need <= b.cap && !b.borrowed) return AMG_OK;
  DevBuf nb;
  AMGCHK(nb.ensure(need + need / 2));
  if (used && b.p) HIPCHK(hipMemcpyAsync(nb.p, b.p, used, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  b.release();
  b = nb;
  return AMG_OK;
}

// ------------------------------------------------------------------ the host's steps
int corr_nw_sizes(amg_ctx* c, const CorrSwitches& sw, const CorrScratch& S, const CorrArgs& a, long long n_gapped,
                  FetchList& shape) {
  ClearList cl;
  cl.add(S.nw_size, (size_t)(n_gapped + 1) * sizeof(long long));
  cl.add(S.plen, (size_t)(n_gapped + 1) * sizeof(long long));
  cl.add(S.n_general, sizeof(unsigned long long));
  AMGCHK(clear_many(c, cl));
  AMGCHK(c->nw_rec.ensure((size_t)(n_gapped + 1) * sizeof(NwRec)));
  // (global scratch only for reads too large for the register-resident kernel)
  hipLaunchKernelGGL(k_nw_sizes, dim3(nblk(n_gapped, 256)), dim3(256), 0, c->stream, S.glist->as<int>(),
                     n_gapped, a.read_off, S.new_len, S.tmp_off, S.new_off, S.final_cls, S.nw_size, sw.fast_nw,
                     S.n_general, c->nw_rec.as<NwRec>(), a.pos_off, S.plen);
  AMGCHK(prim_exscan_i64_pair(c, S.nw_size, S.nw_off, S.plen, S.poffs, (size_t)n_gapped));
  shape.add(S.nw_off + n_gapped);
  shape.add(S.poffs + n_gapped);
  shape.add(S.n_general);
  return AMG_OK;
}

int corr_grow_pos_pools(amg_ctx* c, const CorrCounts& n) {
  AMGCHK(c->nw_big.ensure((size_t)n.big_total + 64));
  // the pool of produced positions grows by what this correction adds (earlier entries stay:
  // reads corrected before keep pointing at them)
  const size_t used = (size_t)c->pos1_used * sizeof(long long);
  const size_t need = (size_t)(c->pos1_used + n.pos_total + 64) * sizeof(long long);
  AMGCHK(grow_keep(c, c->pos1_s, need, used));
  AMGCHK(grow_keep(c, c->pos1_e, need, used));
  return AMG_OK;
}

int corr_positions(amg_ctx* c, const CorrSwitches& sw, const CorrScratch& S, const CorrArgs& a, const CorrCounts& n,
                   unsigned char* route) {
  hipStream_t st = c->stream;
  const long long n_gapped = n.n_gapped;
  hipLaunchKernelGGL(k_nw_place, dim3(nblk(n_gapped, 256)), dim3(256), 0, st, n_gapped, S.poffs,
                     (long long)c->pos1_used, (long long)c->pos_n0, c->nw_rec.as<NwRec>(), S.pos_new);
  NwArgs W;
  W.a = a;  // (a.cls_final is S.final_cls, here and in amg_nw_probe: the kernels read the classes through it)
  W.rec = c->nw_rec.as<NwRec>();
  W.o_gs = c->pos1_s.as<long long>();
  W.o_ge = c->pos1_e.as<long long>();
  W.n_gapped = n_gapped;
  W.big_off = S.nw_off;
  W.big_buf = c->nw_big.as<unsigned char>();
  W.allow_fast = sw.fast_nw;
  W.shortcuts = sw.nw_shortcuts;
  W.route = route;
  if (W.allow_fast) hipLaunchKernelGGL(k_corr_nw_fast, dim3((unsigned int)n_gapped), dim3(64), 0, st, W);
  if (n.n_general > 0)  // reads too long for the register-resident kernel
    hipLaunchKernelGGL(k_corr_nw, dim3((unsigned int)n_gapped), dim3(64), 0, st, W);
  return AMG_OK;
}
