// amg_correct_nw.hip — position carry-over of the re-threaded reads (stage correct_positions of amg_correct_reads;
// reference construct_graph.py:1314-1325, 1433-1480, 1669-1691): sizes and places of what the carry-over produces,
// the register-resident and the general Needleman-Wunsch kernel, with the host functions that run them.
// (Pipeline: amg_correct.hip.)
#include "amg_correct.h"

// ---- positions for gapped reads: one wave per read (general path: any N, M)
#define NW_LDS_N 1024       // rows kept in LDS (rolling anti-diagonals, op list)
#define NW_LDS_CELLS 16384  // pointer-matrix cells kept in LDS (one byte each)
__global__ __launch_bounds__(64) void k_corr_nw(NwArgs A) {
  __shared__ unsigned char s_ptr[NW_LDS_CELLS];
  __shared__ int s_diag[3 * (NW_LDS_N + 1)];
  __shared__ unsigned char s_ops[2 * NW_LDS_N];
  const CorrArgs& a = A.a;
  const long long gi = blockIdx.x;
  if (gi >= A.n_gapped) return;
  const long long r = A.rec[gi].r;
  const long long pdst = A.rec[gi].pdst;
  if (A.final_cls[r] == RC_KEEP_ORIG) return;  // original genes kept: positions untouched
  const int lane = threadIdx.x;
  const long long t0 = a.read_off[r];
  const int M = (int)(a.read_off[r + 1] - t0);  // y = original genes
  const int N = (int)a.new_len[r];              // x = corrected genes
  if (A.allow_fast && nw_fast_ok(N, M)) return;  // k_corr_nw_fast handles it
  const long long dst = a.tmp_off[r];
  const int* x = a.tmp_tok + dst;
  const int* y = a.tokens + t0;
  const long long *ogs, *oge;
  pos_base(a, A.rec[gi].poff, ogs, oge);
  unsigned char* P = s_ptr;
  int* dg = s_diag;
  unsigned char* ops = s_ops;
  const bool small = (N <= NW_LDS_N && M <= NW_LDS_N && (long long)N * M <= NW_LDS_CELLS);
  if (!small) {
    unsigned char* base = A.big_buf + A.big_off[gi];
    P = base;
    ops = base + (long long)N * M;
    dg = reinterpret_cast<int*>(base + (((long long)N * M + N + M + 15) & ~15ll));
  }
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
  if (lane != 0) return;
  // traceback (:1458-1480); ops are collected back to front
  int n_ops = 0;
  int i = N - 1, j = M - 1;
  while (i >= 0 && j >= 0) {
    unsigned char p = P[(long long)i * M + j];
    ops[n_ops++] = p;
    if (p == 0) { --i; --j; }
    else if (p == 1) --i;
    else --j;
  }
  while (i >= 0) { ops[n_ops++] = 1; --i; }
  while (j >= 0) { ops[n_ops++] = 2; --j; }
  // carry positions over (:1314-1325), alignment walked front to back.  A mismatching
  // diagonal column yields (None, None) WITHOUT consuming an original position.
  const long long NONE = (long long)0x8000000000000000ull;
  int xi = 0, yj = 0, cur = 0, out = 0;
  for (int o = n_ops - 1; o >= 0; --o) {
    unsigned char p = ops[o];
    if (p == 0) {
      if (x[xi] == y[yj]) {
        A.o_gs[pdst + out] = ogs[cur];
        A.o_ge[pdst + out] = oge[cur];
        ++cur;
      } else {
        A.o_gs[pdst + out] = NONE;
        A.o_ge[pdst + out] = NONE;
      }
      ++out; ++xi; ++yj;
    } else if (p == 1) {
      A.o_gs[pdst + out] = NONE;
      A.o_ge[pdst + out] = NONE;
      ++out; ++xi;
    } else {
      ++cur; ++yj;
    }
  }
  // replace_invalid_gene_positions (:1669-1691): prev_end is the end of the last entry that
  // was valid BEFORE repair; the look-ahead only sees entries that are still unrepaired.
  long long prev_end = 0;
  const long long rl = a.read_len ? a.read_len[r] : 0;
  for (int q = 0; q < N; ++q) {
    long long sv = A.o_gs[pdst + q], ev = A.o_ge[pdst + q];
    if (ev != NONE) prev_end = ev;
    if (sv == NONE && ev == NONE) {
      long long nxt = NONE;
      for (int w = q + 1; w < N; ++w)
        if (A.o_gs[pdst + w] != NONE) { nxt = A.o_gs[pdst + w]; break; }
      A.o_gs[pdst + q] = prev_end;
      A.o_ge[pdst + q] = (nxt != NONE) ? nxt : rl - 1;
    }
  }
}


// ---- fast path: M <= 64 original genes, N <= 128 corrected genes.  One wave per read, no
// workgroup barriers: lane j owns column j of the DP matrix and the wave computes one row per
// step — F[i-1,j] stays in the lane's own register, F[i-1,j-1] arrives from lane j-1 by a DPP
// shift, the dependency along the row is a prefix maximum (DPP scan).  Pointers are packed
// 2 bits per cell (16 rows per LDS word per lane).

#define NWF_WPB 1  // reads per workgroup (see GF_WPB: most reads take the shortcut, some fill a matrix:
                   // 0.94 ms with four, 0.87 with two, 0.71 with one)
struct NwfLds {  // one read's staging
  int x[NWF_MAX_N];
  unsigned int opw[(NWF_MAX_N + NWF_MAX_M) / 16 + 1];  // alignment ops, 2 bits each
  long long gs[NWF_MAX_N];
  long long ge[NWF_MAX_N];
  long long ogs[NWF_MAX_M];  // positions of the original genes
  long long oge[NWF_MAX_M];
};

__device__ __forceinline__ void nw_fast_read(const NwArgs& A, long long gi, int lane, NwfLds& S) {
  int (*s_x)[NWF_MAX_N] = &S.x;
  unsigned int (*s_opw)[(NWF_MAX_N + NWF_MAX_M) / 16 + 1] = &S.opw;
  long long (*s_gs)[NWF_MAX_N] = &S.gs;
  long long (*s_ge)[NWF_MAX_N] = &S.ge;
  long long (*s_ogs)[NWF_MAX_M] = &S.ogs;
  long long (*s_oge)[NWF_MAX_M] = &S.oge;
  const CorrArgs& a = A.a;
  const int wv = 0;
  // The kernel is bound by its chain of dependent global loads (one wave per read, ~15 us per
  // wave at full occupancy), not by the fill: one record load, then every per-gene load of the
  // read in one batch (the original positions included: the carry-over below reads them from
  // LDS), then only stores.
  const NwRec q = A.rec[gi];
  // wave-uniform by construction; tell the compiler so that loop control stays scalar
  const int N = __builtin_amdgcn_readfirstlane(q.N);
  if (N == 0) return;  // original genes kept, or a read for k_corr_nw
  const int M = __builtin_amdgcn_readfirstlane(q.M);
  const long long r = q.r, t0 = q.t0, dst = q.dst, pdst = q.pdst;
  int* X = s_x[wv];
  unsigned int* OPW = s_opw[wv];
  long long* GS = s_gs[wv];
  long long* GE = s_ge[wv];
  long long* OGS = s_ogs[wv];
  long long* OGE = s_oge[wv];
  const int x0 = lane < N ? a.tmp_tok[dst + lane] : -2;            // corrected genes 0..63
  const int x1 = lane + 64 < N ? a.tmp_tok[dst + lane + 64] : -2;  // and 64..127, one per lane
  const int yj = lane < M ? a.tokens[t0 + lane] : -1;
  const long long *pgs, *pge;
  pos_base(a, q.poff, pgs, pge);
  const long long ogs = lane < M ? pgs[lane] : 0;
  const long long oge = lane < M ? pge[lane] : 0;
  const long long rl = a.read_len ? a.read_len[r] : 0;  // (with the batch: not a third dependent round trip)
  if (lane < N) X[lane] = x0;
  if (lane + 64 < N) X[lane + 64] = x1;
  OGS[lane] = ogs;
  OGE[lane] = oge;
  // ---- shortcut: equally long gene lists that differ in at most two places.
  // With the reference's scores (match +1, mismatch 0, gap -1, and borders F[i,-1] = -i,
  // F[-1,j] = -j that make the first gap of a LEADING run free) an alignment of two lists of
  // the same length N with p >= 1 gaps in each scores at most (N - p) - 2p + 1 <= N - 2, the
  // pure diagonal N - m for m mismatching places.  m <= 1: the diagonal is the only optimum.
  // m == 2 (mismatches at a < b): N - 2 is reached only by "one free leading gap, N - 1
  // matches, one gap of the other kind somewhere": y[0] skipped, x[i] == y[i+1] up to the gap
  // that skips x[j], plain matches after it — which needs j >= b (no mismatch may follow the
  // gap) and therefore x[i] == y[i+1] for all i < b; or the mirror image with x[i+1] == y[i].
  // If neither holds the diagonal is again the only optimum.  A unique optimum is what the
  // traceback returns whatever the tie order, so the matrix is not needed: columns are
  // (x[q], y[q]), a mismatching column gives (None, None) and does not consume an original
  // position (:1314-1325).  (Tandem gene arrays do produce the tie: found by tools/fuzz_sweep.py,
  // kept as tests/golden/data/nw_tie_case.json.xz.)
  const long long NONE = (long long)0x8000000000000000ull;
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
      // Three or four mismatches: the diagonal scores N - m >= N - 4, any alignment with two or more gaps per
      // list at most N - 5, so only the alignments with ONE gap in each list can reach it.  Such an alignment
      // runs on the diagonal up to its first gap at u, one place off it (x[i] against y[i+1], or the mirror
      // image) up to its second gap at l, and on the diagonal again; it scores its matches - 2, + 1 when the
      // first gap is a leading one (u = 0: the first gap of a leading run is free).  With the match indicators
      // as bit masks (D diagonal, S shifted) its matches are prefD(u) - prefS(u) + prefS(l) + sufD(l): the best
      // over u <= l is a prefix maximum over the lanes.  If even the best such alignment stays BELOW N - m the
      // diagonal is the unique optimum (a tie would not do: the traceback prefers gaps).  Checked exhaustively
      // against the reference's alignment in tests/test_nw_shortcut_cpu.py.
      const unsigned long long dmask = ~mm & (N == 64 ? ~0ull : ((1ull << N) - 1ull));
      const unsigned long long below = (1ull << lane) - 1ull;
      const int prefD = __popcll(dmask & below);
      const int sufD = lane >= 63 ? 0 : __popcll(dmask >> (lane + 1));
      const int ID = (int)0x80000000 / 2;
      int best = ID;
#pragma unroll
      for (int side = 0; side < 2; ++side) {
        const int prefS = __popcll((side == 0 ? eq_a : eq_b) & below);
        int g = lane < N ? prefD - prefS + (lane == 0 ? 1 : 0) : ID;
        g = max(g, __builtin_amdgcn_update_dpp(ID, g, 0x111, 0xf, 0xf, false));  // row_shr:1
        g = max(g, __builtin_amdgcn_update_dpp(ID, g, 0x112, 0xf, 0xf, false));  // row_shr:2
        g = max(g, __builtin_amdgcn_update_dpp(ID, g, 0x114, 0xf, 0xf, false));  // row_shr:4
        g = max(g, __builtin_amdgcn_update_dpp(ID, g, 0x118, 0xf, 0xf, false));  // row_shr:8
        g = max(g, __builtin_amdgcn_update_dpp(ID, g, 0x142, 0xa, 0xf, false));  // row_bcast:15
        g = max(g, __builtin_amdgcn_update_dpp(ID, g, 0x143, 0xc, 0xf, false));  // row_bcast:31
        int h = lane < N ? g + prefS + sufD - 2 : ID;
        for (int d = 32; d > 0; d >>= 1) h = max(h, __shfl_xor(h, d, 64));
        best = max(best, h);
      }
      diagonal = best < N - m;
    }
    diagonal = diagonal && A.shortcuts != 0;
    if (diagonal) route = NW_ROUTE_EQUAL;
    if (diagonal && lane < N) {
      const bool match = ((mm >> lane) & 1ull) == 0ull;
      const int cur = __popcll(~mm & ((1ull << lane) - 1ull));  // matches before this column
      GS[lane] = match ? OGS[cur] : NONE;
      GE[lane] = match ? OGE[cur] : NONE;
    }
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
      if (lane < N) {
        const bool match = ((matched >> lane) & 1ull) != 0ull;
        const int cur = s_off + __popcll(matched & ((1ull << lane) - 1ull));
        GS[lane] = match ? OGS[cur] : NONE;
        GE[lane] = match ? OGE[cur] : NONE;
      }
    }
  }
  if (!diagonal) {
    // ---- fill, one matrix ROW per step (N steps instead of the N + M - 1 anti-diagonals of a
    // systolic sweep, which also idles half the lanes while it ramps up and down).  Lane j owns
    // column j and keeps F[i-1, j].  With c_j = max(F[i-1,j-1] + match, F[i-1,j] - 1) the row is
    //   F[i, j] = max(c_j, F[i, j-1] - 1) = max_{k <= j} (c_k + k) - j   (F[i,-1] = -i enters as k = -1)
    // i.e. a prefix maximum over the lanes: six DPP steps.  The pointer follows from the three
    // candidates with the reference's tie order UP (0,-1) > LEFT (-1,0) > DIAG.  Pointers stay in
    // registers: 2 bits per cell, word b of lane j = rows 16b .. 16b+15 of column j.
    int Fp = -lane;  // F[-1, j] = -j
    unsigned int ptrs[NWF_MAX_N / 16];
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
        int g = c + lane;
        const int ID = (int)0x80000000;
        g = max(g, __builtin_amdgcn_update_dpp(ID, g, 0x111, 0xf, 0xf, false));  // row_shr:1
        g = max(g, __builtin_amdgcn_update_dpp(ID, g, 0x112, 0xf, 0xf, false));  // row_shr:2
        g = max(g, __builtin_amdgcn_update_dpp(ID, g, 0x114, 0xf, 0xf, false));  // row_shr:4
        g = max(g, __builtin_amdgcn_update_dpp(ID, g, 0x118, 0xf, 0xf, false));  // row_shr:8
        g = max(g, __builtin_amdgcn_update_dpp(ID, g, 0x142, 0xa, 0xf, false));  // row_bcast:15
        g = max(g, __builtin_amdgcn_update_dpp(ID, g, 0x143, 0xc, 0xf, false));  // row_bcast:31
        const int Fc = max(g, -i - 1) - lane;  // F[i, j]
        // F[i, j-1] - 1: pointer UP = (0, -1); lane 0 takes the border F[i, -1] = -i
        const int s_u = __builtin_amdgcn_update_dpp(-i, Fc, 0x138, 0xf, 0xf, false) - 1;
        const unsigned int ptr = s_u >= c ? 2u : (s_l >= s_d ? 1u : 0u);
        acc |= ptr << ((i & 15) * 2);
        Fp = Fc;
      }
      ptrs[blk] = acc;
    }
    // ---- traceback on the scalar unit: i, j and the ops are wave-uniform, a pointer is one
    // v_readlane away (no LDS round trip per step).  Ops are collected back to front, 16 per word.
    int n_ops = 0;
    {
      int i = N - 1, j = M - 1;
      unsigned int pack = 0;
  #pragma unroll
      for (int blk = NWF_MAX_N / 16 - 1; blk >= 0; --blk) {
        while (i >= blk * 16 && j >= 0) {
          const unsigned int w = (unsigned int)__builtin_amdgcn_readlane((int)ptrs[blk], j);
          const unsigned int p = (w >> ((i & 15) * 2)) & 3u;
          pack |= p << ((n_ops & 15) * 2);
          if ((n_ops & 15) == 15) {
            if (lane == 0) OPW[n_ops >> 4] = pack;
            pack = 0;
          }
          ++n_ops;
          if (p == 0) { --i; --j; }
          else if (p == 1) --i;
          else --j;
        }
      }
      while (i >= 0) {  // leading corrected genes: LEFT
        pack |= 1u << ((n_ops & 15) * 2);
        if ((n_ops & 15) == 15) {
          if (lane == 0) OPW[n_ops >> 4] = pack;
          pack = 0;
        }
        ++n_ops;
        --i;
      }
      while (j >= 0) {  // leading original genes: UP
        pack |= 2u << ((n_ops & 15) * 2);
        if ((n_ops & 15) == 15) {
          if (lane == 0) OPW[n_ops >> 4] = pack;
          pack = 0;
        }
        ++n_ops;
        --j;
      }
      if ((n_ops & 15) != 0 && lane == 0) OPW[n_ops >> 4] = pack;
    }
    wave_sync();
    // ---- positions, in parallel over the alignment columns (front to back)
    int base_x = 0, base_y = 0, base_cur = 0;
    for (int c0 = 0; c0 < n_ops; c0 += 64) {
      const int f = c0 + lane;
      const bool in = f < n_ops;
      const int g = in ? n_ops - 1 - f : 0;
      const unsigned int op = in ? (OPW[g >> 4] >> ((g & 15) * 2)) & 3u : 3u;
      const bool isx = in && (op == 0 || op == 1), isy = in && (op == 0 || op == 2);
      const unsigned long long lt = (1ull << lane) - 1ull;
      const unsigned long long bx = __ballot(isx), by = __ballot(isy);
      const int xi = base_x + __popcll(bx & lt), yy = base_y + __popcll(by & lt);
      const int ysel = __shfl(yj, yy < 64 ? yy : 0, 64);  // all lanes take part in the shuffle
      const bool match = in && op == 0 && X[xi < NWF_MAX_N ? xi : 0] == ysel;
      const bool inc = in && (op == 2 || match);
      const unsigned long long bc = __ballot(inc);
      const int cur = base_cur + __popcll(bc & lt);
      if (isx) {
        GS[xi] = match ? OGS[cur < NWF_MAX_M ? cur : 0] : NONE;
        GE[xi] = match ? OGE[cur < NWF_MAX_M ? cur : 0] : NONE;
      }
      base_x += __popcll(bx);
      base_y += __popcll(by);
      base_cur += __popcll(bc);
    }
  }
  wave_sync();
  if (A.route && lane == 0) A.route[gi] = (unsigned char)route;
  // ---- replace_invalid_gene_positions, each lane repairs its own entries
  for (int q = lane; q < N; q += 64) {
    long long sv = GS[q], ev = GE[q];
    if (sv == NONE && ev == NONE) {
      long long prev_end = 0;
      for (int w = q - 1; w >= 0; --w)
        if (GE[w] != NONE) { prev_end = GE[w]; break; }
      long long nxt = NONE;
      for (int w = q + 1; w < N; ++w)
        if (GS[w] != NONE) { nxt = GS[w]; break; }
      sv = prev_end;
      ev = (nxt != NONE) ? nxt : rl - 1;
    }
    A.o_gs[pdst + q] = sv;
    A.o_ge[pdst + q] = ev;
  }
}

// (Sixteen lanes per read for the reads whose alignment is provably the diagonal — three reads in four — were built and
// measured in round 5: 0.27 ms for them plus 0.56 ms for the others against 0.575 ms for everybody here.  The pass IS
// the reads that fill a matrix, ~3 000 instructions each; the diagonal ones ride along for nothing.)
__global__ __launch_bounds__(64 * NWF_WPB) void k_corr_nw_fast(NwArgs A) {
  __shared__ NwfLds s_lds;
  if ((long long)blockIdx.x < A.n_gapped) nw_fast_read(A, (long long)blockIdx.x, (int)threadIdx.x, s_lds);
}

// global NW scratch size of gapped read gi (0 when it fits the LDS path)
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
  {
    // everything k_corr_nw_fast needs to start, in one 32-byte record (instead of a chain of
    // dependent per-read loads at the head of a latency-bound kernel)
    NwRec q;
    q.r = (int)r;
    q.M = (int)(M > 0x7fffffff ? 0x7fffffff : M);
    q.N = (final_cls[r] != RC_KEEP_ORIG && allow_fast && nw_fast_ok(N, M)) ? (int)N : 0;  // 0: not for the fast kernel
    q.pad = 0;
    q.t0 = read_off[r];
    q.dst = tmp_off[r];
    q.pdst = 0;  // k_nw_place
    q.poff = pos_off ? pos_off[r] : read_off[r];
    rec[gi] = q;
    plen[gi] = final_cls[r] != RC_KEEP_ORIG ? N : 0;  // new positions of this read
  }
  bool small = (N <= NW_LDS_N && M <= NW_LDS_N && N * M <= NW_LDS_CELLS);
  long long bytes = 0;
  if (!small && final_cls[r] != RC_KEEP_ORIG)
    bytes = ((N * M + N + M + 15) & ~15ll) + ((3 * (N + 1) * 4 + 15) & ~15ll);
  size[gi] = bytes;
  if (final_cls[r] != RC_KEEP_ORIG && !(allow_fast && nw_fast_ok(N, M))) atomicAdd(n_general, 1ull);
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
  {
    ClearList cl;
    cl.add(S.nw_size, (size_t)(n_gapped + 1) * sizeof(long long));
    cl.add(S.plen, (size_t)(n_gapped + 1) * sizeof(long long));
    cl.add(S.n_general, sizeof(unsigned long long));
    AMGCHK(clear_many(c, cl));
  }
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
  W.a = a;
  W.rec = c->nw_rec.as<NwRec>();
  W.o_gs = c->pos1_s.as<long long>();
  W.o_ge = c->pos1_e.as<long long>();
  W.gapped_reads = nullptr;  // the records carry the read ids
  W.n_gapped = n_gapped;
  W.final_cls = S.final_cls;
  W.big_off = S.nw_off;
  W.big_buf = c->nw_big.as<unsigned char>();
  W.allow_fast = sw.fast_nw;
  W.shortcuts = sw.nw_shortcuts;
  W.route = route;
  if (W.allow_fast)
    hipLaunchKernelGGL(k_corr_nw_fast, dim3((unsigned int)n_gapped), dim3(64 * NWF_WPB), 0, st, W);
  if (n.n_general > 0)  // reads too long for the register-resident kernel
    hipLaunchKernelGGL(k_corr_nw, dim3((unsigned int)n_gapped), dim3(64), 0, st, W);
  return AMG_OK;
}

// ------------------------------------------------------------------ amg_nw_probe (tests: one carry-over on host arrays)
// The context's position pools and what fill_pos_args reads of it, lent to the probe for one call: the probe's own
// arrays stand in, and the destructor frees them and puts the context back as it was.
struct NwProbeLoan {
  amg_ctx* c;
  DevBuf gene_start, gene_end, pos_off, pos1_s, pos1_e;
  bool have_pos, pos_identity;
  int64_t pos_n0, pos1_used;
  explicit NwProbeLoan(amg_ctx* ctx)
      : c(ctx), gene_start(ctx->gene_start), gene_end(ctx->gene_end), pos_off(ctx->pos_off), pos1_s(ctx->pos1_s),
        pos1_e(ctx->pos1_e), have_pos(ctx->have_pos), pos_identity(ctx->pos_identity), pos_n0(ctx->pos_n0),
        pos1_used(ctx->pos1_used) {
    c->gene_start = c->gene_end = c->pos_off = c->pos1_s = c->pos1_e = DevBuf();
  }
  ~NwProbeLoan() {
    c->gene_start.release(), c->gene_end.release(), c->pos_off.release(), c->pos1_s.release(), c->pos1_e.release();
    c->gene_start = gene_start, c->gene_end = gene_end, c->pos_off = pos_off, c->pos1_s = pos1_s, c->pos1_e = pos1_e;
    c->have_pos = have_pos, c->pos_identity = pos_identity, c->pos_n0 = pos_n0, c->pos1_used = pos1_used;
  }
};
// the probe's own device arrays
struct NwProbeBufs {
  DevBuf tokens, read_off, tmp_tok, tmp_off, new_len, final_cls, read_len, glist, sizes, places, route;
  ~NwProbeBufs() {
    for (DevBuf* b : {&tokens, &read_off, &tmp_tok, &tmp_off, &new_len, &final_cls, &read_len, &glist, &sizes, &places,
                      &route})
      b->release();
  }
};
static int probe_up(DevBuf& b, const void* src, size_t bytes, size_t room = 0) {
  AMGCHK(b.ensure(bytes + room + 16));
  if (bytes) HIPCHK(hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
  return AMG_OK;
}

#define NWP_GUARD 64      // guard words behind the produced positions and behind the staged genes
#define NWP_GUARD_PRE 8   // and in front of the produced positions
#define NWP_N0_POOLED 5   // entries of the caller's pool when the originals live in the pool of produced positions
extern "C" int amg_nw_probe(amg_ctx* c, int64_t n_pairs, const int32_t* x_tok, const int64_t* x_off, const int32_t* y_tok,
                            const int64_t* y_off, const int64_t* y_start, const int64_t* y_end, const int64_t* read_len,
                            const uint8_t* keep_orig, int flags, int64_t* out_start, int64_t* out_end, uint8_t* route,
                            int64_t* state) {
  if (!c || n_pairs < 1 || n_pairs > (1ll << 20) || !x_off || !y_tok || !y_off || !y_start || !y_end || !route || !state ||
      flags < 0 || flags > 7 || x_off[0] != 0 || y_off[0] != 0)
    return amg_fail(AMG_E_ARG, "nw_probe: bad arguments");
  // what the kernels cannot take is refused here: nothing is launched for it
  long long want_pos = 0, want_big = 0;
  for (int64_t p = 0; p < n_pairs; ++p) {
    const long long N = x_off[p + 1] - x_off[p], M = y_off[p + 1] - y_off[p];
    const bool keep = keep_orig && keep_orig[p];
    if (N < 0 || M < 1 || (N < 1 && !keep) || N > (1 << 24) || M > (1 << 24))
      return amg_fail(AMG_E_ARG, "nw_probe: pair %lld has %lld corrected and %lld original genes", (long long)p, N, M);
    if (keep) continue;
    want_pos += N;
    if (!(N <= NW_LDS_N && M <= NW_LDS_N && N * M <= NW_LDS_CELLS)) want_big += N * M + 16 * (N + M) + 64;
    if (want_big > (1ll << 30)) return amg_fail(AMG_E_ARG, "nw_probe: more than 1 GiB of matrix scratch");
  }
  const long long total_x = x_off[n_pairs], total_y = y_off[n_pairs];
  if (total_x > 0 && !x_tok) return amg_fail(AMG_E_ARG, "nw_probe: no corrected genes");
  if (want_pos > 0 && (!out_start || !out_end)) return amg_fail(AMG_E_ARG, "nw_probe: no room for the positions");
  for (long long i = 0; i < total_x; ++i)
    if (x_tok[i] < 0) return amg_fail(AMG_E_ARG, "nw_probe: negative corrected gene at %lld", i);
  for (long long i = 0; i < total_y; ++i)
    if (y_tok[i] < 0) return amg_fail(AMG_E_ARG, "nw_probe: negative original gene at %lld", i);
  HIPCHK(hipSetDevice(c->device));

  const bool pooled = (flags & 4) != 0;
  NwProbeLoan loan(c);
  NwProbeBufs B;
  CorrSwitches sw = {};
  sw.fast_nw = (flags & 1) ? 0 : 1;
  sw.nw_shortcuts = (flags & 2) ? 0 : 1;
  // ---- the read set, the staged genes and the classes, as amg_correct_reads has them before its shape step
  std::vector<unsigned int> new_len((size_t)n_pairs);
  std::vector<unsigned char> cls((size_t)n_pairs);
  std::vector<int> glist((size_t)n_pairs);
  for (int64_t p = 0; p < n_pairs; ++p) {
    new_len[p] = (unsigned int)(x_off[p + 1] - x_off[p]);
    cls[p] = (keep_orig && keep_orig[p]) ? RC_KEEP_ORIG : RC_GAPPED;
    glist[p] = (int)p;
  }
  const size_t np1 = (size_t)n_pairs + 1;
  AMGCHK(probe_up(B.tokens, y_tok, (size_t)total_y * 4));
  AMGCHK(probe_up(B.read_off, y_off, np1 * 8));
  AMGCHK(probe_up(B.tmp_tok, x_tok, (size_t)total_x * 4, NWP_GUARD * 4));
  HIPCHK(hipMemset(B.tmp_tok.as<int>() + total_x, 0xff, NWP_GUARD * 4));
  AMGCHK(probe_up(B.tmp_off, x_off, np1 * 8));
  AMGCHK(probe_up(B.new_len, new_len.data(), (size_t)n_pairs * 4));
  AMGCHK(probe_up(B.final_cls, cls.data(), (size_t)n_pairs));
  if (read_len) AMGCHK(probe_up(B.read_len, read_len, (size_t)n_pairs * 8));
  AMGCHK(probe_up(B.glist, glist.data(), (size_t)n_pairs * 4));
  AMGCHK(B.sizes.ensure((n_pairs + 2) * 2 * sizeof(long long)));
  AMGCHK(B.places.ensure((n_pairs + 2) * 3 * sizeof(long long)));
  AMGCHK(B.route.ensure((size_t)n_pairs + 16));
  HIPCHK(hipMemset(B.route.p, 0, (size_t)n_pairs));
  // ---- the positions of the original genes: the caller's pool, or the pool of produced positions with NWP_GUARD_PRE
  // guard words behind them; that pool is allocated for what it holds and no more, so that this call's products have
  // grow_keep move it (state[4] says whether it did)
  const long long used = (pooled ? total_y : 0) + NWP_GUARD_PRE;
  {
    std::vector<long long> ps((size_t)used, -1ll), pe((size_t)used, -1ll);
    if (pooled) {
      memcpy(ps.data(), y_start, (size_t)total_y * 8);
      memcpy(pe.data(), y_end, (size_t)total_y * 8);
      const long long filler[NWP_N0_POOLED] = {-1, -1, -1, -1, -1};
      std::vector<long long> off((size_t)n_pairs);
      for (int64_t p = 0; p < n_pairs; ++p) off[p] = NWP_N0_POOLED + y_off[p];
      AMGCHK(probe_up(c->gene_start, filler, sizeof(filler)));
      AMGCHK(probe_up(c->gene_end, filler, sizeof(filler)));
      AMGCHK(probe_up(c->pos_off, off.data(), (size_t)n_pairs * 8));
    } else {
      AMGCHK(probe_up(c->gene_start, y_start, (size_t)total_y * 8));
      AMGCHK(probe_up(c->gene_end, y_end, (size_t)total_y * 8));
    }
    AMGCHK(c->pos1_s.ensure((size_t)used * 8));
    AMGCHK(c->pos1_e.ensure((size_t)used * 8));
    HIPCHK(hipMemcpy(c->pos1_s.p, ps.data(), (size_t)used * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(c->pos1_e.p, pe.data(), (size_t)used * 8, hipMemcpyHostToDevice));
  }
  c->have_pos = true;
  c->pos_identity = !pooled;
  c->pos_n0 = pooled ? NWP_N0_POOLED : total_y;
  c->pos1_used = used;
  HIPCHK(hipDeviceSynchronize());

  CorrScratch S;
  S.per_read = (size_t)n_pairs + 2;
  S.final_cls = B.final_cls.as<unsigned char>();
  S.nw_size = B.sizes.as<long long>();
  S.nw_off = S.nw_size + (n_pairs + 2);
  S.new_len = B.new_len.as<unsigned int>();
  S.tmp_off = B.tmp_off.as<long long>();
  S.tmp_tok = B.tmp_tok.as<int>();
  S.plen = B.places.as<long long>();
  S.poffs = S.plen + (n_pairs + 2);
  S.pos_new = S.poffs + (n_pairs + 2);
  S.n_general = c->status.as<unsigned long long>() + ST_MISC;
  S.glist = &B.glist;
  CorrArgs a;
  memset(&a, 0, sizeof(a));
  a.tokens = B.tokens.as<int>();
  a.read_off = B.read_off.as<long long>();
  fill_pos_args(c, a);
  a.read_len = read_len ? B.read_len.as<long long>() : nullptr;
  a.n_reads = n_pairs;
  a.have_pos = 1;
  a.cls_final = S.final_cls;
  a.tmp_off = S.tmp_off;
  a.new_len = S.new_len;
  a.tmp_tok = S.tmp_tok;
  // ---- the shape step's part, the pools, the kernels: the calls amg_correct_reads makes
  CorrCounts n;
  n.n_gapped = n_pairs;
  n.carry = true;
  FetchList shape;
  AMGCHK(corr_nw_sizes(c, sw, S, a, n_pairs, shape));
  unsigned long long v[3] = {0, 0, 0};
  AMGCHK(fetch(c, shape, v));
  n.big_total = (long long)v[0];
  n.pos_total = (long long)v[1];
  n.n_general = v[2];
  const void* pool_before = c->pos1_s.p;
  AMGCHK(corr_grow_pos_pools(c, n));
  fill_pos_args(c, a);
  const long long span = n.pos_total + NWP_GUARD;  // corr_grow_pos_pools leaves 64 entries behind the products
  HIPCHK(hipMemsetAsync(c->pos1_s.as<long long>() + used, 0xff, (size_t)span * 8, c->stream));
  HIPCHK(hipMemsetAsync(c->pos1_e.as<long long>() + used, 0xff, (size_t)span * 8, c->stream));
  AMGCHK(corr_positions(c, sw, S, a, n, B.route.as<unsigned char>()));
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));

  // ---- what came of it
  std::vector<long long> gs((size_t)(used + span)), ge((size_t)(used + span)), nw_size((size_t)n_pairs);
  std::vector<NwRec> rec((size_t)n_pairs);
  std::vector<int> tail(NWP_GUARD);
  HIPCHK(hipMemcpy(gs.data(), c->pos1_s.p, gs.size() * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(ge.data(), c->pos1_e.p, ge.size() * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(nw_size.data(), S.nw_size, (size_t)n_pairs * 8, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(rec.data(), c->nw_rec.p, (size_t)n_pairs * sizeof(NwRec), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(route, B.route.p, (size_t)n_pairs, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(tail.data(), B.tmp_tok.as<int>() + total_x, NWP_GUARD * 4, hipMemcpyDeviceToHost));
  bool intact = true;
  for (long long i = 0; i < used; ++i) {
    const bool orig = pooled && i < total_y;
    if (gs[i] != (orig ? y_start[i] : -1ll) || ge[i] != (orig ? y_end[i] : -1ll)) intact = false;
  }
  for (long long i = used + n.pos_total; i < used + span; ++i)
    if (gs[i] != -1ll || ge[i] != -1ll) intact = false;
  for (int i = 0; i < NWP_GUARD; ++i)
    if (tail[i] != -1) intact = false;
  const long long take = n.pos_total < want_pos ? n.pos_total : want_pos;
  if (take > 0) {
    memcpy(out_start, gs.data() + used, (size_t)take * 8);
    memcpy(out_end, ge.data() + used, (size_t)take * 8);
  }
  for (int64_t p = 0; p < n_pairs; ++p)  // the general kernel's pairs: by the record and the size k_nw_sizes made
    if (cls[p] != RC_KEEP_ORIG && rec[p].N == 0) route[p] = nw_size[p] > 0 ? NW_ROUTE_GLOBAL : NW_ROUTE_LDS;
  state[0] = n.big_total;
  state[1] = n.pos_total;
  state[2] = (int64_t)n.n_general;
  state[3] = intact ? 1 : 0;
  state[4] = c->pos1_s.p != pool_before ? 1 : 0;
  return AMG_OK;
}
