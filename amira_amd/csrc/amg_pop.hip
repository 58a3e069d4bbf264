// amg_pop.hip — bubble popping's last step on the device: the reads of all correction operations of one
// correct_bubble_paths call rewritten in one go (reference construct_graph.py:1833-1955 with its helpers :1577-1751,
// :1977-2014; the pinned restatement is oracle/amira_oracle/bubbles.py:243-360).
//
//   k_pop_plan      a wave per operation: needleman_wunsch(better, worse) (:1433-1480 — match 1, mismatch 0, gap -1,
//                   borders -index, the best of (score, pointer) with DIAG < LEFT < UP, so a tie goes UP, then LEFT:
//                   amg_nw_align's recurrence and traceback), the veto of an operation that would delete a gene of
//                   interest (:1880-1884), and for every gene-mer of `worse` whether it is the first of its kind.
//   k_pop_rewrite   a wave per read: the orientation vote over DISTINCT gene-mers (:1591-1612), the first longest run
//                   the read shares with the worse side of the chosen alignment (:1992-2014), the second alignment
//                   where the better genes of that stretch are not the read's (:1731-1735), the spliced genes (:1616-1628)
//                   and, per gene, the index of the old read whose position it keeps (:1641-1667) — into the read's own
//                   stretch of a staging buffer.
//   k_pop_pack      the rewritten reads packed in read order behind the scan of their lengths.
//
// The alignment is filled an anti-diagonal at a time: every cell is the reference's own three-way comparison, so the tie
// order needs no argument.  The matrix is at most 128 x 128: the pointer bytes and three anti-diagonals of scores live in
// LDS.  Every block is one wave.
//
// What the admitted sizes cost.  The call is made for bubble popping's sizes: a few thousand operations of at most
// 64 + k - 1 genes and reads of some dozens of genes.  The entry point admits far more (2^20 operations, reads of 2^24
// genes) and stays correct there, but not cheap: a PopPlan is 2.2 KB, so 2^20 operations ask for 2.2 GB of plans (a
// failed allocation is AMG_E_NOMEM, nothing else happens), and one wave walks its whole read: per 64 windows of the read
// two ballots and up to k compares for each distinct gene-mer of the path (the vote), then one row step per gene of the
// path (the run) — about 126 x 2 ballots x 262 k chunks for a read of 2^24 genes, seconds of one wave.
#include "amg_internal.h"

#define POP_MAX 128          // genes of a better / worse list
#define POP_COLS (2 * POP_MAX)  // columns of an alignment of two such lists
#define POP_GAP (-1)         // "*"
#define POP_DIAG_STRIDE (POP_MAX + 2)
#define POP_MAX_READ (1ll << 24)
#define POP_MAX_ITEMS (1ll << 20)

struct PopPlan {
  int ncol, veto;
  int hi[POP_COLS], lo[POP_COLS];   // the columns of needleman_wunsch(better, worse): (better gene, worse gene)
  unsigned char first[POP_MAX];     // gene-mer w of worse is the first of its kind
};

// grow-only page-locked host memory: a copy to or from it is one DMA transfer the stream orders (a copy from pageable
// memory is staged by the runtime, which may wait on its own)
struct PopPinned {
  unsigned char* p = nullptr;
  size_t cap = 0;
  int ensure(size_t bytes) {
    if (bytes <= cap) return AMG_OK;
    release();
    const size_t want = bytes + bytes / 8 + 256;
    hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&p), want, hipHostMallocDefault);
    if (e != hipSuccess) {
      p = nullptr;
      return amg_fail(AMG_E_NOMEM, "hipHostMalloc(%zu) failed: %s", want, hipGetErrorString(e));
    }
    cap = want;
    return AMG_OK;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
};

struct PopState {
  DevBuf in, out, plans, len, stage_tok, stage_src;
  PopPinned host_in, host_out;  // what travels, as one block each way
};

void pop_release(amg_ctx* c) {
  if (!c->pop) return;
  PopState* s = c->pop;
  DevBuf* all[] = {&s->in, &s->out, &s->plans, &s->len, &s->stage_tok, &s->stage_src};
  for (DevBuf* d : all) d->release();
  s->host_in.release();
  s->host_out.release();
  delete s;
  c->pop = nullptr;
}

// what one wave's alignment needs in LDS
struct PopNwLds {
  int x[POP_MAX], y[POP_MAX];
  int diag[3 * POP_DIAG_STRIDE];
  unsigned char ptr[POP_MAX * POP_MAX];
};

// needleman_wunsch(x[0..n), y[0..m)) by the whole wave (the block): the columns, front to back, into colh / coll
// (POP_COLS each, LDS); returns their number.  n, m <= POP_MAX; either may be 0.
__device__ int pop_nw(PopNwLds& s, int n, int m, int* colh, int* coll, int lane) {
  __shared__ int s_ncol;
  __syncthreads();  // (x and y are written)
  for (int d = 0; n > 0 && m > 0 && d <= n + m - 2; ++d) {
    int* cur = s.diag + (d % 3) * POP_DIAG_STRIDE;                // F[i, d - i] at [i]
    const int* p1 = s.diag + ((d + 2) % 3) * POP_DIAG_STRIDE;     // anti-diagonal d - 1
    const int* p2 = s.diag + ((d + 1) % 3) * POP_DIAG_STRIDE;     // anti-diagonal d - 2
    for (int i = lane; i < n; i += 64) {
      const int j = d - i;
      if (j < 0 || j >= m) continue;
      // the reference's borders: F[i, -1] = -i, F[-1, j] = -j, F[-1, -1] = 0
      const int f_diag = i == 0 ? (j == 0 ? 0 : -(j - 1)) : (j == 0 ? -(i - 1) : p2[i - 1]);
      const int f_left = i == 0 ? -j : p1[i - 1];   // F[i - 1, j]: a gene of x against a gap
      const int f_up = j == 0 ? -i : p1[i];         // F[i, j - 1]: a gene of y against a gap
      int best = f_diag + (s.x[i] == s.y[j] ? 1 : 0);
      unsigned char p = 0;
      if (f_left - 1 >= best) { best = f_left - 1; p = 1; }
      if (f_up - 1 >= best) { best = f_up - 1; p = 2; }
      cur[i] = best;
      s.ptr[i * POP_MAX + j] = p;
    }
    __syncthreads();
  }
  if (lane == 0) {  // the traceback, back to front into the end of the column arrays
    int i = n - 1, j = m - 1, at = POP_COLS;
    while (i >= 0 && j >= 0) {
      const unsigned char p = s.ptr[i * POP_MAX + j];
      --at;
      colh[at] = p == 2 ? POP_GAP : s.x[i];
      coll[at] = p == 1 ? POP_GAP : s.y[j];
      if (p == 0) { --i; --j; } else if (p == 1) { --i; } else { --j; }
    }
    for (; i >= 0; --i) { --at; colh[at] = s.x[i]; coll[at] = POP_GAP; }
    for (; j >= 0; --j) { --at; colh[at] = POP_GAP; coll[at] = s.y[j]; }
    s_ncol = POP_COLS - at;
  }
  __syncthreads();
  const int ncol = s_ncol, from = POP_COLS - ncol;
  int h[POP_COLS / 64], l[POP_COLS / 64];
#pragma unroll
  for (int q = 0; q < POP_COLS / 64; ++q) {
    const int cc = lane + 64 * q;
    h[q] = cc < ncol ? colh[from + cc] : POP_GAP;
    l[q] = cc < ncol ? coll[from + cc] : POP_GAP;
  }
  __syncthreads();
#pragma unroll
  for (int q = 0; q < POP_COLS / 64; ++q) {
    const int cc = lane + 64 * q;
    if (cc < ncol) { colh[cc] = h[q]; coll[cc] = l[q]; }
  }
  __syncthreads();
  return ncol;
}

__global__ __launch_bounds__(64) void k_pop_plan(int k, const int* __restrict__ better_tok, const long long* __restrict__ better_off,
                                                 const int* __restrict__ worse_tok, const long long* __restrict__ worse_off,
                                                 const unsigned char* __restrict__ interest, PopPlan* __restrict__ plans,
                                                 unsigned char* __restrict__ veto) {
  __shared__ PopNwLds s;
  __shared__ int colh[POP_COLS], coll[POP_COLS];
  const int lane = threadIdx.x;
  const long long op = blockIdx.x;
  const long long b0 = better_off[op], w0 = worse_off[op];
  const int n = (int)(better_off[op + 1] - b0), m = (int)(worse_off[op + 1] - w0);
  for (int i = lane; i < n; i += 64) s.x[i] = better_tok[b0 + i];
  for (int j = lane; j < m; j += 64) s.y[j] = worse_tok[w0 + j];
  const int ncol = pop_nw(s, n, m, colh, coll, lane);
  PopPlan& plan = plans[op];
  bool bad = false;
  for (int cc = lane; cc < ncol; cc += 64) {
    const int h = colh[cc], l = coll[cc];
    plan.hi[cc] = h;
    plan.lo[cc] = l;
    // a gene of interest on the worse path against a gap or a gene that is none: the correction would delete it
    if (interest && l != POP_GAP && interest[l] && (h == POP_GAP || !interest[h])) bad = true;
  }
  const int vetoed = __any(bad) ? 1 : 0;
  // gene-mer w of worse (s.y) is the first of its kind
  for (int w = lane; w < m - k + 1; w += 64) {
    bool first = true;
    for (int u = 0; u < w && first; ++u) {
      bool same = true;
      for (int t = 0; t < k; ++t) same = same && s.y[u + t] == s.y[w + t];
      first = !same;
    }
    plan.first[w] = first ? 1 : 0;
  }
  if (lane == 0) {
    plan.ncol = ncol;
    plan.veto = vetoed;
    veto[op] = (unsigned char)vetoed;
  }
}

__device__ __forceinline__ unsigned long long pop_wave_max(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = (unsigned long long)__shfl_xor((long long)v, o);
    v = other > v ? other : v;
  }
  return v;
}

// status: 0 the operation is vetoed, 1 the orientation vote is a tie, 2 rewritten
__global__ __launch_bounds__(64) void k_pop_rewrite(int k, int flip, const PopPlan* __restrict__ plans,
                                                    const int* __restrict__ worse_tok, const long long* __restrict__ worse_off,
                                                    const int* __restrict__ read_tok, const long long* __restrict__ read_off,
                                                    const int* __restrict__ read_op, const long long* __restrict__ stage_off,
                                                    unsigned char* __restrict__ status, int* __restrict__ first_shared,
                                                    int* __restrict__ last_shared, long long* __restrict__ out_len,
                                                    int* __restrict__ stage_tok, int* __restrict__ stage_src) {
  __shared__ PopNwLds s;
  __shared__ int colh[POP_COLS], coll[POP_COLS];   // the operation's alignment as this read looks at it
  __shared__ int c2h[POP_COLS], c2l[POP_COLS];     // the second alignment
  __shared__ int worse[POP_MAX];                   // its worse side without the gaps ...
  __shared__ int col_of[POP_MAX];                  // ... and the column of every gene of it
  __shared__ int mers[POP_MAX];                    // the worse path's own genes (the vote)
  __shared__ unsigned char first[POP_MAX];
  __shared__ int carry[2][POP_MAX];                // run[i][last index of the previous chunk of the read]
  const int lane = threadIdx.x;
  const long long r = blockIdx.x;
  const int op = read_op[r];
  const PopPlan& plan = plans[op];
  const long long r0 = read_off[r];
  const int L = (int)(read_off[r + 1] - r0);
  const int* read = read_tok + r0;
  if (lane == 0) {
    first_shared[r] = -1;
    last_shared[r] = -1;
    out_len[r] = 0;
  }
  if (plan.veto) {
    if (lane == 0) status[r] = 0;
    return;
  }
  const int ncol = plan.ncol;
  const int m = (int)(worse_off[op + 1] - worse_off[op]);
  const int nw = m - k + 1;
  for (int j = lane; j < m; j += 64) mers[j] = worse_tok[worse_off[op] + j];
  for (int w = lane; w < nw; w += 64) first[w] = plan.first[w];
  __syncthreads();
  // ---- orientation: the distinct gene-mers of the read among those of worse, read forward and mirrored.  A gene-mer
  // both lists hold is one of worse's distinct gene-mers that the read holds: count those.
  unsigned long long seen_fw[2] = {0ull, 0ull}, seen_rv[2] = {0ull, 0ull};
  for (int i0 = 0; i0 < L - k + 1; i0 += 64) {
    const int i = i0 + lane;
    const bool live = i < L - k + 1;
    int mine[AMG_MAX_K];
#pragma unroll
    for (int t = 0; t < AMG_MAX_K; ++t) mine[t] = (live && t < k) ? read[i + t] : 0;
    for (int w = 0; w < nw; ++w) {
      if (!first[w]) continue;
      bool fw = live, rv = live;
#pragma unroll
      for (int t = 0; t < AMG_MAX_K; ++t)
        if (t < k) {
          fw = fw && mine[t] == mers[w + t];
          rv = rv && mine[t] == flip - mers[w + k - 1 - t];
        }
      if (__any(fw)) seen_fw[w >> 6] |= 1ull << (w & 63);
      if (__any(rv)) seen_rv[w >> 6] |= 1ull << (w & 63);
    }
  }
  const int fw_count = __popcll(seen_fw[0]) + __popcll(seen_fw[1]);
  const int rv_count = __popcll(seen_rv[0]) + __popcll(seen_rv[1]);
  if (fw_count == rv_count) {
    if (lane == 0) status[r] = 1;
    return;
  }
  const bool mirrored = rv_count > fw_count;
  for (int cc = lane; cc < ncol; cc += 64) {
    const int from = mirrored ? ncol - 1 - cc : cc;
    const int h = plan.hi[from], l = plan.lo[from];
    colh[cc] = (mirrored && h != POP_GAP) ? flip - h : h;
    coll[cc] = (mirrored && l != POP_GAP) ? flip - l : l;
  }
  __syncthreads();
  {
    int base = 0;
    for (int c0 = 0; c0 < ncol; c0 += 64) {
      const int cc = c0 + lane;
      const int l = cc < ncol ? coll[cc] : POP_GAP;
      const unsigned long long has = __ballot(l != POP_GAP);
      if (l != POP_GAP) {
        const int at = base + __popcll(has & ((1ull << lane) - 1ull));
        worse[at] = l;
        col_of[at] = cc;
      }
      base += __popcll(has);
    }
  }
  for (int i = lane; i < POP_MAX; i += 64) carry[0][i] = 0;
  __syncthreads();
  // ---- the first longest common run in (i, j) order: run[i][j] = worse[i] == read[j] ? run[i - 1][j - 1] + 1 : 0,
  // lanes over j, rows over i.  key = length, then the smaller i, then the smaller j.
  unsigned long long best = 0;
  int chunk = 0;
  for (int j0 = 0; j0 < L; j0 += 64, ++chunk) {
    const int j = j0 + lane;
    const int mine = j < L ? read[j] : POP_GAP;
    const int* from_left = carry[chunk & 1];
    int* to_right = carry[(chunk + 1) & 1];
    int run = 0;  // run[i - 1][j]
    for (int i = 0; i < m; ++i) {
      int diag = __shfl_up(run, 1);
      if (lane == 0) diag = i > 0 ? from_left[i - 1] : 0;
      run = (j < L && mine == worse[i]) ? diag + 1 : 0;
      if (lane == 63) to_right[i] = run;
      const unsigned long long key = ((unsigned long long)run << 40) | ((unsigned long long)(255 - i) << 32) |
                                     (unsigned long long)(0xffffffffu - (unsigned int)j);
      if (run > 0 && key > best) best = key;
    }
    __syncthreads();
  }
  best = pop_wave_max(best);
  const int run_len = (int)(best >> 40);
  if (run_len == 0) {  // (a shared gene-mer is a run of k: not reached)
    if (lane == 0) status[r] = 1;
    return;
  }
  const int end_i = 255 - (int)((best >> 32) & 0xff);
  const int end_j = (int)(0xffffffffu - (unsigned int)(best & 0xffffffffull));
  const int first_j = end_j + 1 - run_len, last_j = end_j;
  const int col_a = col_of[end_i + 1 - run_len], col_b = col_of[end_i];
  // ---- the better genes of that stretch of the alignment: the read's own genes there?
  int n_true = 0;
  bool same = true;
  for (int c0 = col_a; c0 <= col_b; c0 += 64) {
    const int cc = c0 + lane;
    const int h = cc <= col_b ? colh[cc] : POP_GAP;
    const unsigned long long has = __ballot(h != POP_GAP);
    if (h != POP_GAP) {
      const int at = n_true + __popcll(has & ((1ull << lane) - 1ull));
      s.x[at] = h;
      if (at >= run_len || read[first_j + at] != h) same = false;
    }
    n_true += __popcll(has);
  }
  same = !__any(!same) && n_true == run_len;
  const int *sub_h, *sub_l;
  int n_sub;
  if (same) {
    sub_h = colh + col_a;
    sub_l = coll + col_a;
    n_sub = col_b - col_a + 1;
  } else {
    for (int j = lane; j < run_len; j += 64) s.y[j] = read[first_j + j];
    n_sub = pop_nw(s, n_true, run_len, c2h, c2l, lane);
    sub_h = c2h;
    sub_l = c2l;
  }
  // ---- prefix + better genes of the stretch + suffix; every gene with the index of the old read whose position it
  // keeps: a column without a better gene and a column of equal genes use one up, a column of two different genes
  // yields -1 and uses none (get_new_gene_position_core)
  int* o_tok = stage_tok + stage_off[r];
  int* o_src = stage_src + stage_off[r];
  for (int i = lane; i < first_j; i += 64) {
    o_tok[i] = read[i];
    o_src[i] = i;
  }
  int n_core = 0, used = 0;
  for (int c0 = 0; c0 < n_sub; c0 += 64) {
    const int cc = c0 + lane;
    const bool live = cc < n_sub;
    const int h = live ? sub_h[cc] : POP_GAP, l = live ? sub_l[cc] : POP_GAP;
    const bool emits = live && h != POP_GAP;
    const bool uses = live && (h == POP_GAP || l == h);
    const unsigned long long em = __ballot(emits), us = __ballot(uses);
    const unsigned long long below = (1ull << lane) - 1ull;
    if (emits) {
      const int at = first_j + n_core + __popcll(em & below);
      o_tok[at] = h;
      o_src[at] = l == h ? first_j + used + __popcll(us & below) : -1;
    }
    n_core += __popcll(em);
    used += __popcll(us);
  }
  const int tail = L - 1 - last_j;
  for (int i = lane; i < tail; i += 64) {
    o_tok[first_j + n_core + i] = read[last_j + 1 + i];
    o_src[first_j + n_core + i] = last_j + 1 + i;
  }
  if (lane == 0) {
    status[r] = 2;
    first_shared[r] = first_j;
    last_shared[r] = last_j;
    out_len[r] = first_j + n_core + tail;
  }
}

__global__ __launch_bounds__(64) void k_pop_pack(const long long* __restrict__ out_len, const long long* __restrict__ out_off,
                                                 const long long* __restrict__ stage_off, const int* __restrict__ stage_tok,
                                                 const int* __restrict__ stage_src, int* __restrict__ out_tok,
                                                 int* __restrict__ out_src) {
  const long long r = blockIdx.x;
  const long long n = out_len[r], from = stage_off[r], to = out_off[r];
  for (long long i = threadIdx.x; i < n; i += 64) {
    out_tok[to + i] = stage_tok[from + i];
    out_src[to + i] = stage_src[from + i];
  }
}

static int pop_check_lists(const char* what, int32_t k, int32_t two_v, int64_t n_ops, const int32_t* tok, const int64_t* off) {
  if (!off || off[0] != 0) return amg_fail(AMG_E_ARG, "%s: bad offsets", what);
  for (int64_t o = 0; o < n_ops; ++o) {
    const int64_t n = off[o + 1] - off[o];
    if (n > POP_MAX) return amg_fail(AMG_E_ARG, "%s list %lld has %lld genes: at most %d", what, (long long)o, (long long)n, POP_MAX);
    if (n < k) return amg_fail(AMG_E_ARG, "%s list %lld has %lld genes: fewer than k", what, (long long)o, (long long)n);
  }
  if (off[n_ops] > 0 && !tok) return amg_fail(AMG_E_ARG, "%s: null tokens", what);
  for (int64_t i = 0; i < off[n_ops]; ++i)
    if (tok[i] < 0 || tok[i] >= two_v) return amg_fail(AMG_E_ARG, "%s: token %d outside [0, two_v)", what, tok[i]);
  return AMG_OK;
}

extern "C" int amg_pop_rewrite(amg_ctx* c, int32_t k, int32_t two_v, int64_t n_ops, const int32_t* better_tok,
                               const int64_t* better_off, const int32_t* worse_tok, const int64_t* worse_off,
                               const uint8_t* interest, int64_t n_reads, const int32_t* read_tok, const int64_t* read_off,
                               const int32_t* read_op, int64_t cap, uint8_t* op_veto, uint8_t* status, int32_t* first_shared,
                               int32_t* last_shared, int64_t* out_off, int32_t* out_tok, int32_t* out_src, int64_t* n_out) {
  if (!c) return amg_fail(AMG_E_ARG, "null ctx");
  if (k < 1 || k > AMG_MAX_K) return amg_fail(AMG_E_ARG, "k must be in [1, %d]", AMG_MAX_K);
  if (two_v <= 0 || (two_v & 1)) return amg_fail(AMG_E_ARG, "two_v must be a positive even number");
  if (n_ops < 1 || n_ops > POP_MAX_ITEMS) return amg_fail(AMG_E_ARG, "n_ops must be in [1, 2^20]");
  if (n_reads < 1 || n_reads > POP_MAX_ITEMS) return amg_fail(AMG_E_ARG, "n_reads must be in [1, 2^20]");
  if (!read_off || !read_op || !op_veto || !status || !first_shared || !last_shared || !out_off || !n_out)
    return amg_fail(AMG_E_ARG, "bad argument");
  AMGCHK(pop_check_lists("better", k, two_v, n_ops, better_tok, better_off));
  AMGCHK(pop_check_lists("worse", k, two_v, n_ops, worse_tok, worse_off));
  if (read_off[0] != 0) return amg_fail(AMG_E_ARG, "read_off[0] must be 0");
  std::vector<long long> stage_off((size_t)n_reads + 1);
  long long need = 0;
  for (int64_t r = 0; r < n_reads; ++r) {
    const int64_t len = read_off[r + 1] - read_off[r];
    if (len < 0) return amg_fail(AMG_E_ARG, "read_off not monotone at read %lld", (long long)r);
    if (len > POP_MAX_READ) return amg_fail(AMG_E_ARG, "read %lld has %lld genes: at most 2^24", (long long)r, (long long)len);
    if (read_op[r] < 0 || read_op[r] >= n_ops) return amg_fail(AMG_E_ARG, "read %lld names operation %d", (long long)r, read_op[r]);
    stage_off[(size_t)r] = need;
    need += len + (better_off[read_op[r] + 1] - better_off[read_op[r]]);
  }
  stage_off[(size_t)n_reads] = need;
  const long long T = read_off[n_reads];
  if (T > 0 && !read_tok) return amg_fail(AMG_E_ARG, "null read tokens");
  for (long long i = 0; i < T; ++i)
    if (read_tok[i] < 0 || read_tok[i] >= two_v) return amg_fail(AMG_E_ARG, "read token %d outside [0, two_v)", read_tok[i]);
  if (cap < need) return amg_fail(AMG_E_ARG, "cap %lld below the sum of read and better lengths %lld", (long long)cap, need);
  if (need > 0 && (!out_tok || !out_src)) return amg_fail(AMG_E_ARG, "null out_tok / out_src");
  HIPCHK(hipSetDevice(c->device));
  if (!c->pop) c->pop = new PopState();
  PopState* s = c->pop;
  hipStream_t st = c->stream;
  const long long NB = better_off[n_ops], NW = worse_off[n_ops];
  stages_reset(c);
  stage_begin(c, "pop_rewrite");
  // one block in, one block out: 8-byte items first, then 4-byte items, then bytes
  const size_t n8_in = 2 * ((size_t)n_ops + 1) + 2 * ((size_t)n_reads + 1);
  const size_t n4_in = (size_t)NB + (size_t)NW + (size_t)T + (size_t)n_reads;
  const size_t n1_in = interest ? (size_t)two_v : 0;
  const size_t in_bytes = n8_in * 8 + n4_in * 4 + n1_in;
  AMGCHK(s->host_in.ensure(in_bytes + 8));
  unsigned char* hin = s->host_in.p;
  AMGCHK(s->in.ensure(in_bytes + 8));
  unsigned char* din = s->in.as<unsigned char>();
  size_t at = 0;
  auto put = [&](const void* src, size_t bytes) -> const void* {
    if (bytes) memcpy(hin + at, src, bytes);
    const void* d = din + at;
    at += bytes;
    return d;
  };
  const long long* d_better_off = (const long long*)put(better_off, ((size_t)n_ops + 1) * 8);
  const long long* d_worse_off = (const long long*)put(worse_off, ((size_t)n_ops + 1) * 8);
  const long long* d_read_off = (const long long*)put(read_off, ((size_t)n_reads + 1) * 8);
  const long long* d_stage_off = (const long long*)put(stage_off.data(), ((size_t)n_reads + 1) * 8);
  const int* d_better_tok = (const int*)put(better_tok, (size_t)NB * 4);
  const int* d_worse_tok = (const int*)put(worse_tok, (size_t)NW * 4);
  const int* d_read_tok = (const int*)put(read_tok, (size_t)T * 4);
  const int* d_read_op = (const int*)put(read_op, (size_t)n_reads * 4);
  const unsigned char* d_interest = interest ? (const unsigned char*)put(interest, (size_t)two_v) : nullptr;
  HIPCHK(hipMemcpyAsync(din, hin, at, hipMemcpyHostToDevice, st));
  // out: out_off [n_reads + 1] | first, last [n_reads], tok, src [need] | status [n_reads], veto [n_ops]
  const size_t out_bytes = ((size_t)n_reads + 1) * 8 + (2 * (size_t)n_reads + 2 * (size_t)need) * 4 + (size_t)n_reads + (size_t)n_ops;
  AMGCHK(s->out.ensure(out_bytes + 8));
  AMGCHK(s->host_out.ensure(out_bytes + 8));
  unsigned char* dout = s->out.as<unsigned char>();
  size_t o_at = 0;
  auto take = [&](size_t bytes) -> size_t {
    const size_t was = o_at;
    o_at += bytes;
    return was;
  };
  const size_t o_off = take(((size_t)n_reads + 1) * 8), o_first = take((size_t)n_reads * 4), o_last = take((size_t)n_reads * 4);
  const size_t o_tok = take((size_t)need * 4), o_src = take((size_t)need * 4), o_status = take((size_t)n_reads);
  const size_t o_veto = take((size_t)n_ops);
  AMGCHK(s->plans.ensure((size_t)n_ops * sizeof(PopPlan)));
  AMGCHK(s->len.ensure((size_t)(n_reads + 2) * sizeof(long long)));
  AMGCHK(s->stage_tok.ensure((size_t)(need + 1) * sizeof(int)));
  AMGCHK(s->stage_src.ensure((size_t)(need + 1) * sizeof(int)));
  {
    ClearList cl;  // (the scan reads one length past the reads)
    cl.add(s->len.as<long long>() + n_reads, sizeof(long long));
    AMGCHK(clear_many(c, cl));
  }
  hipLaunchKernelGGL(k_pop_plan, dim3((unsigned int)n_ops), dim3(64), 0, st, (int)k, d_better_tok, d_better_off, d_worse_tok,
                     d_worse_off, d_interest, s->plans.as<PopPlan>(), dout + o_veto);
  hipLaunchKernelGGL(k_pop_rewrite, dim3((unsigned int)n_reads), dim3(64), 0, st, (int)k, (int)(two_v - 1),
                     s->plans.as<PopPlan>(), d_worse_tok, d_worse_off, d_read_tok, d_read_off, d_read_op, d_stage_off,
                     dout + o_status, (int*)(dout + o_first), (int*)(dout + o_last), s->len.as<long long>(),
                     s->stage_tok.as<int>(), s->stage_src.as<int>());
  AMGCHK(prim_exscan_i64(c, s->len.as<long long>(), (long long*)(dout + o_off), (size_t)n_reads + 1));
  hipLaunchKernelGGL(k_pop_pack, dim3((unsigned int)n_reads), dim3(64), 0, st, s->len.as<long long>(),
                     (const long long*)(dout + o_off), d_stage_off, s->stage_tok.as<int>(), s->stage_src.as<int>(),
                     (int*)(dout + o_tok), (int*)(dout + o_src));
  HIPCHK(hipGetLastError());
  unsigned char* hout = s->host_out.p;
  HIPCHK(hipMemcpyAsync(hout, dout, o_at, hipMemcpyDeviceToHost, st));
  stage_end(c);
  HIPCHK(hipStreamSynchronize(st));  // the call's one wait
  memcpy(out_off, hout + o_off, ((size_t)n_reads + 1) * 8);
  memcpy(first_shared, hout + o_first, (size_t)n_reads * 4);
  memcpy(last_shared, hout + o_last, (size_t)n_reads * 4);
  memcpy(status, hout + o_status, (size_t)n_reads);
  memcpy(op_veto, hout + o_veto, (size_t)n_ops);
  const long long total = out_off[n_reads];
  if (total < 0 || total > need) return amg_fail(AMG_E_OVERFLOW, "pop rewrite: %lld genes packed, room for %lld", total, need);
  if (total) {
    memcpy(out_tok, hout + o_tok, (size_t)total * 4);
    memcpy(out_src, hout + o_src, (size_t)total * 4);
  }
  *n_out = total;
  return AMG_OK;
}
