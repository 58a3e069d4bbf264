// amg_bubbles.hip — the junction path search of bubble popping, on device ids, and the
// host's alignment of two short gene lists:
//
//   amg_junction_paths         every path between two junctions of the live graph that has a rival — the set
//                              get_all_paths_between_junctions_in_component collects (reference construct_graph.py:2066-2098)
//                              with new_find_paths_between_nodes (:2292-2342) run once per (start, stop) PAIR of junctions.
//                              The search from a start does not depend on the stop except for where it ends, and a path
//                              without a repeated node ends at the stop the only time it meets it: ONE search per start that
//                              notes every junction it arrives at finds the same paths, J times cheaper (k_bj_*, on
//                              wave_dfs of amg_wave_dfs.h).
//   amg_get_junction_paths     what the search found, to the caller.
//   amg_nw_align               needleman_wunsch on interned genes, on the host.
//
// The resident bases and the sketches of the paths are amg_sketch.hip's.  What decides with these numbers (which path
// of a pair is the better one, which reads are rewritten) stays host-side orchestration over a handful of paths, as in
// the reference (amira_amd/bubble_popping.py).
#include "amg_wave_dfs.h"

#include <algorithm>

// what amg_junction_paths found, until the caller has fetched it (amg_get_junction_paths), and the search's buffers
struct BubbleState {
  std::vector<int> j_node;
  std::vector<signed char> j_dir;
  std::vector<int> p_start;
  std::vector<long long> p_off;
  std::vector<int> p_node;
  std::vector<signed char> p_dir;
  DevBuf jflag, jpos, jrows, cnt_rec, cnt_int, rec_base, int_base, rec_stop, rec_off, pool_node, pool_dir;
};

void bubbles_release(amg_ctx* c) {
  if (!c->bub) return;
  BubbleState* b = c->bub;
  DevBuf* all[] = {&b->jflag, &b->jpos, &b->jrows, &b->cnt_rec, &b->cnt_int, &b->rec_base, &b->int_base, &b->rec_stop,
                   &b->rec_off, &b->pool_node, &b->pool_dir};
  for (DevBuf* d : all) d->release();
  delete b;
  c->bub = nullptr;
}

static BubbleState* bub_of(amg_ctx* c) {
  if (!c->bub) c->bub = new BubbleState();
  return c->bub;
}

// ------------------------------------------------------------------ junctions (:2252-2265 identify_potential_bubble_starts)
// row 2n (2n + 1) of a live node with more than one live edge in its forward (backward) list; rows ascend = the nodes in
// the reference's insertion order, a node's forward side before its backward side
__global__ void k_bj_flag(GView g, long long rows, unsigned char* __restrict__ flag) {
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  flag[r] = (g.n_alive[r >> 1] && g.lrows[r].y > 1) ? 1 : 0;
}

__global__ void k_bj_rows(const unsigned char* __restrict__ flag, const long long* __restrict__ pos, long long rows,
                          int* __restrict__ jrows) {
  const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (r < rows && flag[r]) jrows[pos[r]] = (int)r;
}

// live edges from node a (either list) to node b
__device__ __forceinline__ int bj_edges_between(const GView& g, int a, int b) {
  int n = 0;
  for (int side = 0; side < 2; ++side) {
    const int4 rw = g.lrows[2ll * a + side];
    for (int i = 0; i < rw.y; ++i) n += (g.lent[rw.x + i].x == b) ? 1 : 0;
  }
  return n;
}

#define BJ_MULTI 1ull    // a path ends at a junction over a pair of nodes with more than one edge between them
#define BJ_BUDGET 2ull   // a search was abandoned
#define BJ_STEPS (1ull << 24)   // nodes a search may enter; AMG_TEST_BJ_STEPS=n (test hook, 1 <= n <= 2^24) asks for fewer

// One WAVE per start junction, the search run cooperatively (wave_dfs, amg_wave_dfs.h: stack level d lives in lane d).
// A node entered at depth d >= 1 with L = d + 1 <= distance nodes on the path that is a junction on the side the
// path arrives at is a record {stop junction, the L nodes and directions}; EMIT = false counts records and path nodes,
// EMIT = true writes them behind the start's share of the pools — in search order, which is the order the reference's
// per-stop searches return them in.  Nodes are expanded while L < distance (a longer path ends nowhere: :2305).
template <bool EMIT>
struct BjVisit {
  const GView& g;
  const unsigned char* jflag;
  const long long *jpos, *rec_base, *int_base;  // (the bases and what follows: EMIT only)
  int* rec_stop;
  long long* rec_off;
  int* pool_node;
  signed char* pool_dir;
  long long j;
  int distance, lane;
  long long n_rec, n_int;
  unsigned long long budget, steps, bad;
  __device__ __forceinline__ int enter(int d, int L, int cur_node, int cur_dir, int my_node, int my_dir) {
    if (++steps > budget) {
      bad |= BJ_BUDGET;
      return WD_ABORT;
    }
    if (d >= 1 && L <= distance && (jflag[2ll * cur_node] | jflag[2ll * cur_node + 1])) {
      // the reference asks for THE edge between the last two nodes of every path that ends at a junction node
      // (:2086, :1515-1523) and fails when there are several
      const int prev = __builtin_amdgcn_readlane(my_node, d - 1);
      if (bj_edges_between(g, prev, cur_node) > 1 || bj_edges_between(g, cur_node, prev) > 1) bad |= BJ_MULTI;
      // arriving with direction +1 is arriving through the node's backward side (:1523: -1 x the edge's target direction)
      const long long arow = 2ll * cur_node + (cur_dir == 1 ? 1 : 0);
      if (jflag[arow]) {
        if (EMIT) {
          const long long ri = rec_base[j] + n_rec, io = int_base[j] + n_int;
          if (lane == 0) {
            rec_stop[ri] = (int)jpos[arow];
            rec_off[ri] = io;
          }
          if (lane < L) {
            pool_node[io + lane] = my_node;
            pool_dir[io + lane] = (signed char)my_dir;
          }
        }
        ++n_rec;
        n_int += L;
      }
    }
    return L >= distance ? WD_RETREAT : WD_EXPAND;
  }
};

template <bool EMIT>
__global__ __launch_bounds__(64) void k_bj_dfs(GView g, const int* __restrict__ jrows, long long J,
                                               const unsigned char* __restrict__ jflag, const long long* __restrict__ jpos,
                                               int distance, unsigned long long budget, long long* __restrict__ cnt_rec,
                                               long long* __restrict__ cnt_int,
                                               const long long* __restrict__ rec_base, const long long* __restrict__ int_base,
                                               int* __restrict__ rec_stop, long long* __restrict__ rec_off,
                                               int* __restrict__ pool_node, signed char* __restrict__ pool_dir,
                                               unsigned long long* __restrict__ flags) {
  const long long j = blockIdx.x;
  if (j >= J) return;
  const int lane = threadIdx.x;
  const int row0 = jrows[j];
  BjVisit<EMIT> v{g, jflag, jpos, rec_base, int_base, rec_stop, rec_off, pool_node, pool_dir, j, distance, lane, 0, 0,
                  budget, 0, 0};
  wave_dfs(g, row0 >> 1, (row0 & 1) ? -1 : 1, lane, v);
  if (lane == 0) {
    if (!EMIT) {
      cnt_rec[j] = v.n_rec;
      cnt_int[j] = v.n_int;
    }
    if (v.bad) atomicOr(flags, v.bad);
  }
}

extern "C" int amg_junction_paths(amg_ctx* c, int32_t max_distance, int64_t* sizes) {
  NEED_BUILT(c);
  if (!sizes) return amg_fail(AMG_E_ARG, "null argument");
  if (max_distance < 2 || max_distance > 64) return amg_fail(AMG_E_ARG, "max_distance must be in [2, 64]");
  unsigned long long budget = BJ_STEPS;
  if (const char* e = getenv("AMG_TEST_BJ_STEPS")) {  // test hook: read on every call, never more than the default
    const long long n = atoll(e);
    budget = n < 1 ? 1ull : ((unsigned long long)n < BJ_STEPS ? (unsigned long long)n : BJ_STEPS);
  }
  BubbleState* b = bub_of(c);
  b->j_node.clear(); b->j_dir.clear(); b->p_start.clear(); b->p_off.assign(1, 0); b->p_node.clear(); b->p_dir.clear();
  sizes[0] = sizes[1] = sizes[2] = sizes[3] = 0;
  const long long D = c->n_nodes, rows = 2 * D;
  if (D == 0) return AMG_OK;
  hipStream_t st = c->stream;
  stages_reset(c);
  AMGCHK(ensure_live_adj(c));
  stage_begin(c, "junction_paths");
  const GView g = make_view(c);
  AMGCHK(b->jflag.ensure((size_t)rows + 64));
  AMGCHK(b->jpos.ensure((size_t)(rows + 2) * sizeof(long long)));
  unsigned long long* flags = c->status.as<unsigned long long>() + ST_MISC;
  {
    ClearList cl;
    cl.add(flags, sizeof(unsigned long long));
    AMGCHK(clear_many(c, cl));
  }
  hipLaunchKernelGGL(k_bj_flag, dim3(nblk(rows, 256)), dim3(256), 0, st, g, rows, b->jflag.as<unsigned char>());
  AMGCHK(prim_exscan_bytes_set(c, b->jflag.as<unsigned char>(), b->jpos.as<long long>(), (size_t)rows));
  long long J = 0;
  {
    FetchList l;
    l.add(b->jpos.as<long long>() + rows);
    AMGCHK(fetch(c, l, reinterpret_cast<unsigned long long*>(&J)));
  }
  if (J == 0) {
    stage_end(c);
    return AMG_OK;
  }
  AMGCHK(b->jrows.ensure((size_t)(J + 1) * sizeof(int)));
  AMGCHK(b->cnt_rec.ensure((size_t)(J + 1) * sizeof(long long)));
  AMGCHK(b->cnt_int.ensure((size_t)(J + 1) * sizeof(long long)));
  AMGCHK(b->rec_base.ensure((size_t)(J + 2) * sizeof(long long)));
  AMGCHK(b->int_base.ensure((size_t)(J + 2) * sizeof(long long)));
  hipLaunchKernelGGL(k_bj_rows, dim3(nblk(rows, 256)), dim3(256), 0, st, b->jflag.as<unsigned char>(), b->jpos.as<long long>(),
                     rows, b->jrows.as<int>());
  hipLaunchKernelGGL(k_bj_dfs<false>, dim3((unsigned int)J), dim3(64), 0, st, g, b->jrows.as<int>(), J,
                     b->jflag.as<unsigned char>(), b->jpos.as<long long>(), (int)max_distance, budget,
                     b->cnt_rec.as<long long>(), b->cnt_int.as<long long>(), (const long long*)nullptr, (const long long*)nullptr, (int*)nullptr,
                     (long long*)nullptr, (int*)nullptr, (signed char*)nullptr, flags);
  AMGCHK(prim_exscan_i64_pair(c, b->cnt_rec.as<long long>(), b->rec_base.as<long long>(), b->cnt_int.as<long long>(),
                              b->int_base.as<long long>(), (size_t)J));
  unsigned long long got[3] = {0, 0, 0};
  {
    FetchList l;
    l.add(b->rec_base.as<long long>() + J);
    l.add(b->int_base.as<long long>() + J);
    l.add(flags);
    AMGCHK(fetch(c, l, got));
  }
  const long long R = (long long)got[0], N = (long long)got[1];
  sizes[3] = (int64_t)got[2];
  std::vector<int> jrows((size_t)J);
  HIPCHK(hipMemcpyAsync(jrows.data(), b->jrows.p, (size_t)J * sizeof(int), hipMemcpyDeviceToHost, st));
  std::vector<long long> rec_base((size_t)J + 1), rec_off((size_t)R + 1);
  std::vector<int> rec_stop((size_t)R), pool_node((size_t)N);
  std::vector<signed char> pool_dir((size_t)N);
  if (R > 0 && !(got[2] & BJ_BUDGET)) {
    AMGCHK(b->rec_stop.ensure((size_t)(R + 1) * sizeof(int)));
    AMGCHK(b->rec_off.ensure((size_t)(R + 1) * sizeof(long long)));
    AMGCHK(b->pool_node.ensure((size_t)(N + 1) * sizeof(int)));
    AMGCHK(b->pool_dir.ensure((size_t)N + 64));
    hipLaunchKernelGGL(k_bj_dfs<true>, dim3((unsigned int)J), dim3(64), 0, st, g, b->jrows.as<int>(), J,
                       b->jflag.as<unsigned char>(), b->jpos.as<long long>(), (int)max_distance, budget,
                       (long long*)nullptr, (long long*)nullptr, b->rec_base.as<long long>(), b->int_base.as<long long>(), b->rec_stop.as<int>(),
                       b->rec_off.as<long long>(), b->pool_node.as<int>(), b->pool_dir.as<signed char>(), flags);
    HIPCHK(hipMemcpyAsync(rec_base.data(), b->rec_base.p, (size_t)(J + 1) * sizeof(long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(rec_off.data(), b->rec_off.p, (size_t)R * sizeof(long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(rec_stop.data(), b->rec_stop.p, (size_t)R * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(pool_node.data(), b->pool_node.p, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(pool_dir.data(), b->pool_dir.p, (size_t)N, hipMemcpyDeviceToHost, st));
  }
  stage_end(c);
  HIPCHK(hipStreamSynchronize(st));
  b->j_node.resize((size_t)J);
  b->j_dir.resize((size_t)J);
  for (long long j = 0; j < J; ++j) {
    b->j_node[(size_t)j] = jrows[(size_t)j] >> 1;
    b->j_dir[(size_t)j] = (jrows[(size_t)j] & 1) ? -1 : 1;
  }
  if (R > 0 && !(got[2] & BJ_BUDGET)) {
    rec_off[(size_t)R] = N;
    // per start: its records by stop (in the order of the junction list, as the reference's inner loop goes), search
    // order kept inside a stop; a stop reached by one path only is no bubble (:2092)
    std::vector<long long> idx;
    for (long long j = 0; j < J; ++j) {
      const long long lo = rec_base[(size_t)j], hi = rec_base[(size_t)j + 1];
      if (hi - lo < 2) continue;
      idx.resize((size_t)(hi - lo));
      for (long long i = lo; i < hi; ++i) idx[(size_t)(i - lo)] = i;
      std::stable_sort(idx.begin(), idx.end(), [&](long long x, long long y) { return rec_stop[(size_t)x] < rec_stop[(size_t)y]; });
      size_t a = 0;
      while (a < idx.size()) {
        size_t e = a + 1;
        while (e < idx.size() && rec_stop[(size_t)idx[e]] == rec_stop[(size_t)idx[a]]) ++e;
        if (e - a > 1)
          for (size_t q = a; q < e; ++q) {
            const long long ri = idx[q];
            b->p_start.push_back((int)j);
            for (long long t = rec_off[(size_t)ri]; t < rec_off[(size_t)ri + 1]; ++t) {
              b->p_node.push_back(pool_node[(size_t)t]);
              b->p_dir.push_back(pool_dir[(size_t)t]);
            }
            b->p_off.push_back((long long)b->p_node.size());
          }
        a = e;
      }
    }
  }
  sizes[0] = J;
  sizes[1] = (int64_t)b->p_start.size();
  sizes[2] = (int64_t)b->p_node.size();
  return AMG_OK;
}

extern "C" int amg_get_junction_paths(amg_ctx* c, int32_t* junction_node, int8_t* junction_dir, int32_t* path_start,
                                      int64_t* path_off, int32_t* path_node, int8_t* path_dir) {
  if (!c) return amg_fail(AMG_E_ARG, "null ctx");
  if (!c->bub) return amg_fail(AMG_E_STATE, "amg_junction_paths first");
  const BubbleState* b = c->bub;
  if (junction_node && !b->j_node.empty()) memcpy(junction_node, b->j_node.data(), b->j_node.size() * sizeof(int));
  if (junction_dir && !b->j_dir.empty()) memcpy(junction_dir, b->j_dir.data(), b->j_dir.size());
  if (path_start && !b->p_start.empty()) memcpy(path_start, b->p_start.data(), b->p_start.size() * sizeof(int));
  if (path_off) memcpy(path_off, b->p_off.data(), b->p_off.size() * sizeof(long long));
  if (path_node && !b->p_node.empty()) memcpy(path_node, b->p_node.data(), b->p_node.size() * sizeof(int));
  if (path_dir && !b->p_dir.empty()) memcpy(path_dir, b->p_dir.data(), b->p_dir.size());
  return AMG_OK;
}

// ------------------------------------------------------------------ the alignment of two short gene lists (host)
// needleman_wunsch (construct_graph.py:1433-1480) on interned genes: match 1, mismatch 0, gap -1, borders -index, the
// best of (score, pointer) with the pointers ordered DIAG < LEFT < UP — a tie goes UP, then LEFT.  ops, in alignment
// order: 0 = (x, y), 1 = (x, *), 2 = (*, y); at most n + m of them.  The two paths of a bubble are a few dozen genes:
// this is the host's share of compare_paths (:1566) where bubble popping rewrites its reads in the loop on the host
// (AMG_POP_REWRITE=0, AMG_BUBBLES_BY_OBJECTS=1, a graph edited on the host, a path beyond amg_pop_rewrite's 128 genes):
// once per correction operation, and once per read whose stretch differs.  By default amg_pop_rewrite (amg_pop.hip)
// computes the same recurrence and traceback on the device.
extern "C" int amg_nw_align(const int32_t* x, int32_t n, const int32_t* y, int32_t m, int8_t* ops, int32_t* n_ops) {
  if (n < 0 || m < 0 || !n_ops || ((n || m) && !ops) || (n && !x) || (m && !y)) return amg_fail(AMG_E_ARG, "bad argument");
  const int W = m + 1;
  std::vector<int> F((size_t)(n + 1) * W);
  std::vector<signed char> P((size_t)(n + 1) * W, 0);
  // F[i + 1][j + 1] = the reference's F[i, j]; its borders are F[i, -1] = -i, F[-1, j] = -j (so F[0, -1] = 0 too)
  F[0] = 0;
  for (int i = 0; i < n; ++i) F[(size_t)(i + 1) * W] = -i;
  for (int j = 0; j < m; ++j) F[(size_t)j + 1] = -j;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < m; ++j) {
      const int diag = F[(size_t)i * W + j] + (x[i] == y[j] ? 1 : 0);
      const int left = F[(size_t)i * W + j + 1] - 1;   // F[i - 1, j] - 1: a gene of x against a gap
      const int up = F[(size_t)(i + 1) * W + j] - 1;   // F[i, j - 1] - 1: a gene of y against a gap
      int best = diag;
      signed char ptr = 0;
      if (left >= best) { best = left; ptr = 1; }
      if (up >= best) { best = up; ptr = 2; }
      F[(size_t)(i + 1) * W + j + 1] = best;
      P[(size_t)(i + 1) * W + j + 1] = ptr;
    }
  std::vector<signed char> rev;
  int i = n - 1, j = m - 1;
  while (i >= 0 && j >= 0) {
    const signed char p = P[(size_t)(i + 1) * W + j + 1];
    rev.push_back(p);
    if (p == 0) { --i; --j; } else if (p == 1) { --i; } else { --j; }
  }
  while (i >= 0) { rev.push_back(1); --i; }
  while (j >= 0) { rev.push_back(2); --j; }
  *n_ops = (int32_t)rev.size();
  for (size_t t = 0; t < rev.size(); ++t) ops[t] = rev[rev.size() - 1 - t];
  return AMG_OK;
}
