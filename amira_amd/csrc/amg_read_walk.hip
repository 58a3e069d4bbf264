// amg_read_walk.hip — three questions asked of every read of a built graph, answered by one walk over `tokens` and
// `tok_node`: the depth of the graph by read length (get_overall_mean_node_coverages, graph_utils.py:299-313), AMR
// trimming (remove_non_AMR_associated_nodes, construct_graph.py:2941-2959) and the AMR reads of every component
// (the validity test inside choose_kmer_size, graph_utils.py:258-296).
//
// Window i of a read [a, b) starts at token a + i; it is LIVE when tok_node[a + i] >= 0 and that node is alive, and an
// AMR window when one of its k tokens is a gene of interest — which is "the node's canonical gene-mer contains the
// gene", read from the token stream, so it also holds for nodes keyed by a fingerprint.
//   A  pairs[j]   = distinct (read, node) pairs with a live window of the read on the node, over reads of at least
//                   min_genes[j] genes (Node.add_read keeps distinct reads, construct_node.py:64-67)
//   B  hit(r)     = read r has a live AMR window; keep(d) = a live window of a hit read sits on node d; every alive node
//                   that is not kept is removed
//   C  n_reads[c] = reads with a live AMR window on a node of component c (a read counts once per component),
//                   n_long[c] = those of them with at least min_genes genes
#include "amg_device.h"
#include "amg_read_walk.h"

#define RW_READS_PER_WAVE 8  // as k_mask_reads (amg_filter.hip), and for its reason: see walk_reads
#define RW_WAVES 4
#define RW_GROUP (RW_WAVES * RW_READS_PER_WAVE)  // reads a workgroup takes at a time
#define RW_MAX_BLOCKS 2048                        // workgroups of a walk: each goes over its share of the groups
// The genes of interest travel as a bitmap of V bits.  A workgroup stages it in LDS when it has at most `lds_words`
// words (a kernel argument, at most RW_FLAG_WORDS_MAX) and reads it from global memory otherwise.  The entry points pass
// RW_FLAG_WORDS_BUDGET: 20 480 genes = 2.5 KB, copied once per workgroup, i.e. once per n_reads / RW_MAX_BLOCKS reads.
#define RW_FLAG_WORDS_MAX 4096
#define RW_FLAG_WORDS_BUDGET 640
#define RW_CACHE_SLOTS 256  // LDS slots in which a workgroup sums up the components of C before it touches global memory

struct RwArgs {
  const int* tok_node;
  const int* tokens;
  const long long* read_off;
  long long n_reads;
  const unsigned char* node_alive;
  const int* node_comp;           // C only
  const unsigned int* flag_bits;  // B (hit), C: bit r set = the gene of rank r is a gene of interest
  int flag_words, lds_words;
  int V, k;
};

struct Flags {
  const unsigned int* words;  // global
  const unsigned int* staged;  // LDS
  bool in_lds;
  int V;
  // rank of token t: t - V for '+', V - 1 - t for '-' (include/amg.h, data model)
  __device__ __forceinline__ bool of_token(int t) const {
    const int r = t >= V ? t - V : V - 1 - t;
    if ((unsigned int)r >= (unsigned int)V) return false;
    const unsigned int w = in_lds ? staged[r >> 5] : words[r >> 5];
    return (w >> (r & 31)) & 1u;
  }
};

// What a lane knows of the window that starts at its token of a 64-token chunk.  The three steps are apart so that
// walk_reads can issue each of them for all its reads before it uses any.
struct RwRaw {
  int node, tok;
};
struct RwDep {
  bool alive, bit;
  int comp;
};
struct RwWin {
  int node, comp;
  bool live, amr;
};

template <class Use>
__device__ __forceinline__ RwRaw rw_load_raw(const RwArgs& g, long long a, long long b, long long p, int lane) {
  const long long t = a + p + lane;
  const bool in = t < b;
  RwRaw r;
  r.node = in ? g.tok_node[t] : -1;
  r.tok = (Use::AMR && in) ? g.tokens[t] : -1;
  return r;
}

template <class Use>
__device__ __forceinline__ RwDep rw_load_dep(const RwArgs& g, const Flags& f, const RwRaw& r) {
  RwDep d;
  d.alive = r.node >= 0 && g.node_alive[r.node] != 0;
  d.comp = (Use::COMP && r.node >= 0) ? g.node_comp[r.node] : 0;
  d.bit = Use::AMR && r.tok >= 0 && f.of_token(r.tok);
  return d;
}

// One ballot of the 64 interest bits answers every window of the chunk: window `lane` holds a gene of interest when one
// of the bits lane .. lane + k - 1 is set.  That settles the windows of lanes 0 .. 64 - k; a walk that looks at genes
// therefore advances by 64 - k + 1 tokens a chunk (rw_step), one that does not by 64.
template <class Use>
__device__ __forceinline__ int rw_step(const RwArgs& g) {
  return Use::AMR ? 64 - g.k + 1 : 64;
}
template <class Use>
__device__ __forceinline__ RwWin rw_make_win(const RwArgs& g, const RwRaw& r, const RwDep& d, int lane) {
  RwWin w;
  w.node = r.node;
  w.comp = d.comp;
  w.live = d.alive && lane < rw_step<Use>(g);
  w.amr = false;
  if (Use::AMR) {
    const unsigned long long m = __ballot(d.bit);
    w.amr = ((m >> lane) & ((1ull << g.k) - 1ull)) != 0ull;
  }
  return w;
}
template <class Use>
__device__ __forceinline__ RwWin rw_chunk(const RwArgs& g, const Flags& f, long long a, long long b, long long p, int lane) {
  const RwRaw r = rw_load_raw<Use>(g, a, b, p, lane);
  return rw_make_win<Use>(g, r, rw_load_dep<Use>(g, f, r), lane);
}

// some lane below `limit` holds the value val (>= 0) in `other`
__device__ __forceinline__ bool rw_seen(int val, int other, int limit) {
  bool seen = false;
  for (unsigned long long m = __ballot(other >= 0); m; m &= m - 1ull) {
    const int s = __ffsll((long long)m) - 1;
    const int o = __builtin_amdgcn_readlane(other, s);
    seen = seen || (s < limit && o == val);
  }
  return seen;
}

// "First occurrence within the read" of a lane's value val = use.value(window) (>= 0; < 0: the window has none), used
// for the node ids of A and the component labels of C: exact for any read length.  Within the chunk the lower lanes
// are compared.  A chunk that is not the read's first is compared against every earlier chunk of the read, which is
// looked at again (through L2): QUADRATIC in the read's windows, and only for reads beyond one chunk (64 windows, or
// 64 - k + 1 where genes are looked at).
template <class Use>
__device__ __forceinline__ bool rw_first_in_read(const Use& use, const RwArgs& g, const Flags& f, long long a, long long b,
                                                 long long p, int val, int lane) {
  if (!__any(val >= 0)) return false;
  bool seen = rw_seen(val, val, lane);
  for (long long q = 0; q < p; q += rw_step<Use>(g)) {
    const bool before = rw_seen(val, use.value(rw_chunk<Use>(g, f, a, b, q, lane)), 64);  // (every lane takes part)
    seen = seen || before;
  }
  return val >= 0 && !seen;
}

// THE walker.  A wave takes RW_READS_PER_WAVE consecutive reads and issues every load of a stage for all of them before
// it uses any — offsets, then node ids and genes, then alive bytes, labels and interest bits — because one read per wave
// is bound by that chain of a single short read (k_mask_reads, amg_filter.hip).  Reads beyond one chunk go on chunk by
// chunk.  Use: AMR / COMP (what is loaded), read_word (a word per read, loaded with the offsets), skip, begin_read,
// chunk, end_read.
template <class Use>
__device__ __forceinline__ void walk_reads(const RwArgs& g, const Flags& f, long long rbase, int lane, Use& use) {
  constexpr int R = RW_READS_PER_WAVE;
  const int step = rw_step<Use>(g);
  const long long off_l = (lane <= R && rbase + lane <= g.n_reads) ? g.read_off[rbase + lane] : 0;
  const int word_l = (lane < R && rbase + lane < g.n_reads) ? use.read_word(rbase + lane) : 0;
  long long a[R], b[R];
  int word[R];
#pragma unroll
  for (int j = 0; j < R; ++j) {
    a[j] = __shfl(off_l, j, 64);
    b[j] = rbase + j < g.n_reads ? __shfl(off_l, j + 1, 64) : a[j];
    word[j] = __shfl(word_l, j, 64);
  }
  RwRaw raw[R];
#pragma unroll
  for (int j = 0; j < R; ++j) raw[j] = rw_load_raw<Use>(g, a[j], b[j], 0, lane);
  RwDep dep[R];
#pragma unroll
  for (int j = 0; j < R; ++j) dep[j] = rw_load_dep<Use>(g, f, raw[j]);
#pragma unroll
  for (int j = 0; j < R; ++j) {
    if (rbase + j >= g.n_reads || use.skip(word[j])) continue;  // (wave-uniform)
    const long long len = b[j] - a[j], n_win = len - g.k + 1;
    use.begin_read(len);
    use.chunk(g, f, a[j], b[j], 0, rw_make_win<Use>(g, raw[j], dep[j], lane), lane);
    for (long long p = step; p < n_win; p += step) use.chunk(g, f, a[j], b[j], p, rw_chunk<Use>(g, f, a[j], b[j], p, lane), lane);
    use.end_read(rbase + j, lane);
  }
}

template <class Use>
__global__ __launch_bounds__(64 * RW_WAVES) void k_read_walk(RwArgs g, Use use) {
  __shared__ unsigned int s_bits[Use::AMR ? RW_FLAG_WORDS_MAX : 1];
  Flags f;
  f.words = g.flag_bits;
  f.staged = s_bits;
  f.in_lds = Use::AMR && g.flag_words <= g.lds_words && g.flag_words <= RW_FLAG_WORDS_MAX;
  f.V = g.V;
  if (f.in_lds)
    for (int i = threadIdx.x; i < g.flag_words; i += blockDim.x) s_bits[i] = g.flag_bits[i];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  use.block_begin(lane);
  __syncthreads();
  const long long n_groups = (g.n_reads + RW_GROUP - 1) / RW_GROUP;
  for (long long grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
    const long long rbase = grp * RW_GROUP + (long long)wave * RW_READS_PER_WAVE;
    if (rbase < g.n_reads) walk_reads(g, f, rbase, lane, use);
  }
  use.block_end(lane, wave);  // (every thread)
}

// ------------------------------------------------------------------ A: depth by read length
struct DepthUse {
  static constexpr bool AMR = false, COMP = false;
  int min_genes[RW_MAX_LENGTHS];
  int n;
  unsigned long long* pairs;  // [n]
  // per thread: lane j < n sums up the pairs of the reads with at least min_genes[j] genes
  int mine;
  long long len;
  unsigned long long acc;
  unsigned int cnt;
  __device__ __forceinline__ void block_begin(int lane) {
    mine = 0x7fffffff;
#pragma unroll
    for (int j = 0; j < RW_MAX_LENGTHS; ++j)
      if (j < n && lane == j) mine = min_genes[j];
    acc = 0;
  }
  __device__ __forceinline__ int read_word(long long) const { return 0; }
  __device__ __forceinline__ bool skip(int) const { return false; }
  __device__ __forceinline__ int value(const RwWin& w) const { return w.live ? w.node : -1; }
  __device__ __forceinline__ void begin_read(long long l) {
    len = l;
    cnt = 0;
  }
  __device__ __forceinline__ void chunk(const RwArgs& g, const Flags& f, long long a, long long b, long long p, const RwWin& w,
                                        int lane) {
    cnt += (unsigned int)__popcll(__ballot(rw_first_in_read(*this, g, f, a, b, p, value(w), lane)));
  }
  __device__ __forceinline__ void end_read(long long, int) {
    if (len >= (long long)mine) acc += cnt;
  }
  // one atomic per length and WORKGROUP
  __device__ __forceinline__ void block_end(int lane, int wave) {
    __shared__ unsigned long long s_part[RW_WAVES][RW_MAX_LENGTHS];
    if (lane < RW_MAX_LENGTHS) s_part[wave][lane] = acc;
    __syncthreads();
    if (wave == 0 && lane < n) {
      unsigned long long sum = 0;
      for (int w = 0; w < RW_WAVES; ++w) sum += s_part[w][lane];
      if (sum) atomicAdd(&pairs[lane], sum);
    }
  }
};

__global__ __launch_bounds__(256) void k_rw_count_alive(const unsigned char* __restrict__ alive, long long n,
                                                        unsigned long long* __restrict__ out) {
  __shared__ unsigned long long s_part[4];
  unsigned long long v = 0;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    v += alive[i] ? 1ull : 0ull;
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long sum = s_part[0] + s_part[1] + s_part[2] + s_part[3];
    if (sum) atomicAdd(out, sum);
  }
}

// ------------------------------------------------------------------ B: AMR trimming
struct HitUse {
  static constexpr bool AMR = true, COMP = false;
  unsigned char* hit;  // [n_reads], every entry written
  bool any;
  __device__ __forceinline__ void block_begin(int) {}
  __device__ __forceinline__ int read_word(long long) const { return 0; }
  __device__ __forceinline__ bool skip(int) const { return false; }
  __device__ __forceinline__ void begin_read(long long) { any = false; }
  __device__ __forceinline__ void chunk(const RwArgs&, const Flags&, long long, long long, long long, const RwWin& w, int) {
    any = any || (w.live && w.amr);
  }
  __device__ __forceinline__ void end_read(long long r, int lane) {
    const bool h = __any(any);
    if (lane == 0) hit[r] = h ? 1 : 0;
  }
  __device__ __forceinline__ void block_end(int, int) {}
};

struct KeepUse {
  static constexpr bool AMR = false, COMP = false;
  const unsigned char* hit;  // [n_reads]
  unsigned char* keep;       // [n_nodes], zeroed; byte stores of 1 that race benignly
  __device__ __forceinline__ void block_begin(int) {}
  __device__ __forceinline__ int read_word(long long r) const { return hit[r]; }
  __device__ __forceinline__ bool skip(int word) const { return word == 0; }
  __device__ __forceinline__ void begin_read(long long) {}
  __device__ __forceinline__ void chunk(const RwArgs&, const Flags&, long long, long long, long long, const RwWin& w, int) {
    if (w.live) keep[w.node] = 1;
  }
  __device__ __forceinline__ void end_read(long long, int) {}
  __device__ __forceinline__ void block_end(int, int) {}
};

__global__ void k_rw_kill_unkept(const unsigned char* __restrict__ alive, const unsigned char* __restrict__ keep, long long n,
                                 unsigned char* __restrict__ kill) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && alive[i] && !keep[i]) kill[i] = 1;
}

// ------------------------------------------------------------------ C: AMR reads per component
// In a real graph nearly every read lands in the one giant component: a workgroup sums its reads per component in LDS
// (direct-mapped slots, claimed by the first component that asks; a component that finds its slot taken goes to global
// memory at once) and adds every slot to global memory once, when it is done with all its groups.
struct CompCache {
  int label[RW_CACHE_SLOTS];
  unsigned int n[RW_CACHE_SLOTS], n_long[RW_CACHE_SLOTS];
};
__device__ __forceinline__ CompCache* rw_comp_cache() {
  __shared__ CompCache s_cache;
  return &s_cache;
}

struct CompUse {
  static constexpr bool AMR = true, COMP = true;
  unsigned long long* n_reads;  // [n_comp], entry c: the component with label c + 1 (ensure_components labels from 1)
  unsigned long long* n_long;   // [n_comp]
  int n_comp, min_genes;
  bool is_long;
  __device__ __forceinline__ void block_begin(int) {
    CompCache* c = rw_comp_cache();
    for (int i = threadIdx.x; i < RW_CACHE_SLOTS; i += blockDim.x) {
      c->label[i] = -1;
      c->n[i] = c->n_long[i] = 0u;
    }
  }
  __device__ __forceinline__ int read_word(long long) const { return 0; }
  __device__ __forceinline__ bool skip(int) const { return false; }
  __device__ __forceinline__ int value(const RwWin& w) const {
    return (w.live && w.amr && (unsigned int)(w.comp - 1) < (unsigned int)n_comp) ? w.comp - 1 : -1;
  }
  __device__ __forceinline__ void begin_read(long long len) { is_long = len >= (long long)min_genes; }
  __device__ __forceinline__ void add(int c) {
    CompCache* s = rw_comp_cache();
    const int slot = c & (RW_CACHE_SLOTS - 1);
    const int old = atomicCAS(&s->label[slot], -1, c);
    if (old == -1 || old == c) {
      atomicAdd(&s->n[slot], 1u);
      if (is_long) atomicAdd(&s->n_long[slot], 1u);
    } else {
      atomicAdd(&n_reads[c], 1ull);
      if (is_long) atomicAdd(&n_long[c], 1ull);
    }
  }
  __device__ __forceinline__ void chunk(const RwArgs& g, const Flags& f, long long a, long long b, long long p, const RwWin& w,
                                        int lane) {
    const int val = value(w);
    if (rw_first_in_read(*this, g, f, a, b, p, val, lane)) add(val);  // (one lane per component of the read)
  }
  __device__ __forceinline__ void end_read(long long, int) {}
  __device__ __forceinline__ void block_end(int, int) {
    __syncthreads();
    CompCache* s = rw_comp_cache();
    for (int i = threadIdx.x; i < RW_CACHE_SLOTS; i += blockDim.x) {
      const int c = s->label[i];
      if (c < 0) continue;
      if (s->n[i]) atomicAdd(&n_reads[c], (unsigned long long)s->n[i]);
      if (s->n_long[i]) atomicAdd(&n_long[c], (unsigned long long)s->n_long[i]);
    }
  }
};

// ------------------------------------------------------------------ host side
// A graph made by amg_dist_merge* has the nodes of all ranks' reads and the windows of this rank's reads alone: the
// single-GPU calls would answer for a shard, the collective (amg_dist_walk*, amg_dist_walk.hip) answers for all reads
#define NEED_ALL_READS(c, what)                                                                                         \
  do {                                                                                                                  \
    NEED_BUILT(c);                                                                                                      \
    if ((c)->dist_mode)                                                                                                 \
      return amg_fail(AMG_E_STATE, what ": the graph came from a merged build (amg_dist_merge*), this ctx holds only "  \
                                        "its own shard of the reads; sums across ranks are not made here "              \
                                        "(the collective: amg_dist_walk*)");                                            \
  } while (0)

static RwArgs rw_args(amg_ctx* c, const unsigned int* flag_bits, int flag_words) {
  RwArgs g;
  g.tok_node = c->tok_node.as<int>();
  g.tokens = c->tokens.as<int>();
  g.read_off = c->read_off.as<long long>();
  g.n_reads = c->n_reads;
  g.node_alive = c->node_alive.as<unsigned char>();
  g.node_comp = c->node_comp.as<int>();
  g.flag_bits = flag_bits;
  g.flag_words = flag_words;
  g.lds_words = RW_FLAG_WORDS_BUDGET;
  g.V = c->two_v / 2;
  g.k = c->k;
  return g;
}

template <class Use>
static void rw_launch(amg_ctx* c, const RwArgs& g, const Use& use) {
  const unsigned int groups = nblk(c->n_reads, RW_GROUP);
  hipLaunchKernelGGL(k_read_walk<Use>, dim3(groups < RW_MAX_BLOCKS ? groups : RW_MAX_BLOCKS), dim3(64 * RW_WAVES), 0, c->stream,
                     g, use);
}

// gene_flags[V] (host bytes) as a bitmap on the device; `words` holds the host copy until the stream has taken it
struct RwFlagBits {
  const unsigned int* bits = nullptr;
  int words = 0;
};
static int rw_upload_flags(amg_ctx* c, const uint8_t* gene_flags, std::vector<unsigned int>* words, RwFlagBits* out) {
  const int V = c->two_v / 2;
  words->assign((size_t)(V + 31) / 32, 0u);
  for (int r = 0; r < V; ++r)
    if (gene_flags[r]) (*words)[(size_t)r >> 5] |= 1u << (r & 31);
  AMGCHK(c->s5.ensure(words->size() * sizeof(unsigned int) + 64));
  HIPCHK(hipMemcpyAsync(c->s5.p, words->data(), words->size() * sizeof(unsigned int), hipMemcpyHostToDevice, c->stream));
  *out = RwFlagBits{c->s5.as<unsigned int>(), (int)words->size()};
  return AMG_OK;
}

// ---- the local phases: the walks over the reads THIS ctx holds.  The single-GPU entry points below are a local phase
// and a read-back; the walks across ranks (amg_dist_walk.hip) put an exchange and a fold between the two.
int rw_depth_local(amg_ctx* c, const int32_t* min_genes, int32_t n, unsigned long long* out) {
  stage_begin(c, "depth");
  {
    ClearList cl;
    cl.add(out, RW_DEPTH_WORDS * sizeof(unsigned long long));
    AMGCHK(clear_many(c, cl));
  }
  DepthUse use;
  for (int j = 0; j < RW_MAX_LENGTHS; ++j) use.min_genes[j] = j < n ? min_genes[j] : 0;
  use.n = n;
  use.pairs = out;
  if (c->n_reads > 0) rw_launch(c, rw_args(c, nullptr, 0), use);
  if (c->n_nodes > 0)
    hipLaunchKernelGGL(k_rw_count_alive, dim3(nblk(c->n_nodes, 2048) < 256u ? nblk(c->n_nodes, 2048) : 256u), dim3(256), 0,
                       c->stream, c->node_alive.as<unsigned char>(), c->n_nodes, out + RW_MAX_LENGTHS);
  stage_end(c);
  return AMG_OK;
}

int rw_keep_local(amg_ctx* c, const uint8_t* gene_flags, std::vector<unsigned int>* words, RwKeep* out) {
  const long long D = c->n_nodes;
  RwFlagBits flags;
  AMGCHK(rw_upload_flags(c, gene_flags, words, &flags));
  ClearList cl;
  AMGCHK(kill_marks_reserve(c, &cl, &out->marks));
  AMGCHK(c->s1.ensure((size_t)c->n_reads + 8));
  AMGCHK(c->s4.ensure((size_t)D + 8));
  cl.add(c->s4.p, (size_t)D + 8);
  AMGCHK(clear_many(c, cl));
  out->keep = c->s4.as<unsigned char>();
  if (c->n_reads > 0) {
    HitUse hit;
    hit.hit = c->s1.as<unsigned char>();
    rw_launch(c, rw_args(c, flags.bits, flags.words), hit);
    KeepUse keep;
    keep.hit = c->s1.as<unsigned char>();
    keep.keep = c->s4.as<unsigned char>();
    rw_launch(c, rw_args(c, nullptr, 0), keep);
  }
  return AMG_OK;
}

int rw_comp_local(amg_ctx* c, const uint8_t* gene_flags, int32_t min_genes, std::vector<unsigned int>* words, RwComp* out) {
  const long long nc = c->n_components;
  stage_begin(c, "amr_reads");
  RwFlagBits flags;
  AMGCHK(rw_upload_flags(c, gene_flags, words, &flags));
  const size_t out_bytes = 2 * (size_t)nc * sizeof(unsigned long long);
  AMGCHK(c->s4.ensure(out_bytes));
  {
    ClearList cl;
    cl.add(c->s4.p, out_bytes);
    AMGCHK(clear_many(c, cl));
  }
  unsigned long long* counts = c->s4.as<unsigned long long>();
  *out = RwComp{counts, counts + nc, nc};
  if (c->n_reads > 0) {
    CompUse use;
    use.n_reads = counts;
    use.n_long = counts + nc;
    use.n_comp = (int)nc;
    use.min_genes = min_genes;
    rw_launch(c, rw_args(c, flags.bits, flags.words), use);
  }
  stage_end(c);
  return AMG_OK;
}

// ------------------------------------------------------------------ the single-GPU entry points
extern "C" int amg_depth_by_length(amg_ctx* c, const int32_t* min_genes, int32_t n, int64_t* pairs, int64_t* n_alive) {
  NEED_ALL_READS(c, "amg_depth_by_length");
  if (!min_genes || !pairs || !n_alive) return amg_fail(AMG_E_ARG, "null argument");
  if (n < 1 || n > RW_MAX_LENGTHS) return amg_fail(AMG_E_ARG, "n must be in [1, %d]", RW_MAX_LENGTHS);
  stages_reset(c);
  AMGCHK(c->s4.ensure(RW_DEPTH_WORDS * sizeof(unsigned long long)));
  unsigned long long* out = c->s4.as<unsigned long long>();
  AMGCHK(rw_depth_local(c, min_genes, n, out));
  unsigned long long host[RW_DEPTH_WORDS];
  FetchList l;
  l.add_words(out, RW_DEPTH_WORDS);
  AMGCHK(fetch(c, l, host));
  for (int j = 0; j < n; ++j) pairs[j] = (int64_t)host[j];
  *n_alive = (int64_t)host[RW_MAX_LENGTHS];
  return AMG_OK;
}

extern "C" int amg_remove_non_amr_nodes(amg_ctx* c, const uint8_t* gene_flags, int64_t* n_removed) {
  NEED_ALL_READS(c, "amg_remove_non_amr_nodes");
  if (!gene_flags || !n_removed) return amg_fail(AMG_E_ARG, "null argument");
  *n_removed = 0;
  const long long D = c->n_nodes;
  if (D == 0) return AMG_OK;
  ctx_removal_begins(c);
  stages_reset(c);
  stage_begin(c, "amr_trim");
  std::vector<unsigned int> words;
  RwKeep kept;
  AMGCHK(rw_keep_local(c, gene_flags, &words, &kept));
  hipLaunchKernelGGL(k_rw_kill_unkept, dim3(nblk(D, 256)), dim3(256), 0, c->stream, c->node_alive.as<unsigned char>(),
                     kept.keep, D, kept.marks.bytes);
  const int r = finish_kill(c, kept.marks, n_removed, nullptr);  // (waits for the stream: `words` has been taken)
  stage_end(c);
  return r;
}

extern "C" int amg_component_amr_reads(amg_ctx* c, const uint8_t* gene_flags, int32_t min_genes, int64_t cap, int64_t* n_reads,
                                       int64_t* n_long, int64_t* n_components) {
  NEED_ALL_READS(c, "amg_component_amr_reads");
  if (!n_components) return amg_fail(AMG_E_ARG, "null argument");
  stages_reset(c);
  AMGCHK(ensure_components(c));
  const long long nc = c->n_components;
  *n_components = nc;
  if (!gene_flags || !n_reads || !n_long) return amg_fail(AMG_E_ARG, "null argument");
  if (cap < nc) return amg_fail(AMG_E_ARG, "room for %lld components, the graph has %lld", (long long)cap, nc);
  if (nc == 0) return AMG_OK;
  std::vector<unsigned int> words;
  RwComp counts;
  AMGCHK(rw_comp_local(c, gene_flags, min_genes, &words, &counts));
  HIPCHK(hipMemcpyAsync(n_reads, counts.n_reads, (size_t)nc * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(n_long, counts.n_long, (size_t)nc * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return AMG_OK;
}
