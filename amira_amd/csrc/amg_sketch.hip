// amg_sketch.hip — scaled MinHash sketches of nucleotide bases on the device (the containment
// test of bubble popping, reference construct_graph.py:2148-2194 and :1567-1575, which call
// sourmash.MinHash(n=0, ksize=K, scaled=S).add_sequence(seq, force=True)).
//
// sourmash is a third-party dependency of the reference (pyproject.toml:28, not vendored); its published sketch
// definition for DNA is implemented here: upper-cased sequence, every window of `ksize` bases without a character
// outside ACGT, canonical form = the bytewise smaller of the k-mer and its reverse complement, hash = first 64 bits of
// MurmurHash3_x64_128(k-mer, seed 42), kept when hash <= max_hash (km_max_hash, amg_bases.h).
//
//   amg_minhash                the (set, hash) pairs of host segments: k_minhash, one thread per k-mer start on
//                              base_tile (amg_bases.h), the survivors compacted by block_emit.  Algorithmic traffic:
//                              1 byte read per base, 12 bytes written per kept hash (1/scaled of them): an HBM stream,
//                              integer work only.
//   amg_seqs_create            the reads' nucleotide sequences resident in HBM (uploaded once per cleaning run, not once
//                              per sketch call; amg_kcount.hip counts the k-mers of the same bases).
//   amg_path_sketch_overlaps   the node sketches (:2148-2158: ksize 11, scaled 10, of the stretch of every read under
//                              every occurrence of the node), their unions per path (:1747-1751) and the number of
//                              hashes two paths share (:1775-1786), for every pair the caller lists: windows -> segments
//                              -> k_bs_hash (one wave per segment, straight from the resident bases) -> (path, hash)
//                              pairs -> two stable radix sorts -> one binary search per hash of the first path of a pair.
#include "amg_bases.h"

#include <algorithm>

#define MH_MAX_K KM_MAX_K

// the device buffers of amg_path_sketch_overlaps, kept from call to call
struct SketchState {
  DevBuf path_off, path_node, pair_a, pair_b, ncnt, noff, ncur, nlist, segs, out_p, out_h, srt_h, srt_p, srt_i, iota, h2,
      size, pstart, common, row_seq, seg_cnt, seg_base;
};

void sketch_release(amg_ctx* c) {
  if (!c->sk) return;
  SketchState* b = c->sk;
  DevBuf* all[] = {&b->path_off, &b->path_node, &b->pair_a, &b->pair_b, &b->ncnt, &b->noff, &b->ncur, &b->nlist,
                   &b->segs, &b->out_p, &b->out_h, &b->srt_h, &b->srt_p, &b->srt_i, &b->iota, &b->h2, &b->size,
                   &b->pstart, &b->common, &b->row_seq, &b->seg_cnt, &b->seg_base};
  for (DevBuf* d : all) d->release();
  delete b;
  c->sk = nullptr;
}

// ------------------------------------------------------------------ sketches of host segments
template <int NW>  // words of a k-mer: (ksize + 7) / 8
__global__ __launch_bounds__(256) void k_minhash(BaseStream s, const int* __restrict__ seg_set, int ksize,
                                                 unsigned long long max_hash, unsigned long long* counter, long long cap,
                                                 int* __restrict__ out_set, unsigned long long* __restrict__ out_hash) {
  BaseWin w;
  base_tile<false, km_canonical_hash<NW>>(s, ksize, (long long)blockIdx.x * BT_TILE, w);
  int set[4];
  unsigned int keep = 0;
#pragma unroll
  for (int it = 0; it < 4; ++it)
    if (w.valid[it] && w.key[it] <= max_hash) {  // force=True: windows with other characters are skipped
      set[it] = seg_set[w.seg[it]];
      keep |= 1u << it;
    }
  block_emit(keep, counter, cap, [&](unsigned long long o, int it) {
    out_set[o] = set[it];
    out_hash[o] = w.key[it];
  });
}

// Hashes of every valid k-mer of every segment that pass the scaled cut, one (set id, hash) pair per
// k-mer occurrence, in no particular order (the caller makes sets of them).  bases / seg_off /
// seg_set are HOST arrays; *n_out = number of pairs; out_set / out_hash (host, capacity cap) may be
// NULL to get the count only.  scaled = 1 keeps every hash.
extern "C" int amg_minhash(amg_ctx* c, const uint8_t* bases, const int64_t* seg_off, const int32_t* seg_set,
                           int64_t n_seg, int32_t ksize, uint64_t scaled, int32_t* out_set, uint64_t* out_hash,
                           int64_t cap, int64_t* n_out) {
  if (!c || !n_out) return amg_fail(AMG_E_ARG, "null argument");
  if (ksize < 1 || ksize > MH_MAX_K) return amg_fail(AMG_E_ARG, "ksize must be in [1, %d]", MH_MAX_K);
  if (n_seg < 0 || (n_seg > 0 && (!bases || !seg_off || !seg_set))) return amg_fail(AMG_E_ARG, "bad segments");
  *n_out = 0;
  if (n_seg == 0) return AMG_OK;
  const int64_t n_bases = seg_off[n_seg];
  AMGCHK(offsets_check(seg_off, n_seg, "seg_off[0] must be 0", "seg_off not monotone"));
  if (n_bases == 0) return AMG_OK;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  if (scaled == 0) return amg_fail(AMG_E_ARG, "scaled must be >= 1");
  // upper bound of the output: every k-mer start (scaled == 1) or a generous share of them
  const int64_t want = (out_set && out_hash) ? cap : 0;
  DevBuf &d_b = c->s0, &d_off = c->s1, &d_set = c->s2, &d_os = c->s3, &d_oh = c->s4;
  AMGCHK(d_b.ensure((size_t)n_bases + 64));
  AMGCHK(d_off.ensure((size_t)(n_seg + 1) * sizeof(long long)));
  AMGCHK(d_set.ensure((size_t)(n_seg + 1) * sizeof(int)));
  AMGCHK(d_os.ensure((size_t)(want + 1) * sizeof(int)));
  AMGCHK(d_oh.ensure((size_t)(want + 1) * sizeof(unsigned long long)));
  HIPCHK(hipMemcpyAsync(d_b.p, bases, (size_t)n_bases, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_off.p, seg_off, (size_t)(n_seg + 1) * sizeof(long long), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_set.p, seg_set, (size_t)n_seg * sizeof(int), hipMemcpyHostToDevice, st));
  unsigned long long* ctr = c->status.as<unsigned long long>() + ST_MISC;
  HIPCHK(hipMemsetAsync(ctr, 0, sizeof(unsigned long long), st));
  stages_reset(c);
  stage_begin(c, "minhash");
  const BaseStream src{d_b.as<unsigned char>(), (long long)n_bases, d_off.as<long long>(), (long long)n_seg, nullptr};
  hipLaunchKernelGGL(KM_BY_WORDS(ksize, &k_minhash<NW>), dim3(nblk(n_bases, BT_TILE)), dim3(256), 0, st, src,
                     d_set.as<int>(), (int)ksize, km_max_hash(scaled), ctr, (long long)want, d_os.as<int>(),
                     d_oh.as<unsigned long long>());
  stage_end(c);
  unsigned long long n = 0;
  HIPCHK(hipMemcpyAsync(&n, ctr, sizeof(n), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  *n_out = (int64_t)n;
  if (want > 0) {
    const int64_t m = (int64_t)n < want ? (int64_t)n : want;
    HIPCHK(hipMemcpyAsync(out_set, d_os.p, (size_t)m * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(out_hash, d_oh.p, (size_t)m * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  return AMG_OK;
}

// ------------------------------------------------------------------ the reads' bases, resident
extern "C" int amg_seqs_create(int32_t device, const char* const* seq, const int64_t* len, int64_t n, amg_seqs** out) {
  if (!out || n < 0 || (n > 0 && (!seq || !len))) return amg_fail(AMG_E_ARG, "bad argument");
  *out = nullptr;
  HIPCHK(hipSetDevice(device));
  std::vector<long long> off((size_t)n + 1, 0);
  for (int64_t i = 0; i < n; ++i) {
    if (len[i] < 0 || (len[i] > 0 && !seq[i])) return amg_fail(AMG_E_ARG, "sequence %lld: bad length or pointer", (long long)i);
    off[(size_t)i + 1] = off[(size_t)i] + len[i];
  }
  amg_seqs* s = new amg_seqs();
  s->device = device;
  s->n = n;
  s->total = off[(size_t)n];
  auto fail = [&](int r) {
    s->bases.release();
    s->off.release();
    delete s;
    return r;
  };
  if (s->bases.ensure((size_t)s->total + 256) != AMG_OK) return fail(AMG_E_NOMEM);
  if (s->off.ensure((size_t)(n + 2) * sizeof(long long)) != AMG_OK) return fail(AMG_E_NOMEM);
  // two pinned buffers take turns: the host fills one while the other is on its way
  const size_t CH = (size_t)32 << 20;
  char* pin[2] = {nullptr, nullptr};
  hipStream_t st = nullptr;
  hipEvent_t ev[2] = {nullptr, nullptr};
  hipError_t e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
  for (int i = 0; i < 2 && e == hipSuccess; ++i) {
    e = hipHostMalloc(reinterpret_cast<void**>(&pin[i]), CH, hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ev[i], hipEventDisableTiming);
  }
  int which = 0;
  bool in_flight[2] = {false, false};
  size_t fill = 0;
  long long dst = 0;
  auto flush = [&]() -> hipError_t {
    if (fill == 0) return hipSuccess;
    hipError_t r = hipMemcpyAsync(s->bases.as<char>() + dst, pin[which], fill, hipMemcpyHostToDevice, st);
    if (r != hipSuccess) return r;
    r = hipEventRecord(ev[which], st);
    in_flight[which] = true;
    dst += (long long)fill;
    fill = 0;
    which ^= 1;
    if (r == hipSuccess && in_flight[which]) {
      r = hipEventSynchronize(ev[which]);
      in_flight[which] = false;
    }
    return r;
  };
  for (int64_t i = 0; i < n && e == hipSuccess; ++i) {
    size_t done = 0;
    const size_t L = (size_t)len[i];
    while (done < L && e == hipSuccess) {
      const size_t take = std::min(L - done, CH - fill);
      memcpy(pin[which] + fill, seq[i] + done, take);
      fill += take;
      done += take;
      if (fill == CH) e = flush();
    }
  }
  if (e == hipSuccess) e = flush();
  if (e == hipSuccess) e = hipMemcpyAsync(s->off.p, off.data(), (size_t)(n + 1) * sizeof(long long), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  for (int i = 0; i < 2; ++i) {
    if (pin[i]) (void)hipHostFree(pin[i]);
    if (ev[i]) (void)hipEventDestroy(ev[i]);
  }
  if (st) (void)hipStreamDestroy(st);
  if (e != hipSuccess) return fail(amg_fail(AMG_E_HIP, "amg_seqs_create: %s", hipGetErrorString(e)));
  *out = s;
  return AMG_OK;
}

extern "C" int amg_seqs_destroy(amg_seqs* s) {
  if (!s) return AMG_OK;
  (void)hipSetDevice(s->device);
  s->bases.release();
  s->off.release();
  delete s;
  return AMG_OK;
}

// ------------------------------------------------------------------ sketches of paths and what two of them share
struct BsSeg {
  long long src;  // first base in the resident stream
  int len;
  int node;
};
static_assert(sizeof(BsSeg) == 16, "segment record");

#define BS_NEG_POS 1ull  // a gene position below zero: Python's slice would count from the end of the read

__global__ void k_bs_mark(const int* __restrict__ path_node, long long n, unsigned int* __restrict__ ncnt) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) atomicAdd(&ncnt[path_node[i]], 1u);
}

// the paths of every node: path p lists node x at some place, x lists p at some place
__global__ void k_bs_fill(const long long* __restrict__ path_off, const int* __restrict__ path_node, long long n_paths,
                          const long long* __restrict__ noff, unsigned int* __restrict__ ncur, int* __restrict__ nlist) {
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_paths) return;
  for (long long i = path_off[p]; i < path_off[p + 1]; ++i) {
    const int x = path_node[i];
    nlist[noff[x] + atomicAdd(&ncur[x], 1u)] = (int)p;
  }
}

// the windows of the reads that sit on a node of some path: sequence[start of the window's first gene : end of its last
// gene + 1] (:2154-2157) with the clipping of a Python slice.  FILL = false counts them.
template <bool FILL>
__global__ __launch_bounds__(256) void k_bs_segs(const int* __restrict__ tok_node, long long n_tokens,
                                                 const long long* __restrict__ read_off, long long n_reads, int k,
                                                 const long long* __restrict__ gs, const long long* __restrict__ ge,
                                                 const unsigned int* __restrict__ ncnt, const int* __restrict__ row_seq,
                                                 const long long* __restrict__ seq_off, long long n_seqs,
                                                 unsigned long long* __restrict__ ctr, BsSeg* __restrict__ segs,
                                                 unsigned long long* __restrict__ flags) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  bool mine = false;
  int node = -1;
  if (t < n_tokens) {
    node = tok_node[t];
    mine = node >= 0 && ncnt[node] != 0u;
  }
  const unsigned long long vote = __ballot(mine);
  if (vote == 0ull) return;
  const int lane = threadIdx.x & 63;
  unsigned long long base = 0;
  if (lane == 0) base = atomicAdd(ctr, (unsigned long long)__popcll(vote));
  base = (unsigned long long)__shfl((long long)base, 0);
  if (!FILL || !mine) return;
  const long long lo = last_offset_le(read_off, 0, n_reads, t);  // the token's read
  const long long si = row_seq ? (long long)row_seq[lo] : lo;
  BsSeg s;
  s.node = node;
  s.src = 0;
  s.len = 0;
  if (si >= 0 && si < n_seqs) {
    const long long a = gs[t], b = ge[t + k - 1] + 1;
    if (a < 0 || b < 0) atomicOr(flags, BS_NEG_POS);
    const long long L = seq_off[si + 1] - seq_off[si];
    const long long x = a < L ? a : L, y = b < L ? b : L;
    if (a >= 0 && b >= 0 && y > x) {
      s.src = seq_off[si] + x;
      s.len = (int)(y - x > 0x7fffffffll ? 0x7fffffffll : y - x);
    }
  } else {
    atomicOr(flags, BS_NEG_POS << 1);
  }
  segs[base + (unsigned long long)__popcll(vote & ((1ull << lane) - 1ull))] = s;
}

#define BS_CHUNK 1024
#define BS_MAX_K KM_MAX_K
#define BS_WPB 4

// One WAVE per segment: the segment goes through the wave's slab of LDS a chunk at a time (k - 1 bases of overlap), lane
// i hashes the k-mers that start at i, i + 64, ...; a hash that passes the scaled cut is one (path, hash) pair for every
// path that lists the segment's node.  EMIT = false counts the pairs of every segment (seg_cnt), EMIT = true writes them
// behind the segment's own offset (seg_base = the prefix sums of the counts): no counter is shared between waves — one
// returning atomic per wave and round on a single word was five sixths of this kernel's time.
template <bool EMIT, int NW>  // NW: words of a k-mer, (ksize + 7) / 8 (amg_bases.h)
__global__ __launch_bounds__(64 * BS_WPB) void k_bs_hash(const BsSeg* __restrict__ segs, long long n_segs,
                                                         const unsigned char* __restrict__ bases, int ksize,
                                                         unsigned long long max_hash, const long long* __restrict__ noff,
                                                         const int* __restrict__ nlist, long long* __restrict__ seg_cnt,
                                                         const long long* __restrict__ seg_base,
                                                         long long cap, unsigned int* __restrict__ out_p,
                                                         unsigned long long* __restrict__ out_h) {
  __shared__ __attribute__((aligned(8))) unsigned char s_b[BS_WPB][BS_CHUNK + BS_MAX_K + 24];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long si = (long long)blockIdx.x * BS_WPB + wv;
  if (si >= n_segs) return;
  const BsSeg sg = segs[si];
  const long long n0 = noff[sg.node];
  const int n_paths = (int)(noff[sg.node + 1] - n0);
  unsigned long long counted = EMIT ? (unsigned long long)seg_base[si] : 0ull;
  unsigned char* sb = s_b[wv];
  for (int c0 = 0; c0 + ksize <= sg.len; c0 += BS_CHUNK) {
    const int have = min(sg.len - c0, BS_CHUNK + ksize - 1);
    for (int i = lane; i < have + 24; i += 64) sb[i] = i < have ? km_stage(bases[sg.src + c0 + i]) : (unsigned char)0;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int starts = have - ksize + 1;
    for (int i0 = 0; i0 < starts; i0 += 64) {
      const int i = i0 + lane;
      bool keep = false;
      unsigned long long hv = 0;
      if (i < starts) keep = km_canonical_hash<NW>(sb, i, ksize, &hv) && hv <= max_hash;
      const unsigned long long vote = __ballot(keep);
      if (vote == 0ull) continue;
      const unsigned long long n_keep = (unsigned long long)__popcll(vote);
      const unsigned long long base = counted;
      counted += n_keep * (unsigned long long)n_paths;
      if (!EMIT) continue;
      if (keep) {
        unsigned long long o = base + (unsigned long long)__popcll(vote & ((1ull << lane) - 1ull)) * (unsigned long long)n_paths;
        for (int q = 0; q < n_paths; ++q, ++o)
          if ((long long)o < cap) {
            out_p[o] = (unsigned int)nlist[n0 + q];
            out_h[o] = hv;
          }
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  if (!EMIT && lane == 0) seg_cnt[si] = (long long)counted;
}

__global__ void k_bs_iota(unsigned int* __restrict__ v, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) v[i] = (unsigned int)i;
}

// after the two sorts: pairs in (path, hash) order.  The first pair of a run of equal ones stands for the hash in the
// path's sketch; a path's sketch size is the number of its runs.
__global__ void k_bs_unique(const unsigned int* __restrict__ sp, const unsigned int* __restrict__ si,
                            const unsigned long long* __restrict__ h1, long long n, unsigned long long* __restrict__ h2,
                            unsigned long long* __restrict__ size) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  bool first = false;
  unsigned int p = 0xffffffffu;
  if (i < n) {
    const unsigned long long h = h1[si[i]];
    h2[i] = h;
    p = sp[i];
    first = i == 0 || sp[i - 1] != p || h1[si[i - 1]] != h;
  }
  // a path's pairs are thousands in a row: nearly every wave sits inside ONE path and adds its count once
  const unsigned int p0 = (unsigned int)__shfl((int)p, 0);
  const unsigned long long firsts = __ballot(first);
  if (__ballot(p != p0 && i < n) == 0ull) {
    if ((threadIdx.x & 63) == 0 && firsts) atomicAdd(&size[p0], (unsigned long long)__popcll(firsts));
  } else if (first) {
    atomicAdd(&size[p], 1ull);
  }
}

__global__ void k_bs_pstart(const unsigned int* __restrict__ sp, long long n, long long n_paths, long long* __restrict__ pstart) {
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p > n_paths) return;
  long long lo = 0, hi = n;  // first i with sp[i] >= p
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if ((long long)sp[mid] < p) lo = mid + 1; else hi = mid;
  }
  pstart[p] = lo;
}

// |sketch(a) & sketch(b)| for one pair per workgroup: every distinct hash of a is looked up in b's stretch
__global__ __launch_bounds__(256) void k_bs_common(const int* __restrict__ pair_a, const int* __restrict__ pair_b,
                                                   const long long* __restrict__ pstart, const unsigned long long* __restrict__ h2,
                                                   unsigned long long* __restrict__ common) {
  __shared__ unsigned long long s_sum[4];
  const long long q = blockIdx.x;
  const int a = pair_a[q], b = pair_b[q];
  const long long a0 = pstart[a], a1 = pstart[a + 1], b0 = pstart[b], b1 = pstart[b + 1];
  unsigned long long mine = 0;
  for (long long i = a0 + threadIdx.x; i < a1; i += 256) {
    const unsigned long long h = h2[i];
    if (i > a0 && h2[i - 1] == h) continue;
    long long lo = b0, hi = b1;
    while (lo < hi) {
      const long long mid = (lo + hi) >> 1;
      if (h2[mid] < h) lo = mid + 1; else hi = mid;
    }
    if (lo < b1 && h2[lo] == h) ++mine;
  }
  for (int o = 32; o > 0; o >>= 1) mine += (unsigned long long)__shfl_down((long long)mine, o);
  if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0) common[q] = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
}

extern "C" int amg_path_sketch_overlaps(amg_ctx* c, const amg_seqs* seqs, const int32_t* row_to_seq, int32_t ksize,
                                        uint64_t scaled, int64_t n_paths, const int64_t* path_off, const int32_t* path_node,
                                        int64_t n_pairs, const int32_t* pair_a, const int32_t* pair_b, int64_t* sketch_size,
                                        int64_t* common) {
  NEED_BUILT(c);
  if (!seqs || n_paths < 0 || n_pairs < 0 || (n_paths > 0 && (!path_off || !sketch_size)) ||
      (n_pairs > 0 && (!pair_a || !pair_b || !common)))
    return amg_fail(AMG_E_ARG, "bad argument");
  if (seqs->device != c->device) return amg_fail(AMG_E_ARG, "the sequences live on another device");
  if (ksize < 1 || ksize > BS_MAX_K) return amg_fail(AMG_E_ARG, "ksize must be in [1, %d]", BS_MAX_K);
  if (scaled == 0) return amg_fail(AMG_E_ARG, "scaled must be >= 1");
  if (!c->have_pos || !c->pos_identity) return amg_fail(AMG_E_STATE, "gene positions of the graph's reads are needed (amg_set_positions)");
  if (n_paths == 0) return AMG_OK;
  const long long D = c->n_nodes, T = c->n_tokens, R = c->n_reads;
  const long long N = path_off[n_paths];
  if (N < 0 || (N > 0 && !path_node)) return amg_fail(AMG_E_ARG, "bad path offsets");
  AMGCHK(offsets_check(path_off, n_paths, "bad path offsets", "path offsets not monotone"));
  for (long long i = 0; i < N; ++i)
    if (path_node[i] < 0 || path_node[i] >= D) return amg_fail(AMG_E_ARG, "path node %d outside the graph", path_node[i]);
  for (int64_t q = 0; q < n_pairs; ++q)
    if (pair_a[q] < 0 || pair_a[q] >= n_paths || pair_b[q] < 0 || pair_b[q] >= n_paths)
      return amg_fail(AMG_E_ARG, "pair %lld names a path that is not there", (long long)q);
  if (row_to_seq == nullptr && seqs->n < R) return amg_fail(AMG_E_ARG, "fewer sequences than reads");
  const unsigned long long max_hash = km_max_hash(scaled);
  if (!c->sk) c->sk = new SketchState();
  SketchState* b = c->sk;
  hipStream_t st = c->stream;
  stages_reset(c);
  stage_begin(c, "path_sketches");
  for (int64_t p = 0; p < n_paths; ++p) sketch_size[p] = 0;
  for (int64_t q = 0; q < n_pairs; ++q) common[q] = 0;
  AMGCHK(b->path_off.ensure((size_t)(n_paths + 2) * sizeof(long long)));
  AMGCHK(b->path_node.ensure((size_t)(N + 2) * sizeof(int)));
  AMGCHK(b->pair_a.ensure((size_t)(n_pairs + 2) * sizeof(int)));
  AMGCHK(b->pair_b.ensure((size_t)(n_pairs + 2) * sizeof(int)));
  AMGCHK(b->ncnt.ensure((size_t)(D + 2) * sizeof(unsigned int)));
  AMGCHK(b->ncur.ensure((size_t)(D + 2) * sizeof(unsigned int)));
  AMGCHK(b->noff.ensure((size_t)(D + 2) * sizeof(long long)));
  AMGCHK(b->nlist.ensure((size_t)(N + 2) * sizeof(int)));
  AMGCHK(b->size.ensure((size_t)(n_paths + 2) * sizeof(unsigned long long)));
  AMGCHK(b->pstart.ensure((size_t)(n_paths + 2) * sizeof(long long)));
  AMGCHK(b->common.ensure((size_t)(n_pairs + 2) * sizeof(unsigned long long)));
  HIPCHK(hipMemcpyAsync(b->path_off.p, path_off, (size_t)(n_paths + 1) * sizeof(long long), hipMemcpyHostToDevice, st));
  if (N) HIPCHK(hipMemcpyAsync(b->path_node.p, path_node, (size_t)N * sizeof(int), hipMemcpyHostToDevice, st));
  if (n_pairs) {
    HIPCHK(hipMemcpyAsync(b->pair_a.p, pair_a, (size_t)n_pairs * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(b->pair_b.p, pair_b, (size_t)n_pairs * sizeof(int), hipMemcpyHostToDevice, st));
  }
  const int* d_row_seq = nullptr;
  if (row_to_seq) {
    AMGCHK(b->row_seq.ensure((size_t)(R + 2) * sizeof(int)));
    HIPCHK(hipMemcpyAsync(b->row_seq.p, row_to_seq, (size_t)R * sizeof(int), hipMemcpyHostToDevice, st));
    d_row_seq = b->row_seq.as<int>();
  }
  unsigned long long* ctr = c->status.as<unsigned long long>() + ST_COMPACT_A;  // [0] segments, [1] pairs
  unsigned long long* flags = c->status.as<unsigned long long>() + ST_MISC;
  {
    ClearList cl;
    cl.add(b->ncnt.p, (size_t)(D + 2) * sizeof(unsigned int));
    cl.add(b->ncur.p, (size_t)(D + 2) * sizeof(unsigned int));
    cl.add(b->size.p, (size_t)(n_paths + 2) * sizeof(unsigned long long));
    cl.add(ctr, 2 * sizeof(unsigned long long));
    cl.add(flags, sizeof(unsigned long long));
    AMGCHK(clear_many(c, cl));
  }
  auto finish = [&]() -> int {  // sizes and overlaps to the caller
    HIPCHK(hipMemcpyAsync(sketch_size, b->size.p, (size_t)n_paths * sizeof(long long), hipMemcpyDeviceToHost, st));
    stage_end(c);
    HIPCHK(hipStreamSynchronize(st));
    return AMG_OK;
  };
  if (N == 0) return finish();
  hipLaunchKernelGGL(k_bs_mark, dim3(nblk(N, 256)), dim3(256), 0, st, b->path_node.as<int>(), N, b->ncnt.as<unsigned int>());
  AMGCHK(prim_exscan_u32_to_i64(c, b->ncnt.as<unsigned int>(), b->noff.as<long long>(), (size_t)D + 1));  // (ncnt[D] = 0: noff[D] = the sum)
  hipLaunchKernelGGL(k_bs_fill, dim3(nblk(n_paths, 64)), dim3(64), 0, st, b->path_off.as<long long>(), b->path_node.as<int>(),
                     (long long)n_paths, b->noff.as<long long>(), b->ncur.as<unsigned int>(), b->nlist.as<int>());
  const long long* gs = c->gene_start.as<long long>();
  const long long* ge = c->gene_end.as<long long>();
  hipLaunchKernelGGL(k_bs_segs<false>, dim3(nblk(T, 256)), dim3(256), 0, st, c->tok_node.as<int>(), T,
                     c->read_off.as<long long>(), R, (int)c->k, gs, ge, b->ncnt.as<unsigned int>(), d_row_seq,
                     seqs->off.as<long long>(), (long long)seqs->n, ctr, (BsSeg*)nullptr, flags);
  unsigned long long n_segs = 0;
  {
    FetchList l;
    l.add(ctr);
    ClearList after;
    after.add(ctr, sizeof(unsigned long long));
    AMGCHK(fetch(c, l, &n_segs, &after));
  }
  if (n_segs == 0) return finish();
  AMGCHK(b->segs.ensure((size_t)(n_segs + 1) * sizeof(BsSeg)));
  hipLaunchKernelGGL(k_bs_segs<true>, dim3(nblk(T, 256)), dim3(256), 0, st, c->tok_node.as<int>(), T,
                     c->read_off.as<long long>(), R, (int)c->k, gs, ge, b->ncnt.as<unsigned int>(), d_row_seq,
                     seqs->off.as<long long>(), (long long)seqs->n, ctr, b->segs.as<BsSeg>(), flags);
  // pairs per segment -> where every segment's pairs go
  AMGCHK(b->seg_cnt.ensure((size_t)(n_segs + 2) * sizeof(long long)));
  AMGCHK(b->seg_base.ensure((size_t)(n_segs + 2) * sizeof(long long)));
  {
    ClearList cl;
    cl.add(b->seg_cnt.as<long long>() + n_segs, sizeof(long long));
    AMGCHK(clear_many(c, cl));
  }
  auto count_kernel = KM_BY_WORDS(ksize, (&k_bs_hash<false, NW>));
  auto emit_kernel = KM_BY_WORDS(ksize, (&k_bs_hash<true, NW>));
  hipLaunchKernelGGL(count_kernel, dim3(nblk((long long)n_segs, BS_WPB)), dim3(64 * BS_WPB), 0, st, b->segs.as<BsSeg>(),
                     (long long)n_segs, seqs->bases.as<unsigned char>(), (int)ksize, max_hash, b->noff.as<long long>(),
                     b->nlist.as<int>(), b->seg_cnt.as<long long>(), (const long long*)nullptr, 0ll, (unsigned int*)nullptr,
                     (unsigned long long*)nullptr);
  AMGCHK(prim_exscan_i64(c, b->seg_cnt.as<long long>(), b->seg_base.as<long long>(), (size_t)n_segs + 1));  // (seg_cnt[n_segs] = 0)
  unsigned long long got[3] = {0, 0, 0};
  {
    FetchList l;
    l.add(b->seg_base.as<long long>() + n_segs);
    l.add(flags);
    l.add(ctr);
    AMGCHK(fetch(c, l, got));
  }
  if (got[2] != n_segs) {  // (both passes over the windows must have seen the same)
    stage_end(c);
    return amg_fail(AMG_E_OVERFLOW, "path sketches: %llu of %llu segments written", got[2], n_segs);
  }
  if (got[1] & BS_NEG_POS) {
    stage_end(c);
    return amg_fail(AMG_E_ARG, "a gene position below zero");
  }
  if (got[1] & (BS_NEG_POS << 1)) {
    stage_end(c);
    return amg_fail(AMG_E_ARG, "a read without a sequence (row_to_seq)");
  }
  const long long M = (long long)got[0];
  if (M == 0) return finish();
  long long max_pairs = 1ll << 30;  // (40 bytes of buffers per pair; the sorts index pairs with 32 bits)
  if (const char* e = getenv("AMG_TEST_SKETCH_PAIRS")) max_pairs = atoll(e);  // test hook: callers split their paths
  if (M >= max_pairs) {
    stage_end(c);
    return amg_fail(AMG_E_NOMEM, "%lld (path, hash) pairs in one call: split the paths", M);
  }
  AMGCHK(b->out_p.ensure((size_t)(M + 1) * sizeof(unsigned int)));
  AMGCHK(b->out_h.ensure((size_t)(M + 1) * sizeof(unsigned long long)));
  AMGCHK(b->srt_h.ensure((size_t)(M + 1) * sizeof(unsigned long long)));
  AMGCHK(b->srt_p.ensure((size_t)(M + 1) * sizeof(unsigned int)));
  AMGCHK(b->srt_i.ensure((size_t)(M + 1) * sizeof(unsigned int)));
  AMGCHK(b->iota.ensure((size_t)(M + 1) * sizeof(unsigned int)));
  AMGCHK(b->h2.ensure((size_t)(M + 1) * sizeof(unsigned long long)));
  hipLaunchKernelGGL(emit_kernel, dim3(nblk((long long)n_segs, BS_WPB)), dim3(64 * BS_WPB), 0, st, b->segs.as<BsSeg>(),
                     (long long)n_segs, seqs->bases.as<unsigned char>(), (int)ksize, max_hash, b->noff.as<long long>(),
                     b->nlist.as<int>(), (long long*)nullptr, b->seg_base.as<long long>(), M, b->out_p.as<unsigned int>(),
                     b->out_h.as<unsigned long long>());
  // (path, hash) order by two stable sorts: by hash, then by path
  AMGCHK(prim_sort_u64_u32(c, b->out_h.as<unsigned long long>(), b->srt_h.as<unsigned long long>(), b->out_p.as<unsigned int>(),
                           b->srt_p.as<unsigned int>(), (size_t)M, 64));
  hipLaunchKernelGGL(k_bs_iota, dim3(nblk(M, 256)), dim3(256), 0, st, b->iota.as<unsigned int>(), M);
  AMGCHK(prim_sort_u32_u32(c, b->srt_p.as<unsigned int>(), b->out_p.as<unsigned int>(), b->iota.as<unsigned int>(),
                           b->srt_i.as<unsigned int>(), (size_t)M, ilog2_ceil((uint64_t)n_paths + 1) + 1));
  hipLaunchKernelGGL(k_bs_unique, dim3(nblk(M, 256)), dim3(256), 0, st, b->out_p.as<unsigned int>(), b->srt_i.as<unsigned int>(),
                     b->srt_h.as<unsigned long long>(), M, b->h2.as<unsigned long long>(), b->size.as<unsigned long long>());
  hipLaunchKernelGGL(k_bs_pstart, dim3(nblk(n_paths + 1, 256)), dim3(256), 0, st, b->out_p.as<unsigned int>(), M,
                     (long long)n_paths, b->pstart.as<long long>());
  if (n_pairs) {
    hipLaunchKernelGGL(k_bs_common, dim3((unsigned int)n_pairs), dim3(256), 0, st, b->pair_a.as<int>(), b->pair_b.as<int>(),
                       b->pstart.as<long long>(), b->h2.as<unsigned long long>(), b->common.as<unsigned long long>());
    HIPCHK(hipMemcpyAsync(common, b->common.p, (size_t)n_pairs * sizeof(long long), hipMemcpyDeviceToHost, st));
  }
  return finish();
}
