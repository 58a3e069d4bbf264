// amg_kcount.hip — canonical nucleotide k-mer counts on the device: the counts, histogram and per-read-set medians
// that estimate_copy_numbers (reference result_utils.py:1089-1159, with estimate_overall_read_depth :1050-1080) gets
// from four calls of the external tool jellyfish.
//
// jellyfish is not part of the reference's tree, and it exists neither where this unit is built nor where it runs, so
// what follows RESTATES its documented behaviour (as amg_sketch.hip restates sourmash's) and nobody has checked the
// restatement against the tool itself:
//   count -m k -C   every window of k bases of every sequence is counted, upper and lower case alike; a window that
//                   holds a character outside ACGT is skipped; no window spans two sequences; a k-mer and its reverse
//                   complement are ONE key (which of the two stands for the pair is not observable here)
//   histo           bin v (1 <= v <= 10 000) = distinct keys counted exactly v times, bin 10 001 = those counted more
//                   often; with a minimum count m (count's -L m) keys counted fewer than m times are absent
//   query -s        one count per valid window occurrence of the queried sequences, 0 for an absent key
// k is 1 .. 31: two bits per base in one 64-bit key, all-ones stays free as the empty mark.
//
// Table: open addressing, linear probing, a power of two of slots; keys are 8-byte words claimed by one 64-bit
// compare-and-swap, counts 32-bit words in an array of their own bumped by an atomicAdd whose result nobody reads.
// Every probe loop is bounded by the number of slots; an insert that finds no place raises a status word and the call
// fails with AMG_E_NOMEM ("k-mer table full") instead of spinning.
//
// Insert, query and emit walk their bases with base_tile (amg_bases.h: the stream, the tile, the search, the
// compaction of k_kc_emit's records); their key is kc_key: the k-mer cut out of LDS as words and packed to two bits
// per base, (c >> 1) & 3 gives A 0, C 1, T 2, G 3, and the complement is ^ 2.  This unit holds that key, the table
// (kc_upsert, kc_find), the tally, the histogram, the medians' pick and the host calls.
// Traffic of the count pass: 1 byte per base read (a stream) + one 64-byte sector per probe + one per add (random).
#include "amg_bases.h"

#define KC_MAX_K 31
#define KC_EMPTY (~0ull)
#define KC_BINS 10002  // bins 0 .. 10 001 of a histogram (bin 0 stays empty)

struct amg_kcount {
  int device = 0;
  int k = 0;
  int64_t slots = 0, windows = 0, distinct = 0;
  DevBuf keys, counts;  // uint64[slots], uint32[slots]
  // scratch of amg_kcount_medians (the handle is const to its readers; a ctx is not thread-safe, nor is this)
  mutable DevBuf m_row, m_set, m_len, m_src, m_off, m_key, m_srt, m_v0, m_v1, m_out;
};

// eight staged bases (a byte each) -> sixteen bits, first base lowest
__device__ __forceinline__ unsigned long long kc_pack8(unsigned long long w) {
  unsigned long long x = (w >> 1) & 0x0303030303030303ull;
  x = (x | (x >> 6)) & 0x000F000F000F000Full;
  x = (x | (x >> 12)) & 0x000000FF000000FFull;
  x = (x | (x >> 24)) & 0xFFFFull;
  return x;
}

// the canonical key of the k-mer at byte i of the staged bases: the smaller of the packed k-mer and its packed
// reverse complement; false: a base outside ACGT among the k
template <int NW>
__device__ __forceinline__ bool kc_key(const unsigned char* lds, int i, int k, unsigned long long* key) {
  unsigned long long f[NW];
  if (!km_load<NW>(lds, i, k, f)) return false;
  unsigned long long x = 0ull;
#pragma unroll
  for (int j = 0; j < NW; ++j) x |= kc_pack8(f[j]) << (16 * j);
  // the 32 two-bit groups in reverse order (a bit reversal, then the two bits of every group swapped back), the
  // 32 - k groups of padding shifted out, every base complemented
  unsigned long long r = __brevll(x);
  r = ((r >> 1) & 0x5555555555555555ull) | ((r & 0x5555555555555555ull) << 1);
  const int sh = 64 - 2 * k;  // 2 .. 62
  r = (r >> sh) ^ (0xAAAAAAAAAAAAAAAAull >> sh);
  *key = x < r ? x : r;
  return true;
}

// `add` occurrences of `key` into the table.  The slot's key is read with a plain load first: at sequencing depth
// most windows find their key in place, and a stale read can only show an empty slot, which the compare-and-swap then
// puts right (a slot's key never changes once set).
__device__ __forceinline__ void kc_upsert(unsigned long long* keys, unsigned int* counts, unsigned long long mask,
                                          unsigned long long key, unsigned int add, unsigned long long* full) {
  unsigned long long idx = km_fmix(key) & mask;
  for (unsigned long long p = 0; p <= mask; ++p) {
    // once any thread has found the table full the others stop walking it
    if ((p & 63ull) == 63ull && *reinterpret_cast<const volatile unsigned long long*>(full)) return;
    unsigned long long cur = keys[idx];
    if (cur == KC_EMPTY) {
      cur = atomicCAS(&keys[idx], KC_EMPTY, key);
      if (cur == KC_EMPTY) cur = key;
    }
    if (cur == key) {
      atomicAdd(&counts[idx], add);
      return;
    }
    idx = (idx + 1ull) & mask;
  }
  atomicOr(full, 1ull);
}

__device__ __forceinline__ unsigned int kc_find(const unsigned long long* __restrict__ keys,
                                                const unsigned int* __restrict__ counts, unsigned long long mask,
                                                unsigned long long key) {
  unsigned long long idx = km_fmix(key) & mask;
  for (unsigned long long p = 0; p <= mask; ++p) {
    const unsigned long long cur = keys[idx];
    if (cur == key) return counts[idx];
    if (cur == KC_EMPTY) return 0u;
    idx = (idx + 1ull) & mask;
  }
  return 0u;
}

// FOLD: consecutive windows of a homopolymer or a short-period repeat carry the same key, and a wave holds 64
// consecutive windows: the first lane of every run of equal keys adds the run's length, the others add nothing
// (tens of thousands of adds on one word would otherwise queue up at the rate one word takes them).
template <int NW, bool FOLD>
__global__ __launch_bounds__(256) void k_kc_insert(BaseStream s, int k, unsigned long long* keys, unsigned int* counts,
                                                   unsigned long long mask, unsigned long long* full) {
  BaseWin w;
  base_tile<false, kc_key<NW>>(s, k, (long long)blockIdx.x * BT_TILE, w);
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    unsigned int add = w.valid[it] ? 1u : 0u;
    if (FOLD) {
      const unsigned long long prev = (unsigned long long)__shfl_up((long long)w.key[it], 1, 64);
      const int prev_valid = __shfl_up((int)w.valid[it], 1, 64);
      const bool head = w.valid[it] && (lane == 0 || !prev_valid || prev != w.key[it]);
      const unsigned long long heads = __ballot(head), live = __ballot(w.valid[it]);
      // the run of a head ends before the next head or the next lane without a window
      const unsigned long long stop = (heads | ~live) & ~((2ull << lane) - 1ull);
      const int end = stop ? __ffsll((long long)stop) - 1 : 64;
      add = head ? (unsigned int)(end - lane) : 0u;
    }
    if (add) kc_upsert(keys, counts, mask, w.key[it], add, full);
  }
}

// out[t] = count of the k-mer that starts at stream position t (0: absent or below min_count), -1: no valid window
template <int NW>
__global__ __launch_bounds__(256) void k_kc_query(BaseStream s, int k, const unsigned long long* __restrict__ keys,
                                                  const unsigned int* __restrict__ counts, unsigned long long mask,
                                                  unsigned int min_count, long long* __restrict__ out) {
  const long long t0 = (long long)blockIdx.x * BT_TILE;
  BaseWin w;
  base_tile<false, kc_key<NW>>(s, k, t0, w);
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const long long t = t0 + threadIdx.x + it * 256;
    if (t >= s.n_bases) continue;
    long long v = -1;
    if (w.valid[it]) {
      const unsigned int cnt = kc_find(keys, counts, mask, w.key[it]);
      v = cnt >= min_count ? (long long)cnt : 0ll;
    }
    out[t] = v;
  }
}

// (set << 32 | count) of every valid window of a GATHERED stream whose count is >= min_count (>= 1), unordered
// (block_emit: nothing is written at or beyond cap, *counter says how many there were)
template <int NW>
__global__ __launch_bounds__(256) void k_kc_emit(BaseStream s, int k, const unsigned long long* __restrict__ keys,
                                                 const unsigned int* __restrict__ counts, unsigned long long mask,
                                                 unsigned int min_count, const int* __restrict__ seg_set,
                                                 unsigned long long* counter, long long cap,
                                                 unsigned long long* __restrict__ out) {
  BaseWin w;
  base_tile<true, kc_key<NW>>(s, k, (long long)blockIdx.x * BT_TILE, w);
  unsigned long long rec[4];
  unsigned int keep = 0;
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    if (!w.valid[it]) continue;
    const unsigned int cnt = kc_find(keys, counts, mask, w.key[it]);
    if (cnt >= min_count) {
      rec[it] = ((unsigned long long)(unsigned int)seg_set[w.seg[it]] << 32) | cnt;
      keep |= 1u << it;
    }
  }
  block_emit(keep, counter, cap, [&](unsigned long long o, int it) { out[o] = rec[it]; });
}

// sum over the sequences of the windows they can hold: max(len - k + 1, 0)
__global__ __launch_bounds__(256) void k_kc_bound(const long long* __restrict__ off, long long n, int k,
                                                  unsigned long long* out) {
  __shared__ unsigned long long s_sum[4];
  unsigned long long mine = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const long long w = off[i + 1] - off[i] - k + 1;
    if (w > 0) mine += (unsigned long long)w;
  }
  for (int o = 32; o > 0; o >>= 1) mine += (unsigned long long)__shfl_down((long long)mine, o);
  if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = mine;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long t = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
    if (t) atomicAdd(out, t);
  }
}

// out[0] += slots in use, out[1] += the sum of their counts (the windows counted)
__global__ __launch_bounds__(256) void k_kc_tally(const unsigned long long* __restrict__ keys,
                                                  const unsigned int* __restrict__ counts, long long slots,
                                                  unsigned long long* out) {
  __shared__ unsigned long long s_sum[8];
  unsigned long long used = 0, sum = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < slots; i += (long long)gridDim.x * 256)
    if (keys[i] != KC_EMPTY) {
      ++used;
      sum += counts[i];
    }
  for (int o = 32; o > 0; o >>= 1) {
    used += (unsigned long long)__shfl_down((long long)used, o);
    sum += (unsigned long long)__shfl_down((long long)sum, o);
  }
  if ((threadIdx.x & 63) == 0) {
    s_sum[threadIdx.x >> 6] = used;
    s_sum[4 + (threadIdx.x >> 6)] = sum;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long u = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3], t = s_sum[4] + s_sum[5] + s_sum[6] + s_sum[7];
    if (u) atomicAdd(out, u);
    if (t) atomicAdd(out + 1, t);
  }
}

// one pass over the slots: every workgroup fills a histogram of its own in LDS and adds its non-zero bins to the
// 64-bit global ones
__global__ __launch_bounds__(256) void k_kc_histo(const unsigned long long* __restrict__ keys,
                                                  const unsigned int* __restrict__ counts, long long slots,
                                                  unsigned int min_count, unsigned long long* bins) {
  __shared__ unsigned int s_h[KC_BINS];
  for (int i = threadIdx.x; i < KC_BINS; i += 256) s_h[i] = 0u;
  __syncthreads();
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < slots; i += (long long)gridDim.x * 256) {
    if (keys[i] == KC_EMPTY) continue;
    const unsigned int cnt = counts[i];
    if (cnt >= min_count) atomicAdd(&s_h[cnt < (unsigned int)(KC_BINS - 1) ? cnt : (unsigned int)(KC_BINS - 1)], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < KC_BINS; i += 256)
    if (s_h[i]) atomicAdd(&bins[i], (unsigned long long)s_h[i]);
}

// per (set, row) pair: the row's length and where its bases start
__global__ void k_kc_pairs(const long long* __restrict__ row, long long n, const long long* __restrict__ off,
                           long long* __restrict__ len, long long* __restrict__ src) {
  const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p > n) return;
  if (p == n) {
    len[p] = 0;  // (the scan's last output is the total)
    return;
  }
  const long long r = row[p];
  len[p] = off[r + 1] - off[r];
  src[p] = off[r];
}

// srt: the (set << 32 | count) records in ascending order.  Per set: how many, and the two middle ones' counts
__global__ void k_kc_pick(const unsigned long long* __restrict__ srt, long long m, long long n_sets,
                          long long* __restrict__ out /*[3 n_sets]: n, lower middle, upper middle*/) {
  const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_sets) return;
  long long bound[2];
  for (int e = 0; e < 2; ++e) {  // first record of set s + e or a later one
    const unsigned long long want = (unsigned long long)(s + e) << 32;
    long long lo = 0, hi = m;
    while (lo < hi) {
      const long long mid = (lo + hi) >> 1;
      if (srt[mid] < want) lo = mid + 1; else hi = mid;
    }
    bound[e] = lo;
  }
  const long long n = bound[1] - bound[0];
  out[s] = n;
  out[n_sets + s] = n ? (long long)(srt[bound[0] + (n - 1) / 2] & 0xffffffffull) : 0ll;
  out[2 * n_sets + s] = n ? (long long)(srt[bound[0] + n / 2] & 0xffffffffull) : 0ll;
}

// canonical k-mers there are of this k: (4^k + palindromes) / 2, palindromes = 4^(k/2) for even k, none for odd k
static unsigned long long kc_canonical_kmers(int k) {
  const unsigned long long all = 1ull << (2 * k);
  return k % 2 ? all / 2 : (all + (1ull << k)) / 2;
}

static unsigned int kc_grid(long long n) {
  const long long b = (n + 255) / 256;
  return (unsigned int)(b < 1 ? 1 : b > 4096 ? 4096 : b);
}

extern "C" int amg_kcount_create(amg_ctx* c, const amg_seqs* seqs, int32_t k, int32_t slots_log2, amg_kcount** out) {
  if (!c || !seqs || !out) return amg_fail(AMG_E_ARG, "null argument");
  *out = nullptr;
  if (k < 1 || k > KC_MAX_K) return amg_fail(AMG_E_ARG, "k must be in [1, %d]", KC_MAX_K);
  if (slots_log2 < 0 || slots_log2 > 40) return amg_fail(AMG_E_ARG, "slots_log2 must be in [0, 40]");
  if (seqs->device != c->device) return amg_fail(AMG_E_ARG, "the sequences live on another device");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  // [0] windows the sequences can hold, then slots in use; [1] windows counted; [2] the table was full
  unsigned long long* word = c->status.as<unsigned long long>() + ST_COMPACT_A;
  static_assert(ST_COMPACT_A + 2 == ST_MISC, "three status words in a row");
  HIPCHK(hipMemsetAsync(word, 0, 3 * sizeof(unsigned long long), st));
  unsigned long long bound = 0;
  if (seqs->n > 0 && seqs->total > 0) {
    hipLaunchKernelGGL(k_kc_bound, dim3(kc_grid(seqs->n)), dim3(256), 0, st, seqs->off.as<long long>(),
                       (long long)seqs->n, (int)k, word);
    HIPCHK(hipMemcpyAsync(&bound, word, sizeof(bound), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(hipMemsetAsync(word, 0, sizeof(unsigned long long), st));
  }
  if (bound >= (1ull << 32)) return amg_fail(AMG_E_ARG, "%llu windows: fewer than 2^32 can be counted", bound);
  uint64_t slots;
  if (slots_log2 == 0) {
    const unsigned long long kinds = kc_canonical_kmers(k);
    slots = 1ull << ilog2_ceil(2 * (bound < kinds ? bound : kinds));
    if (slots < 2) slots = 2;
  } else {
    slots = 1ull << slots_log2;
  }
  amg_kcount* h = new amg_kcount();
  h->device = c->device;
  h->k = k;
  h->slots = (int64_t)slots;
  auto fail = [&](int r) {
    amg_kcount_destroy(h);
    return r;
  };
  if (h->keys.ensure((size_t)slots * sizeof(unsigned long long)) != AMG_OK) return fail(AMG_E_NOMEM);
  if (h->counts.ensure((size_t)slots * sizeof(unsigned int)) != AMG_OK) return fail(AMG_E_NOMEM);
  hipError_t e = hipMemsetAsync(h->keys.p, 0xff, (size_t)slots * sizeof(unsigned long long), st);
  if (e == hipSuccess) e = hipMemsetAsync(h->counts.p, 0, (size_t)slots * sizeof(unsigned int), st);
  if (e != hipSuccess) return fail(amg_fail(AMG_E_HIP, "amg_kcount_create: %s", hipGetErrorString(e)));
  stages_reset(c);
  unsigned long long got[3] = {0, 0, 0};
  if (bound > 0) {
    const char* sw = getenv("AMG_KCOUNT_FOLD");  // A/B switch: 0 = one add per window
    const bool fold = !(sw && sw[0] == '0');
    const BaseStream src{seqs->bases.as<unsigned char>(), (long long)seqs->total, seqs->off.as<long long>(),
                         (long long)seqs->n, nullptr};
    stage_begin(c, "kcount_insert");
    auto kern = KM_BY_WORDS(k, (fold ? &k_kc_insert<NW, true> : &k_kc_insert<NW, false>));
    hipLaunchKernelGGL(kern, dim3(nblk(seqs->total, BT_TILE)), dim3(256), 0, st, src, (int)k,
                       h->keys.as<unsigned long long>(), h->counts.as<unsigned int>(), (unsigned long long)(slots - 1),
                       word + 2);
    stage_end(c);
    stage_begin(c, "kcount_tally");
    hipLaunchKernelGGL(k_kc_tally, dim3(kc_grid((long long)slots)), dim3(256), 0, st, h->keys.as<unsigned long long>(),
                       h->counts.as<unsigned int>(), (long long)slots, word);
    stage_end(c);
    e = hipMemcpyAsync(got, word, sizeof(got), hipMemcpyDeviceToHost, st);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return fail(amg_fail(AMG_E_HIP, "amg_kcount_create: %s", hipGetErrorString(e)));
  if (got[2]) return fail(amg_fail(AMG_E_NOMEM, "k-mer table full: %llu slots do not hold the keys of %llu windows",
                                   (unsigned long long)slots, bound));
  h->distinct = (int64_t)got[0];
  h->windows = (int64_t)got[1];
  *out = h;
  return AMG_OK;
}

extern "C" int amg_kcount_destroy(amg_kcount* h) {
  if (!h) return AMG_OK;
  (void)hipSetDevice(h->device);
  for (DevBuf* b : {&h->keys, &h->counts, &h->m_row, &h->m_set, &h->m_len, &h->m_src, &h->m_off, &h->m_key, &h->m_srt,
                    &h->m_v0, &h->m_v1, &h->m_out})
    b->release();
  delete h;
  return AMG_OK;
}

extern "C" int amg_kcount_sizes(const amg_kcount* h, int64_t sizes[4]) {
  if (!h || !sizes) return amg_fail(AMG_E_ARG, "null argument");
  sizes[0] = h->k;
  sizes[1] = h->windows;
  sizes[2] = h->distinct;
  sizes[3] = h->slots;
  return AMG_OK;
}

// what a minimum count means to the kernels: m <= 1 is "every key" (a key in the table was counted once at least)
static unsigned int kc_min_count(int64_t m) { return m <= 1 ? 1u : m > 0xffffffffll ? 0xffffffffu : (unsigned int)m; }

extern "C" int amg_kcount_histo(amg_ctx* c, const amg_kcount* h, int64_t min_count, int64_t histo[KC_BINS]) {
  if (!c || !h || !histo) return amg_fail(AMG_E_ARG, "null argument");
  if (h->device != c->device) return amg_fail(AMG_E_ARG, "the k-mer table lives on another device");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  DevBuf& d_bins = c->s0;
  AMGCHK(d_bins.ensure(KC_BINS * sizeof(unsigned long long)));
  HIPCHK(hipMemsetAsync(d_bins.p, 0, KC_BINS * sizeof(unsigned long long), st));
  stages_reset(c);
  stage_begin(c, "kcount_histo");
  // (a workgroup's flush is 10 002 words whatever it saw: few workgroups with many slots each)
  const long long per_block = 256 * 64;
  const long long want = (h->slots + per_block - 1) / per_block;
  hipLaunchKernelGGL(k_kc_histo, dim3((unsigned int)(want < 1 ? 1 : want > 1024 ? 1024 : want)), dim3(256), 0, st,
                     h->keys.as<unsigned long long>(), h->counts.as<unsigned int>(), (long long)h->slots,
                     kc_min_count(min_count), d_bins.as<unsigned long long>());
  stage_end(c);
  static_assert(sizeof(int64_t) == sizeof(unsigned long long), "bins are copied as they are");
  HIPCHK(hipMemcpyAsync(histo, d_bins.p, KC_BINS * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return AMG_OK;
}

extern "C" int amg_kcount_query(amg_ctx* c, const amg_kcount* h, const uint8_t* bases, const int64_t* seg_off,
                                int64_t n_seg, int64_t min_count, int64_t* out_count) {
  if (!c || !h) return amg_fail(AMG_E_ARG, "null argument");
  if (h->device != c->device) return amg_fail(AMG_E_ARG, "the k-mer table lives on another device");
  if (n_seg < 0 || (n_seg > 0 && !seg_off)) return amg_fail(AMG_E_ARG, "bad segments");
  if (n_seg == 0) return AMG_OK;
  AMGCHK(offsets_check(seg_off, n_seg, "seg_off[0] must be 0", "seg_off not monotone"));
  const int64_t n_bases = seg_off[n_seg];
  if (n_bases == 0) return AMG_OK;
  if (!bases || !out_count) return amg_fail(AMG_E_ARG, "null argument");
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  DevBuf &d_b = c->s0, &d_off = c->s1, &d_out = c->s2;
  AMGCHK(d_b.ensure((size_t)n_bases + 64));
  AMGCHK(d_off.ensure((size_t)(n_seg + 1) * sizeof(long long)));
  AMGCHK(d_out.ensure((size_t)n_bases * sizeof(long long)));
  HIPCHK(hipMemcpyAsync(d_b.p, bases, (size_t)n_bases, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_off.p, seg_off, (size_t)(n_seg + 1) * sizeof(long long), hipMemcpyHostToDevice, st));
  stages_reset(c);
  stage_begin(c, "kcount_query");
  const BaseStream src{d_b.as<unsigned char>(), (long long)n_bases, d_off.as<long long>(), (long long)n_seg, nullptr};
  hipLaunchKernelGGL(KM_BY_WORDS(h->k, &k_kc_query<NW>), dim3(nblk(n_bases, BT_TILE)), dim3(256), 0, st, src, (int)h->k,
                     h->keys.as<unsigned long long>(), h->counts.as<unsigned int>(), (unsigned long long)(h->slots - 1),
                     kc_min_count(min_count), d_out.as<long long>());
  stage_end(c);
  HIPCHK(hipMemcpyAsync(out_count, d_out.p, (size_t)n_bases * sizeof(long long), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return AMG_OK;
}

extern "C" int amg_kcount_medians(amg_ctx* c, const amg_kcount* h, const amg_seqs* seqs, const int64_t* set_off,
                                  const int64_t* set_row, int64_t n_sets, int64_t min_count, int64_t* n,
                                  int64_t* mid_lo, int64_t* mid_hi, int64_t max_pairs) {
  if (!c || !h || !seqs) return amg_fail(AMG_E_ARG, "null argument");
  if (h->device != c->device || seqs->device != c->device)
    return amg_fail(AMG_E_ARG, "the k-mer table or the sequences live on another device");
  if (n_sets < 0 || n_sets >= (1ll << 31) || (n_sets > 0 && (!set_off || !n || !mid_lo || !mid_hi)))
    return amg_fail(AMG_E_ARG, "bad sets");
  if (n_sets == 0) return AMG_OK;
  const int64_t P = set_off[n_sets];
  if (P > 0 && !set_row) return amg_fail(AMG_E_ARG, "bad set offsets");
  AMGCHK(offsets_check(set_off, n_sets, "bad set offsets", "set offsets not monotone"));
  for (int64_t p = 0; p < P; ++p)
    if (set_row[p] < 0 || set_row[p] >= seqs->n)
      return amg_fail(AMG_E_ARG, "set row %lld is not a sequence", (long long)set_row[p]);
  if (max_pairs <= 0) max_pairs = 1ll << 30;  // (20 bytes of buffers per pair)
  for (int64_t s = 0; s < n_sets; ++s) n[s] = mid_lo[s] = mid_hi[s] = 0;
  if (P == 0) return AMG_OK;
  HIPCHK(hipSetDevice(c->device));
  hipStream_t st = c->stream;
  std::vector<int> pair_set((size_t)P);
  for (int64_t s = 0; s < n_sets; ++s)
    for (int64_t p = set_off[s]; p < set_off[s + 1]; ++p) pair_set[(size_t)p] = (int)s;
  AMGCHK(h->m_row.ensure((size_t)P * sizeof(long long)));
  AMGCHK(h->m_set.ensure((size_t)P * sizeof(int)));
  AMGCHK(h->m_len.ensure((size_t)(P + 1) * sizeof(long long)));
  AMGCHK(h->m_src.ensure((size_t)(P + 1) * sizeof(long long)));
  AMGCHK(h->m_off.ensure((size_t)(P + 1) * sizeof(long long)));
  AMGCHK(h->m_out.ensure((size_t)(3 * n_sets) * sizeof(long long)));
  HIPCHK(hipMemcpyAsync(h->m_row.p, set_row, (size_t)P * sizeof(long long), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(h->m_set.p, pair_set.data(), (size_t)P * sizeof(int), hipMemcpyHostToDevice, st));
  unsigned long long* counter = c->status.as<unsigned long long>() + ST_MISC;
  HIPCHK(hipMemsetAsync(counter, 0, sizeof(unsigned long long), st));
  stages_reset(c);
  stage_begin(c, "kcount_medians");
  hipLaunchKernelGGL(k_kc_pairs, dim3(nblk(P + 1, 256)), dim3(256), 0, st, h->m_row.as<long long>(), (long long)P,
                     seqs->off.as<long long>(), h->m_len.as<long long>(), h->m_src.as<long long>());
  AMGCHK(prim_exscan_i64(c, h->m_len.as<long long>(), h->m_off.as<long long>(), (size_t)P + 1));
  long long V = 0;  // bases over all listed rows
  HIPCHK(hipMemcpyAsync(&V, h->m_off.as<long long>() + P, sizeof(V), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (V == 0) {
    stage_end(c);
    return AMG_OK;
  }
  // a window per base at most: room for all of them, or for as many as one call may make
  const long long cap = V < max_pairs ? V : max_pairs;
  AMGCHK(h->m_key.ensure((size_t)(cap + 1) * sizeof(unsigned long long)));
  const BaseStream src{seqs->bases.as<unsigned char>(), V, h->m_off.as<long long>(), (long long)P,
                       h->m_src.as<long long>()};
  hipLaunchKernelGGL(KM_BY_WORDS(h->k, &k_kc_emit<NW>), dim3(nblk(V, BT_TILE)), dim3(256), 0, st, src, (int)h->k, h->keys.as<unsigned long long>(),
                     h->counts.as<unsigned int>(), (unsigned long long)(h->slots - 1), kc_min_count(min_count),
                     h->m_set.as<int>(), counter, cap, h->m_key.as<unsigned long long>());
  unsigned long long M = 0;
  HIPCHK(hipMemcpyAsync(&M, counter, sizeof(M), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if ((long long)M > max_pairs) {
    stage_end(c);
    return amg_fail(AMG_E_NOMEM, "%llu (set, count) pairs in one call, %lld at most: split the sets", M,
                    (long long)max_pairs);
  }
  if (M > 0) {
    AMGCHK(h->m_srt.ensure((size_t)(M + 1) * sizeof(unsigned long long)));
    AMGCHK(h->m_v0.ensure((size_t)(M + 1) * sizeof(unsigned int)));
    AMGCHK(h->m_v1.ensure((size_t)(M + 1) * sizeof(unsigned int)));
    // (the sort moves pairs; nobody reads the values)
    HIPCHK(hipMemsetAsync(h->m_v0.p, 0, (size_t)M * sizeof(unsigned int), st));
    AMGCHK(prim_sort_u64_u32(c, h->m_key.as<unsigned long long>(), h->m_srt.as<unsigned long long>(),
                             h->m_v0.as<unsigned int>(), h->m_v1.as<unsigned int>(), (size_t)M,
                             32 + ilog2_ceil((uint64_t)n_sets + 1)));
    hipLaunchKernelGGL(k_kc_pick, dim3(nblk(n_sets, 256)), dim3(256), 0, st, h->m_srt.as<unsigned long long>(),
                       (long long)M, (long long)n_sets, h->m_out.as<long long>());
    HIPCHK(hipMemcpyAsync(n, h->m_out.p, (size_t)n_sets * sizeof(long long), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(mid_lo, h->m_out.as<long long>() + n_sets, (size_t)n_sets * sizeof(long long),
                          hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(mid_hi, h->m_out.as<long long>() + 2 * n_sets, (size_t)n_sets * sizeof(long long),
                          hipMemcpyDeviceToHost, st));
  }
  stage_end(c);
  HIPCHK(hipStreamSynchronize(st));
  return AMG_OK;
}
