// amg_dist_merge.hip — key-owner merge (amg_dist.hip), phases reduce, hold and global.
#include "amg_dist.h"

__device__ __forceinline__ void held_put_tokens(unsigned int* w, const int* tok, int k, bool t16) {
  if (!t16) {
    for (int x = 0; x < k; ++x) w[x] = (unsigned int)tok[x];
    return;
  }
  for (int x = 0; x < k; x += 2)
    w[x >> 1] = ((unsigned int)tok[x] & 0xffffu) | (x + 1 < k ? ((unsigned int)tok[x + 1] << 16) : 0u);
}
__device__ __forceinline__ void held_put_node_head(unsigned int* w, unsigned long long first, unsigned long long total) {
  w[0] = (unsigned int)first;
  w[1] = (unsigned int)(first >> 32);
  w[2] = (unsigned int)total;
}
__device__ __forceinline__ void held_put_edge(unsigned int* w, unsigned long long key, unsigned long long first,
                                              unsigned long long total) {
  w[0] = (unsigned int)key;
  w[1] = (unsigned int)(key >> 32);
  w[2] = (unsigned int)first;
  w[3] = (unsigned int)(first >> 32);
  w[4] = (unsigned int)total;
}

// ------------------------------------------------------------------ phase: owner-side reduce
// Records of one key arrive from every rank that saw it.  They meet in an open-addressing table keyed by the merge key,
// one 32-byte slot = one sector per key.  The record that CREATES a slot (one compare-and-swap on the key) leaves its
// first-seen and count there with plain stores in fields of its own; only the records that FIND their key pay atomics
// (atomicMax on the complement of first-seen, atomicAdd on the count) in the slot's shared fields — nine keys in ten of
// an uncorrected read set come in one record.  Records that all come from ONE rank are distinct keys already: no
// table.  Every record is answered with its key's global first-seen and total, or "dropped" when the total stays
// below the fused filter's threshold.
struct __attribute__((aligned(32))) OSlot {
  unsigned long long key;
  unsigned long long first_inv;  // others: ~min first-seen (0: nobody but the creator)
  unsigned long long cfirst;     // creator's first-seen
  unsigned int cnt;              // others' counts
  unsigned int ccnt;             // creator's count
};
static_assert(sizeof(OSlot) == 32, "owner slot = one sector");

__device__ __forceinline__ bool edge_key_self_loop(unsigned long long key) {
  const unsigned int lo = (unsigned int)((key >> 32) & 0x7fffffffull);
  const unsigned int hi = (unsigned int)(key & 0xffffffffull) - 1u;
  return lo == hi;
}

__global__ void k_own_upsert(const unsigned long long* __restrict__ recs, long long n, OSlot* tab, unsigned long long mask,
                             unsigned int* __restrict__ recslot, unsigned long long* status) {
  long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const unsigned long long key = recs[3 * j], fi = ~recs[3 * j + 1];
  const unsigned int c = (unsigned int)recs[3 * j + 2];
  unsigned long long idx = mix64(key) & mask;
  for (unsigned int probes = 0;; ++probes) {
    OSlot* s = tab + idx;
    unsigned long long cur = ld_u64(&s->key);
    if (cur == 0ull) {
      cur = atomicCAS(&s->key, 0ull, key);
      if (cur == 0ull) {
        s->cfirst = ~fi;
        s->ccnt = c;
        recslot[j] = (unsigned int)idx;
        return;
      }
    }
    if (cur == key) {
      if (ld_u64(&s->first_inv) < fi) atomicMax(&s->first_inv, fi);
      atomicAdd(&s->cnt, c);
      recslot[j] = (unsigned int)idx;
      return;
    }
    if (probes >= (1u << 16)) {
      status[ST_OVERFLOW] = 6;
      recslot[j] = 0u;
      return;
    }
    idx = (idx + 1) & mask;
  }
}

template <bool MULTI>
__global__ void k_own_reply(const unsigned long long* __restrict__ recs, long long n, int is_edge, unsigned int min_cov,
                            const OSlot* __restrict__ tab, const unsigned int* __restrict__ recslot,
                            unsigned long long* __restrict__ replies) {
  long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const unsigned long long key = recs[3 * j];
  unsigned long long gfirst = recs[3 * j + 1];
  unsigned long long total = (unsigned int)recs[3 * j + 2];
  if (MULTI) {
    const OSlot s = tab[recslot[j]];
    const unsigned long long others = ~s.first_inv;  // (nobody but the creator: ~0)
    gfirst = s.cfirst < others ? s.cfirst : others;
    total = (unsigned long long)s.ccnt + s.cnt;
  }
  // (edge classes that are self-loops count twice)
  const unsigned long long cov = (is_edge && edge_key_self_loop(key)) ? total * 2 : total;
  replies[2 * j] = cov >= min_cov ? gfirst : REPLY_DROPPED;
  replies[2 * j + 1] = total;
}

// (made with every other buffer of the round, before the records travel: see st_counts)
int reduce_reserve(amg_ctx* c, DistState* d) {
  if (d->n_sources <= 1) return AMG_OK;
  AMGCHK(d->own_tab.ensure((size_t)pow2_at_least((uint64_t)d->n_recv * 2 + 16) * sizeof(OSlot)));
  return c->s3.ensure((size_t)(d->n_recv + 1) * sizeof(unsigned int));
}

int reduce_records(amg_ctx* c, DistState* d, int is_edge) {
  hipStream_t st = c->stream;
  const long long n = d->n_recv;
  if (n == 0) return AMG_OK;
  const bool multi = d->n_sources > 1;
  const unsigned int min_cov = is_edge ? d->me : d->mn;
  const unsigned long long* recs = static_cast<const unsigned long long*>(d->recv_p);
  unsigned long long* replies = static_cast<unsigned long long*>(d->rep_out_p);
  unsigned long long* status = c->status.as<unsigned long long>();
  if (!multi) {
    hipLaunchKernelGGL(k_own_reply<false>, dim3(nblk(n, 256)), dim3(256), 0, st, recs, n, is_edge, min_cov,
                       (const OSlot*)nullptr, (const unsigned int*)nullptr, replies);
    return AMG_OK;
  }
  const uint64_t slots = pow2_at_least((uint64_t)n * 2 + 16);
  {
    ClearList cl;
    cl.add(d->own_tab.p, (size_t)slots * sizeof(OSlot));
    AMGCHK(clear_many(c, cl));
  }
  hipLaunchKernelGGL(k_own_upsert, dim3(nblk(n, 256)), dim3(256), 0, st, recs, n, d->own_tab.as<OSlot>(),
                     (unsigned long long)(slots - 1), c->s3.as<unsigned int>(), status);
  hipLaunchKernelGGL(k_own_reply<true>, dim3(nblk(n, 256)), dim3(256), 0, st, recs, n, is_edge, min_cov,
                     d->own_tab.as<OSlot>(), c->s3.as<unsigned int>(), replies);
  return AMG_OK;
}

// ------------------------------------------------------------------ phase: hold
// exact-key shards: one flag byte per LOCAL token at the first-seen position of every claim this rank holds
__global__ void k_xh_flags(const unsigned long long* __restrict__ replies, long long n, const unsigned int* __restrict__ order,
                           const unsigned int* __restrict__ first2, unsigned long long base, int shift,
                           unsigned char* __restrict__ flags) {
  long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const unsigned long long g = replies[2 * j];
  if (g == REPLY_DROPPED) return;
  const unsigned int c = order ? order[j] : (unsigned int)j;
  const unsigned int local = ~x_first_inv(first2, c);
  if (base + (unsigned long long)local == g) flags[local >> shift] = 1;
}

__global__ void k_xh_emit_nodes(const unsigned long long* __restrict__ replies, long long n,
                                const unsigned int* __restrict__ order, const unsigned int* __restrict__ first2,
                                unsigned long long base, const unsigned int* __restrict__ bits,
                                const long long* __restrict__ prefix, const Slot16* __restrict__ tab,
                                const unsigned int* __restrict__ slot_by_claim, int k, int xbits, int two,
                                unsigned int* __restrict__ out, int rec_words, int t16) {
  long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const unsigned long long g = replies[2 * j];
  if (g == REPLY_DROPPED) return;
  const unsigned int c = order ? order[j] : (unsigned int)j;
  const unsigned int local = ~x_first_inv(first2, c);
  if (base + (unsigned long long)local != g) return;
  unsigned int* w = out + (size_t)x_rank_of(local >> 1, bits, prefix) * rec_words;
  held_put_node_head(w, g, replies[2 * j + 1]);
  const Slot16 s = tab[slot_by_claim[c]];
  const unsigned int tag = x_tag_of(s, two);
  int tok[AMG_MAX_K];
  for (int x = 0; x < k; ++x) tok[x] = x_unpack(s.w1, tag, xbits, x);
  held_put_tokens(w + 3, tok, k, t16 != 0);
}

__global__ void k_xh_emit_edges(const unsigned long long* __restrict__ replies, long long n,
                                const unsigned int* __restrict__ order, const unsigned int* __restrict__ first2,
                                unsigned long long base, const unsigned int* __restrict__ bits,
                                const long long* __restrict__ prefix, const unsigned long long* __restrict__ sent,
                                unsigned int* __restrict__ out) {
  long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const unsigned long long g = replies[2 * j];
  if (g == REPLY_DROPPED) return;
  const unsigned int c = order ? order[j] : (unsigned int)j;
  const unsigned int local = ~x_first_inv(first2, c);
  if (base + (unsigned long long)local != g) return;
  unsigned int* w = out + 5 * x_rank_of(local >> 3, bits, prefix);
  const unsigned long long key = sent[3 * j];
  held_put_edge(w, key, g, replies[2 * j + 1]);
}

// fingerprint shards: the compaction list is in local first-seen order already — a flag per entry, a scan
__global__ void k_fh_flags(const unsigned long long* __restrict__ replies, long long n, const unsigned int* __restrict__ order,
                           const unsigned long long* __restrict__ firsts, unsigned long long base,
                           unsigned int* __restrict__ flag) {
  long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const unsigned int i = order ? order[j] : (unsigned int)j;
  const unsigned long long g = replies[2 * j];
  flag[i] = (g != REPLY_DROPPED && firsts[i] + base == g) ? 1u : 0u;
}

__global__ void k_fh_emit_nodes(const unsigned long long* __restrict__ replies, long long n,
                                const unsigned int* __restrict__ order, const unsigned long long* __restrict__ firsts,
                                const unsigned int* __restrict__ flag, const long long* __restrict__ pos,
                                const int* __restrict__ tokens, int k, int two_v, unsigned int* __restrict__ out,
                                int rec_words, int t16) {
  long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const unsigned int i = order ? order[j] : (unsigned int)j;
  if (!flag[i]) return;
  unsigned int* w = out + (size_t)pos[i] * rec_words;
  const unsigned long long g = replies[2 * j];
  held_put_node_head(w, g, replies[2 * j + 1]);
  const unsigned long long first = firsts[i];  // local: the node pass ran with token base 0
  const long long t = (long long)(first >> 1);
  const int dir = (first & 1ull) ? -1 : 1;
  const int flip = two_v - 1;
  int tok[AMG_MAX_K];
  for (int x = 0; x < k; ++x) tok[x] = dir > 0 ? tokens[t + x] : flip - tokens[t + k - 1 - x];
  held_put_tokens(w + 3, tok, k, t16 != 0);
}

__global__ void k_fh_emit_edges(const unsigned long long* __restrict__ replies, long long n,
                                const unsigned int* __restrict__ order, const unsigned int* __restrict__ flag,
                                const long long* __restrict__ pos, const unsigned long long* __restrict__ sent,
                                unsigned int* __restrict__ out) {
  long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const unsigned int i = order ? order[j] : (unsigned int)j;
  if (!flag[i]) return;
  unsigned int* w = out + 5 * pos[i];
  const unsigned long long key = sent[3 * j], g = replies[2 * j];
  held_put_edge(w, key, g, replies[2 * j + 1]);
}

__global__ void k_hc_msg(const long long* __restrict__ n_held, int attempt, const unsigned long long* __restrict__ status,
                         long long* __restrict__ msg) {
  long long code = 0;
  if (status[ST_OVERFLOW] || status[ST_DIST_BAD]) code = CODE_ERROR;
  msg[0] = code ? code : *n_held;
  msg[1] = attempt;
}

// holders ranked, held records emitted in local first-seen order, the number held in d->hc_send
int hold_records(amg_ctx* c, DistState* d, int is_edge) {
  hipStream_t st = c->stream;
  const long long n = d->n_send;
  const unsigned long long* rep = static_cast<const unsigned long long*>(d->rep_in_p);
  const unsigned int* order = send_order(d);
  const int shift = is_edge ? 3 : 1;
  const unsigned long long base = (unsigned long long)c->tok_base << shift;
  const int rb = held_bytes(c, is_edge);
  unsigned long long* status = c->status.as<unsigned long long>();
  const long long* n_held = nullptr;
  if (c->dist_x) {
    unsigned char* flags;
    RankBitmap r;
    AMGCHK(rank_bitmap_begin(c, RankFlagsZeroed{}, &flags));
    const unsigned int* first2 = is_edge ? c->x_efirst.as<unsigned int>() : c->x_first.as<unsigned int>();
    if (n > 0)
      hipLaunchKernelGGL(k_xh_flags, dim3(nblk(n, 256)), dim3(256), 0, st, rep, n, order, first2, base, shift, flags);
    AMGCHK(rank_bitmap_finish(c, &r));
    if (n > 0 && !is_edge)
      hipLaunchKernelGGL(k_xh_emit_nodes, dim3(nblk(n, 256)), dim3(256), 0, st, rep, n, order, first2, base,
                         r.bits, r.prefix, c->node_tab.as<Slot16>(),
                         c->x_slot.as<unsigned int>(), c->k, c->x_bits, c->x_two ? 1 : 0,
                         d->held.as<unsigned int>(), rb / 4, held_tok16(c->two_v) ? 1 : 0);
    else if (n > 0)
      hipLaunchKernelGGL(k_xh_emit_edges, dim3(nblk(n, 256)), dim3(256), 0, st, rep, n, order, first2, base,
                         r.bits, r.prefix, d->send.as<unsigned long long>(), d->held.as<unsigned int>());
    n_held = r.total;
  } else {
    AMGCHK(c->s4.ensure((size_t)(n + 2) * sizeof(unsigned int)));
    AMGCHK(c->s5.ensure((size_t)(n + 2) * sizeof(long long)));
    unsigned int* flag = c->s4.as<unsigned int>();
    long long* pos = c->s5.as<long long>();
    HIPCHK(hipMemsetAsync(flag + n, 0, sizeof(unsigned int), st));
    // (nodes: the list holds local first-seen values; edge classes were made after the token base was known)
    const unsigned long long add = is_edge ? 0ull : base;
    if (n > 0)
      hipLaunchKernelGGL(k_fh_flags, dim3(nblk(n, 256)), dim3(256), 0, st, rep, n, order,
                         d->loc_first.as<unsigned long long>(), add, flag);
    AMGCHK(prim_exscan_u32_to_i64(c, flag, pos, (size_t)n + 1));
    if (n > 0 && !is_edge)
      hipLaunchKernelGGL(k_fh_emit_nodes, dim3(nblk(n, 256)), dim3(256), 0, st, rep, n, order,
                         d->loc_first.as<unsigned long long>(), flag, pos, c->tokens.as<int>(), c->k, c->two_v,
                         d->held.as<unsigned int>(), rb / 4, held_tok16(c->two_v) ? 1 : 0);
    else if (n > 0)
      hipLaunchKernelGGL(k_fh_emit_edges, dim3(nblk(n, 256)), dim3(256), 0, st, rep, n, order, flag, pos,
                         d->send.as<unsigned long long>(), d->held.as<unsigned int>());
    n_held = pos + n;
  }
  hipLaunchKernelGGL(k_hc_msg, dim3(1), dim3(1), 0, st, n_held, d->attempt, status, d->hc_send.as<long long>());
  return AMG_OK;
}

// ------------------------------------------------------------------ phase: global ids
// off[r] = held records of the ranks before r (off[world] = all of them)
__global__ void k_offs(const long long* __restrict__ hc, int world, long long* __restrict__ off) {
  if (threadIdx.x || blockIdx.x) return;
  long long s = 0;
  for (int r = 0; r < world; ++r) {
    off[r] = s;
    s += hc[(size_t)r * HC_WORDS] > 0 ? hc[(size_t)r * HC_WORDS] : 0;
  }
  off[world] = s;
}

void held_offsets(amg_ctx* c, DistState* d, const long long* held_counts_msg) {
  hipLaunchKernelGGL(k_offs, dim3(1), dim3(1), 0, c->stream, held_counts_msg, d->world, d->offs.as<long long>());
}

// node arrays in global id order: the gathered buffer (world parts of m record slots) unpacked
__global__ void k_global_nodes(const unsigned int* __restrict__ recs, long long m, int world,
                               const long long* __restrict__ off, int rec_words, int k, int t16, int* __restrict__ node_tokens,
                               unsigned int* __restrict__ node_cov, long long* __restrict__ node_first,
                               unsigned char* __restrict__ node_alive) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m * world) return;
  const int r = (int)(i / m);
  const long long j = i - (long long)r * m;
  if (j >= off[r + 1] - off[r]) return;
  const long long id = off[r] + j;
  const unsigned int* w = recs + (size_t)i * rec_words;
  node_first[id] = (long long)((unsigned long long)w[0] | ((unsigned long long)w[1] << 32));
  node_cov[id] = w[2];
  node_alive[id] = 1;
  for (int x = 0; x < k; ++x)
    node_tokens[id * k + x] = t16 ? (int)((w[3 + (x >> 1)] >> ((x & 1) * 16)) & 0xffffu) : (int)w[3 + x];
}

__global__ void k_global_pairs(const unsigned int* __restrict__ recs, long long m, int world,
                               const long long* __restrict__ off, unsigned long long* __restrict__ pkey,
                               unsigned long long* __restrict__ pfirst, unsigned int* __restrict__ pcnt) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m * world) return;
  const int r = (int)(i / m);
  const long long j = i - (long long)r * m;
  if (j >= off[r + 1] - off[r]) return;
  const long long id = off[r] + j;
  const unsigned int* w = recs + 5 * i;
  pkey[id] = (unsigned long long)w[0] | ((unsigned long long)w[1] << 32);
  pfirst[id] = (unsigned long long)w[2] | ((unsigned long long)w[3] << 32);
  pcnt[id] = w[4];
}

// id of the node whose first-seen value is g: the node arrays are in ascending first-seen order
__device__ __forceinline__ long long id_of_first(const long long* __restrict__ node_first, long long n, unsigned long long g) {
  long long lo = 0, hi = n;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if ((unsigned long long)node_first[mid] < g) lo = mid + 1; else hi = mid;
  }
  return (lo < n && (unsigned long long)node_first[lo] == g) ? lo : -1;
}

// local node (record j of what this rank sent) -> global node id through its owner's reply; -2 when the node fell to
// the fused filter (its windows then read None).  The tuple of the local key must be the holder's.
__global__ void k_map_claims(const unsigned long long* __restrict__ replies, long long n, const unsigned int* __restrict__ order,
                             const long long* __restrict__ node_first, long long n_nodes,
                             const int* __restrict__ node_tokens, const Slot16* __restrict__ tab,
                             const unsigned int* __restrict__ slot_by_claim, int k, int xbits, int two,
                             int* __restrict__ final_of_claim, unsigned long long* status) {
  long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const unsigned int c = order ? order[j] : (unsigned int)j;
  const unsigned long long g = replies[2 * j];
  if (g == REPLY_DROPPED) {
    final_of_claim[c] = -2;
    return;
  }
  const long long id = id_of_first(node_first, n_nodes, g);
  if (id < 0) {
    status[ST_DIST_BAD] = 1;
    final_of_claim[c] = -2;
    return;
  }
  const Slot16 s = tab[slot_by_claim[c]];
  const unsigned int tag = x_tag_of(s, two);
  for (int x = 0; x < k; ++x)
    if (x_unpack(s.w1, tag, xbits, x) != node_tokens[id * k + x]) status[ST_COLLISION] = 1;
  final_of_claim[c] = (int)id;
}

// fingerprint shards: the id goes into the local slot (the edge pass verifies every window's tuple against it)
__global__ void k_map_slots(const unsigned long long* __restrict__ replies, long long n, const unsigned int* __restrict__ order,
                            const long long* __restrict__ node_first, long long n_nodes,
                            const unsigned int* __restrict__ slots, Slot* __restrict__ ltab,
                            const int* __restrict__ node_tokens, int k, int packed, unsigned long long* status) {
  long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const unsigned long long g = replies[2 * j];
  Slot* s = ltab + slots[order ? order[j] : (unsigned int)j];
  long long id = -2;
  if (g != REPLY_DROPPED) {
    id = id_of_first(node_first, n_nodes, g);
    if (id < 0) {
      status[ST_DIST_BAD] = 1;
      id = -2;
    }
  }
  if (!packed) {
    s->id = (int)id;
  } else if (id >= 0) {
    slot_pack(s, (int)id, node_tokens + id * k, k);
  } else {
    int none[AMG_MAX_K] = {0};
    slot_pack(s, -2, none, k);
  }
}

int nodes_global(amg_ctx* c, DistState* d) {
  hipStream_t st = c->stream;
  const long long n = d->n_total, m = d->m_pad;
  const int rb = held_bytes(c, 0);
  stage_begin(c, "merge_node_global");
  c->packed_nodes = !c->dist_x && (c->two_v <= 65536 && c->k <= AMG_PACK_MAX_K);
  c->n_nodes = n;
  AMGCHK(bs_alloc_nodes(c, n));
  if (m > 0)
    hipLaunchKernelGGL(k_global_nodes, dim3(nblk(m * d->world, 256)), dim3(256), 0, st,
                       reinterpret_cast<const unsigned int*>(d->gathered_p), m, d->world, d->offs.as<long long>(), rb / 4,
                       c->k, held_tok16(c->two_v) ? 1 : 0, c->node_tokens.as<int>(), c->node_cov.as<unsigned int>(),
                       c->node_first.as<long long>(), c->node_alive.as<unsigned char>());
  const long long nl = d->n_send;
  const unsigned long long* rep = static_cast<const unsigned long long*>(d->rep_in_p);
  unsigned long long* status = c->status.as<unsigned long long>();
  if (nl > 0 && c->dist_x)
    hipLaunchKernelGGL(k_map_claims, dim3(nblk(nl, 256)), dim3(256), 0, st, rep, nl, send_order(d),
                       c->node_first.as<long long>(), n, c->node_tokens.as<int>(), c->node_tab.as<Slot16>(),
                       c->x_slot.as<unsigned int>(), c->k, c->x_bits, c->x_two ? 1 : 0,
                       c->x_final.as<int>(), status);
  else if (nl > 0)
    hipLaunchKernelGGL(k_map_slots, dim3(nblk(nl, 256)), dim3(256), 0, st, rep, nl, send_order(d),
                       c->node_first.as<long long>(), n, d->loc_slot.as<unsigned int>(), c->node_tab.as<Slot>(),
                       c->node_tokens.as<int>(), c->k, c->packed_nodes ? 1 : 0, status);
  stage_end(c);
  return AMG_OK;
}

int edges_global(amg_ctx* c, DistState* d) {
  hipStream_t st = c->stream;
  const long long n = d->n_total, m = d->m_pad;
  stage_begin(c, "merge_edge_global");
  c->n_pairs = n;
  AMGCHK(bs_alloc_pairs(c, n));
  if (m > 0)
    hipLaunchKernelGGL(k_global_pairs, dim3(nblk(m * d->world, 256)), dim3(256), 0, st,
                       reinterpret_cast<const unsigned int*>(d->gathered_p), m, d->world, d->offs.as<long long>(),
                       c->pair_key.as<unsigned long long>(), c->pair_first.as<unsigned long long>(),
                       c->pair_cnt.as<unsigned int>());
  stage_end(c);
  AMGCHK(bs_finish_from_pairs(c));
  if (c->dist_min_node > 1)
    // fused filter: reads that lost a node join _readsToCorrect (remove_node_from_reads :442-461)
    AMGCHK(bx_flag_dead_reads(c));
  c->dist_min_node = c->dist_min_edge = 1;
  ctx_graph_in_place(c, c->n_local_nodes, false);
  return AMG_OK;
}
