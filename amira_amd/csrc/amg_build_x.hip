// amg_build_x.hip — the build in 16-byte slots with claim ids: EXACT tuple keys, or verified 94-bit fingerprints of the
// tuple in the same slots.  This unit holds the two TABLE PASSES (windows -> node claims, adjacencies -> edge-class
// claims: bx_nodes_upsert, bx_edges_upsert) and their claim plan; what is then done per claim — coverage, the fused
// filter, ranking — and the drivers bx_nodes / bx_nodes_filtered / bx_edges are amg_build_x_claims.hip's, a filtered
// build's components and read flags amg_build_x_comp.hip's.
//
// Same result as the 32-byte fingerprint path of amg_build_fp.hip (GeneMerGraph.__init__, reference construct_graph.py:31-102),
// different bookkeeping.  The canonical k-tuple itself is the key whenever it fits 94 bits (k * ceil(log2(2V)) <= 94:
// k = 3 for any vocabulary, k = 5 up to 2^18 genes); a longer tuple is keyed by its 94-bit fingerprint and every window
// is verified against its key's first occurrence (next section).  The 32-byte path is still taken for 2^29 tokens and
// more, for a merged (multi-GPU) build whose tuple does not fit, with AMG_KEY_MODE=fp or AMG_COUNT_INLINE, and for a
// tuple that would fit while the weak-fingerprint hook (AMG_TEST_WEAK_FP) is set: bx_applicable, bx_fits, bx_tuple_fits.
//
//   * a node slot is 16 bytes: w1 = low 63 bits of the packed tuple (+ a set bit 0), w2 =
//     {remaining tuple bits + a set bit, where the creating window was, claim id + 1} (struct
//     XW2).  One 16-byte (plain, L2-served) load per probe decides it; see x_upsert_one for when a cached view
//     may be trusted.
//   * the thread that creates a slot gives it a CLAIM id: creators of a block are counted
//     with a block scan, one atomicAdd per block reserves the ids, the id is published in the
//     slot (threads that found the key before the id was there wait for it after their own
//     block has published — a block never waits before publishing, so there is no cycle).
//   * every per-key quantity lives in DENSE arrays indexed by claim id: first-seen (x_first, two
//     words per claim, read only by the few windows that might precede the creator), slot
//     (x_slot), final node id (x_final).  Claim order follows the token order, so the
//     frequently hit genome nodes own the first few ten thousand claims: the per-window
//     gathers of the edge pass (claim -> node id) and the first-seen updates hit a small
//     L2-resident region instead of one 128-byte line per hot slot, the occupied slots need
//     no table scan to be listed, and occurrence counting (k_count_ids) works on claim ids
//     directly, without a slot -> id gather.
//   * node id = rank of first-seen among the claims (32-bit keys: tokens < 2^29), as before.
// Edge classes ((lo id, hi id, sign), construct_edge.py:104-124) use the same scheme with a
// one-word key.
#include "amg_tile.h"
#include "amg_x.h"

// ------------------------------------------------------------------ tuples that do not fit the slot: 94-bit fingerprints
// k * ceil(log2 2V) > 94 (k >= 7 on a 20 000-gene vocabulary): the key of the SAME 16-byte slots, claim ids and dense
// per-claim arrays is a 94-bit fingerprint of the canonical tuple instead of the tuple itself (w1 = 63 bits, tag = 31).
// Nothing else of the build changes; what a slot no longer says is read from the token stream where it is needed:
//   * a node's tokens (k_x_assign_nodes_ranked) are the window at its first-seen position, canonical by its direction bit
//     (so they are for every key scheme: node_tuples_from_reads, amg_build_x_claims.hip);
//   * every window's tuple is compared with the tuple at its claim's first-seen position (k_x_verify_fp: the creator's
//     window — for the genome's nodes a few hundred kilobytes of the stream's head, L2-resident): two gene-mers that
//     share a fingerprint raise ST_COLLISION and the build is repeated with the next seed (AMG_TEST_WEAK_FP cuts the
//     fingerprint to 12 bits so that this happens).
// The round-1 path for such k — 32-byte slots, sorted compaction lists, a packed-tuple gather per window in the edge
// pass — took 3.5 to 6 times as long per build as the exact-key path (bench.py multi_k); it stays for inputs beyond
// 2^29 tokens, for the multi-GPU merge and behind AMG_KEY_MODE=fp.
template <class View>
__device__ __forceinline__ void x_fp94(const View& w, int k, int flip, int dir, unsigned long long seed, int weak,
                                       unsigned long long& w1, unsigned int& tag) {
  unsigned long long h1 = seed, h2 = seed ^ 0xC2B2AE3D27D4EB4Full;
  for (int j = 0; j < k; ++j) {
    const unsigned long long c = (unsigned long long)(unsigned int)canon_tok(w, k, flip, dir, j);
    h1 = (h1 ^ c) * 0x9E3779B97F4A7C15ull;
    h1 ^= h1 >> 29;
    h2 = (h2 + c) * 0xD6E8FEB86659FD93ull;
    h2 ^= h2 >> 31;
  }
  h1 = mix64(h1);
  h2 = mix64(h2 ^ (h1 >> 7));
  if (weak) {  // test hook: 12 bits
    h1 &= 0xfffull;
    h2 = 0ull;
  }
  w1 = (h1 << 1) | 1ull;
  tag = ((unsigned int)h2 << 1) | 1u;
}

// fingerprint keys: the tuple of every window against the tuple at its claim's first-seen position
__global__ __launch_bounds__(256) void k_x_verify_fp(const int* __restrict__ tokens, long long n_tokens, int k, int flip,
                                                      const int* __restrict__ tok_claim,
                                                      const signed char* __restrict__ tok_dir,
                                                      const unsigned int* __restrict__ first2,
                                                      unsigned long long* status) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_tokens) return;
  const int raw = tok_claim[t];
  if (raw == -1) return;
  const unsigned int claim = (unsigned int)raw & ~AMG_FLAG_MASK;
  const unsigned int first = ~x_first_inv(first2, claim);
  const long long f = (long long)(first >> 1);
  if (f == t) return;  // the first occurrence itself
  const int dir = tok_dir[t], fdir = (first & 1u) ? -1 : 1;
  bool same = true;
  for (int j = 0; j < k; ++j) {
    const int a = dir > 0 ? tokens[t + j] : flip - tokens[t + k - 1 - j];
    const int b = fdir > 0 ? tokens[f + j] : flip - tokens[f + k - 1 - j];
    same = same && a == b;
  }
  if (!same) status[ST_COLLISION] = 1;  // benign race: every writer stores 1
}

// ------------------------------------------------------------------ nodes, four consecutive windows per thread
// Every gene-mer size (K = 0: k at run time): a thread's 4 + k - 1 tokens leave LDS in 128-bit reads, the
// common 16-bit packing shares half-words between the windows, the results leave as one 16-byte and one 4-byte
// store per thread, creators are counted with ballots, and the hit path (the key with its id in the first slot
// probed: nearly every window of a rebuild) is straight-line code.  Streams are non-temporal so that the L2s keep
// the table's hot lines (tools/ubench/pass_bench.hip: a pass of this shape is bound by the line requests of its
// probes, 0.2 ms per 56 M, plus its streams; whatever else it does has to hide behind those).
template <bool TWO, int K, bool B16, bool HEAD = false>  // HEAD: the short launch over the first tiles (a symbol of its own, as k_edges_v's)
__global__ __launch_bounds__(TILE_THREADS, 8) void k_nodes_v(
    const int* __restrict__ tokens, const unsigned int* __restrict__ bnd_bits, long long n_tokens, int k, int two_v,
    int bits, Slot16* tab, unsigned int mask, unsigned int probe_limit, int* __restrict__ tok_claim,
    signed char* __restrict__ tok_dir, unsigned long long* status, unsigned int* first2,
    unsigned int* __restrict__ slot_by_claim, unsigned int cap, XW2 xf, unsigned int tile0,
    unsigned long long* ctrs, unsigned int head_cap, unsigned long long fp_seed, int fp_weak) {
  // bits == 0 (K == 0 only): the key is a 94-bit fingerprint of the canonical tuple (x_fp94)
  __shared__ __attribute__((aligned(16))) int s_tok[TILE + AMG_MAX_K + 4];
  __shared__ unsigned int s_bits[TILE_BIT_WORDS];
  __shared__ unsigned int s_wave[TILE_THREADS / 64 + 1];
  const int tid = threadIdx.x;
  const long long t0 = (long long)(blockIdx.x + tile0) * TILE;
  const XShard cshard = tile_shard<HEAD>(ctrs, blockIdx.x + tile0, head_cap);
  const int flip = two_v - 1;
  stage_tile_v(tokens, bnd_bits, n_tokens, k + 3, t0, s_tok, s_bits, two_v, status);
  const int i0 = 4 * tid;
  unsigned int id1[TILE_ITEMS];
  unsigned int last = 0, ndir = 0, valid = 0;  // per window: last of its read; direction -1; has a node
  unsigned int made = 0;                       // per window: it created its node's key
  {
    unsigned long long w1[TILE_ITEMS];
    unsigned int idx[TILE_ITEMS], tag[TILE_ITEMS];
    ulonglong2 v[TILE_ITEMS];
    // windows whose k tokens lie in one read: no read ends at the positions t + 1 .. t + k - 1 (a read that ends
    // right after the window makes it the last of its read)
    const unsigned int b = tile_bits(s_bits, i0 + 1, k + 3);
    constexpr int NA = K > 0 ? 4 + K - 1 : 1;
    int a[NA];
    if constexpr (K > 0) {
#pragma unroll
      for (int j = 0; j < (NA + 3) / 4; ++j) {
        const int4 x = reinterpret_cast<const int4*>(s_tok + i0)[j];
        if (4 * j + 0 < NA) a[4 * j + 0] = x.x;
        if (4 * j + 1 < NA) a[4 * j + 1] = x.y;
        if (4 * j + 2 < NA) a[4 * j + 2] = x.z;
        if (4 * j + 3 < NA) a[4 * j + 3] = x.w;
      }
    }
#pragma unroll
    for (int w = 0; w < TILE_ITEMS; ++w) {
      w1[w] = 0;
      tag[w] = 0;
      idx[w] = 0;
      const long long t = t0 + i0 + w;
      const bool inside = ((b >> w) & ((1u << (k - 1)) - 1u)) == 0u;
      if (!((t + k <= n_tokens) && inside)) continue;
      int dir;
      if constexpr (K > 0 && B16) {
        dir = f_canon_pack16<K, TWO>(a + w, flip, w1[w], tag[w]);
      } else if constexpr (K > 0) {
        dir = x_canon_pack<K, TWO>(a + w, flip, bits, w1[w], tag[w]);
      } else {
        LdsView win{s_tok + i0 + w};
        dir = canon_dir(win, k, flip);
        if (dir != 0) {
          if (bits == 0)
            x_fp94(win, k, flip, dir, fp_seed, fp_weak, w1[w], tag[w]);
          else
            x_pack(win, k, flip, dir, bits, w1[w], tag[w]);
        }
      }
      if (dir == 0) {
        status[ST_PALINDROME] = 1;  // benign race: every writer stores 1
        continue;
      }
      idx[w] = hashed_slot(w1[w], tag[w], mask);
      v[w] = *reinterpret_cast<const ulonglong2*>(tab + idx[w]);  // in flight while the next window is prepared
      if (dir < 0) ndir |= 1u << w;
      valid |= 1u << w;
      if ((b >> (w + k - 1)) & 1u) last |= 1u << w;
    }
    const TilePos<1, 1> pos{(unsigned int)t0 + i0, ndir};
    unsigned long long* const ctr = ctrs ? ctrs : status + ST_NODE_INSERTS;
    if constexpr (TWO)
      f_table_phase_own(tab, mask, valid, w1, tag, idx, v, pos, xf, first2, slot_by_claim, ctr, cshard, cap, probe_limit,
                        status, 1, id1, s_wave, &made);
    else
      f_table_phase_one(tab, mask, valid, w1, idx, v, pos, first2, slot_by_claim, ctr, cshard, cap, probe_limit, status, 1,
                        id1, s_wave, &made);
  }
  tile_i4 oc;
  unsigned int od = 0;  // the four direction bytes
#pragma unroll
  for (int w = 0; w < TILE_ITEMS; ++w) {
    oc[w] = claim_word(id1[w], last & (1u << w), made & (1u << w));
    od |= (id1[w] ? ((ndir & (1u << w)) ? 0xffu : 1u) : 0u) << (8 * w);
  }
  const long long t = t0 + i0;
  store_items(tok_claim, t, n_tokens, oc);
  if (t + TILE_ITEMS <= n_tokens) {
    __builtin_nontemporal_store(od, reinterpret_cast<unsigned int*>(tok_dir + t));
  } else {
#pragma unroll
    for (int w = 0; w < TILE_ITEMS; ++w)
      if (t + w < n_tokens) tok_dir[t + w] = (signed char)(od >> (8 * w));
  }
}

// ------------------------------------------------------------------ nodes, minimiser buckets
// k_nodes_v is bound by the 128-byte line requests of its probes (one hashed slot = one line per window, DESIGN.md
// section 4).  Consecutive windows of a read share k - 1 genes, so a key function that consecutive windows mostly
// AGREE on turns neighbouring probes into requests for the same line: the gene of a window with the smallest rank
// (its minimiser; ranks follow sha256 order, i.e. they are a random permutation of the genes) is shared by about
// (k + 1) / 2 consecutive windows.  The table gets a BUCKET REGION in front of its hashed slots: one 128-byte line
// (8 slots) per gene rank.  A gene-mer lives in the line of its minimiser, starting at slot p0 = the position of
// that gene in the tuple read along the gene's own strand: the up to k gene-mers of a genome that share a
// minimiser g hold g at k different positions, so every one of them sits in its FIRST slot (p0 is a function of
// the canonical tuple alone: the key decides where it lives, whatever the orientation of the read).  Whatever
// does not find its slot free or its own (AMG_BUCKET_PROBES = 1 slot looked at; error gene-mers, genes in many copies) goes to its
// hashed slot as before.  A thread's four windows lie 256 apart, so the 64 lanes of one probe instruction look at
// 64 consecutive windows: ~64 * 2 / (k + 1) distinct lines instead of 64.
#define AMG_BUCKET_PROBES 1  // measured on cfg 3 (first build / rebuild, ms): 1: 0.92 / 0.35, 2: 0.97 / 0.36, 3: 1.00 / 0.37, 8: 1.16 / 0.43
template <bool TWO, int K, bool B16, bool HEAD = false>
__global__ __launch_bounds__(TILE_THREADS, 8) void k_nodes_m(
    const int* __restrict__ tokens, const unsigned int* __restrict__ bnd_bits, long long n_tokens, int two_v,
    int bits, Slot16* tab, unsigned int mask, unsigned int probe_limit, int* __restrict__ tok_claim,
    signed char* __restrict__ tok_dir, unsigned long long* status, unsigned int* first2,
    unsigned int* __restrict__ slot_by_claim, unsigned int cap, XW2 xf, unsigned int tile0, unsigned int home_n,
    unsigned long long* ctrs, unsigned int head_cap) {
  __shared__ __attribute__((aligned(16))) int s_tok[TILE + AMG_MAX_K + 4];
  __shared__ unsigned int s_bits[TILE_BIT_WORDS];
  __shared__ unsigned int s_wave[TILE_THREADS / 64 + 1];
  const int tid = threadIdx.x;
  const long long t0 = (long long)(blockIdx.x + tile0) * TILE;
  const XShard cshard = tile_shard<HEAD>(ctrs, blockIdx.x + tile0, head_cap);
  const int flip = two_v - 1, V = two_v >> 1;
  stage_tile_v(tokens, bnd_bits, n_tokens, K + 3, t0, s_tok, s_bits, two_v, status);
  unsigned int id1[TILE_ITEMS];
  unsigned int last = 0, ndir = 0, valid = 0;  // per window: last of its read; direction -1; has a node
  unsigned int made = 0;                       // per window: it created its node's key
  {
    unsigned long long w1[TILE_ITEMS];
    unsigned int idx[TILE_ITEMS], tag[TILE_ITEMS];
    ulonglong2 v[TILE_ITEMS];
#pragma unroll
    for (int w = 0; w < TILE_ITEMS; ++w) {
      w1[w] = 0;
      tag[w] = 0;
      idx[w] = 0;
      const int i = w * TILE_THREADS + tid;
      const long long t = t0 + i;
      // no read ends at the positions t + 1 .. t + k - 1; one that ends right after the window makes it the last of its read
      const unsigned int b = tile_bits(s_bits, i + 1, K);
      if (!((t + K <= n_tokens) && (b & ((1u << (K - 1)) - 1u)) == 0u)) continue;
      int a[K];
#pragma unroll
      for (int j = 0; j < K; ++j) a[j] = s_tok[i + j];
      int dir;
      if constexpr (B16)
        dir = f_canon_pack16<K, TWO>(a, flip, w1[w], tag[w]);
      else
        dir = x_canon_pack<K, TWO>(a, flip, bits, w1[w], tag[w]);
      if (dir == 0) {
        status[ST_PALINDROME] = 1;  // benign race: every writer stores 1
        continue;
      }
      // minimiser of the CANONICAL tuple (first occurrence of the smallest gene rank) and where it sits along its own strand
      int best = 0x7fffffff, bj = 0;
      bool plus = true;
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const int c = dir > 0 ? a[j] : flip - a[K - 1 - j];
        const bool p = c >= V;
        const int r = p ? c - V : V - 1 - c;
        if (r < best) {
          best = r;
          bj = j;
          plus = p;
        }
      }
      idx[w] = (unsigned int)best * 8u + (unsigned int)((plus ? bj : K - 1 - bj) & 7);
      v[w] = *reinterpret_cast<const ulonglong2*>(tab + idx[w]);  // in flight while the next window is prepared
      if (dir < 0) ndir |= 1u << w;
      valid |= 1u << w;
      if ((b >> (K - 1)) & 1u) last |= 1u << w;
    }
    const TilePos<1, TILE_THREADS> pos{(unsigned int)t0 + tid, ndir};
    unsigned long long* const ctr = ctrs ? ctrs : status + ST_NODE_INSERTS;
    if constexpr (TWO)
      f_table_phase_own<1, TILE_THREADS, AMG_BUCKET_PROBES>(tab, mask, valid, w1, tag, idx, v, pos, xf, first2, slot_by_claim,
                                                            ctr, cshard, cap, probe_limit, status, 1, id1, s_wave, &made,
                                                            valid, home_n);
    else
      f_table_phase_one<1, TILE_THREADS, AMG_BUCKET_PROBES>(tab, mask, valid, w1, idx, v, pos, first2, slot_by_claim, ctr,
                                                            cshard, cap, probe_limit, status, 1, id1, s_wave, &made, valid,
                                                            home_n);
  }
#pragma unroll
  for (int w = 0; w < TILE_ITEMS; ++w) {
    const long long t = t0 + w * TILE_THREADS + tid;
    if (t >= n_tokens) continue;
    __builtin_nontemporal_store(claim_word(id1[w], last & (1u << w), made & (1u << w)), tok_claim + t);
    __builtin_nontemporal_store(id1[w] ? ((ndir & (1u << w)) ? (signed char)-1 : (signed char)1) : (signed char)0, tok_dir + t);
  }
}

// ------------------------------------------------------------------ edges, four adjacencies per thread
// HOME = 0: a thread's four adjacencies are consecutive (one LDS read of its neighbours' words, one 16-byte store of its
// results), every class lives where its key hashes to.
// HOME > 0 (`home_n` slots in front of the hashed ones): node ids are first-seen ranks, so nine adjacencies in ten join
// ids n and n + 1 — their class lives in slot n, addressed directly (a second class of the same two nodes, or any other
// pair, goes to the hashed slots behind), and a thread's adjacencies lie 256 windows apart so that the 64 lanes of a
// probe instruction look at 64 consecutive windows: consecutive ids, eight slots to a 128-byte line instead of one
// line per lane (the passes are bound by the line requests of their probes).
// LONE (with HOME): `final_of_claim` carries AMG_SINGLE_BIT on the nodes of coverage 1 (k_x_cov_from_claims).  Every
// adjacency of such a node lies next to its one window, so a class with a single end occurs once — or twice when
// windows t - 1 and t + 1 of the single window t are the same node in the same direction (a period-2 stretch), which
// the two neighbouring words show.  A class known to occur once needs no table: f_table_phase_one's lone items.
template <bool HEAD, bool HOME, bool LONE = false>  // HEAD: the short launch over the first tiles (its own symbol: per-kernel statistics keep the main launch apart)
__global__ __launch_bounds__(TILE_THREADS, 8) void k_edges_v(
    long long n_tokens, const int* __restrict__ tok_claim, const signed char* __restrict__ tok_dir,
    const int* __restrict__ final_of_claim, int* __restrict__ tok_node, Slot16* etab, unsigned int emask,
    unsigned int probe_limit, unsigned long long* status, int* __restrict__ tok_pair, unsigned int* first2,
    unsigned int* __restrict__ slot_by_claim, unsigned int cap, XW2 xf, unsigned int tile0, unsigned int home_n,
    unsigned int lone_base, unsigned long long* ctrs, unsigned int head_cap) {
  static_assert(!LONE || HOME, "lone classes come with the home-slot layout");
  // word per window: node id | single << 29 (LONE) | (direction -1) << 30 | last-of-read << 31, -1: no node
  constexpr unsigned int DIRBIT = 0x40000000u;
  constexpr unsigned int IDMASK = LONE ? AMG_SINGLE_BIT - 1u : DIRBIT - 1u;
  __shared__ __attribute__((aligned(16))) int s_w[TILE + 4];
  __shared__ unsigned int s_wave[TILE_THREADS / 64 + 2];
  const int tid = threadIdx.x;
  const long long t0 = (long long)(blockIdx.x + tile0) * TILE;
  const XShard cshard = tile_shard<HEAD>(ctrs, blockIdx.x + tile0, head_cap);
  const int i0 = 4 * tid;
  const long long t = t0 + i0;
  // node id of a window: -1 no node, -2 a node the merge's fused filter dropped (amg_dist.hip)
  auto node_of = [&](int raw) { return raw == -1 ? -1 : final_of_claim[(unsigned int)raw & ~AMG_FLAG_MASK]; };
  auto word = [&](int raw, int id, unsigned int d) {  // d: the direction byte
    if (id < 0) return -1;
    return (int)((unsigned int)id | ((unsigned int)raw & AMG_LAST_FLAG) | ((d & 0x80u) ? DIRBIT : 0u));
  };
  auto word_at = [&](long long tw) {  // a window outside the tile
    if (tw < 0 || tw >= n_tokens) return -1;
    const int raw = tok_claim[tw];
    return word(raw, node_of(raw), (unsigned int)(unsigned char)tok_dir[tw]);
  };
  int cw[TILE_ITEMS + 1];
  {
    tile_i4 x = {-1, -1, -1, -1};
    unsigned int d = 0;
    if (t + TILE_ITEMS <= n_tokens) {
      x = __builtin_nontemporal_load(reinterpret_cast<const tile_i4*>(tok_claim + t));
      d = __builtin_nontemporal_load(reinterpret_cast<const unsigned int*>(tok_dir + t));
    } else {
#pragma unroll
      for (int w = 0; w < TILE_ITEMS; ++w)
        if (t + w < n_tokens) {
          x[w] = tok_claim[t + w];
          d |= (unsigned int)(unsigned char)tok_dir[t + w] << (8 * w);
        }
    }
    // node id per window (construct_read.py get_geneMers order), as every later stage wants it
    tile_i4 ids;
#pragma unroll
    for (int w = 0; w < TILE_ITEMS; ++w) {
      const int id = node_of(x[w]);
      cw[w] = word(x[w], id, d >> (8 * w));
      ids[w] = (LONE && id >= 0) ? (int)((unsigned int)id & ~AMG_SINGLE_BIT) : id;
    }
    store_items(tok_node, t, n_tokens, ids);
  }
  reinterpret_cast<int4*>(s_w)[tid] = make_int4(cw[0], cw[1], cw[2], cw[3]);
  if (tid == 0) s_w[TILE] = word_at(t0 + TILE);  // the next tile's first window: right-hand neighbour of this tile's last
  if constexpr (LONE) {                          // and the two windows the period-2 check of the tile's ends looks at
    if (tid == 64) s_w[TILE + 1] = word_at(t0 + TILE + 1);
    if (tid == 128) s_w[TILE + 2] = word_at(t0 - 1);
  }
  __syncthreads();
  if constexpr (!HOME) cw[TILE_ITEMS] = s_w[i0 + TILE_ITEMS];

  // adjacency (A, dA) -> (B, dB) of windows t and t + 1 of one read (create_edges :246-262); class key =
  // (smaller id, larger id, dA * dB), first-seen = (token << 3) | orientation
  unsigned long long key[TILE_ITEMS];
  unsigned int idx[TILE_ITEMS], id1[TILE_ITEMS];
  ulonglong2 v[TILE_ITEMS];
  unsigned int valid = 0, orient3 = 0, homed = 0, lone = 0;
#pragma unroll
  for (int w = 0; w < TILE_ITEMS; ++w) {
    key[w] = 0;
    idx[w] = 0;
    const int A = HOME ? s_w[w * TILE_THREADS + tid] : cw[w], B = HOME ? s_w[w * TILE_THREADS + tid + 1] : cw[w + 1];
    if (A == -1 || ((unsigned int)A & AMG_LAST_FLAG) || B == -1) continue;
    const unsigned int a = (unsigned int)A & IDMASK, b = (unsigned int)B & IDMASK;
    const bool negA = ((unsigned int)A & DIRBIT) != 0u, negB = ((unsigned int)B & DIRBIT) != 0u;
    const unsigned int lo = a < b ? a : b, hi = a < b ? b : a;
    const unsigned long long sign = negA != negB ? 1ull : 0ull;
    key[w] = (sign << 63) | ((unsigned long long)lo << 32) | (unsigned long long)(hi + 1u);
    const unsigned int orient = (a == lo ? 1u : 0u) | (negA ? 0u : 2u) | (negB ? 0u : 4u);
    orient3 |= orient << (3 * w);
    valid |= 1u << w;
    if constexpr (LONE) {
      if (((unsigned int)A | (unsigned int)B) & AMG_SINGLE_BIT) {
        const int i = w * TILE_THREADS + tid;
        const int Wm = i == 0 ? s_w[TILE + 2] : s_w[i - 1], Wn = s_w[i + 2];
        // the other adjacency of a single node is the same class: same neighbour node, same direction
        const bool dup_prev = Wm != -1 && !((unsigned int)Wm & AMG_LAST_FLAG) &&
                              (((unsigned int)Wm ^ (unsigned int)B) & (IDMASK | DIRBIT)) == 0u;
        const bool dup_next = !((unsigned int)B & AMG_LAST_FLAG) && Wn != -1 &&
                              (((unsigned int)A ^ (unsigned int)Wn) & (IDMASK | DIRBIT)) == 0u;
        if ((((unsigned int)A & AMG_SINGLE_BIT) && !dup_prev) || (((unsigned int)B & AMG_SINGLE_BIT) && !dup_next)) {
          lone |= 1u << w;
          continue;
        }
      }
    }
    if (HOME && hi == lo + 1u && lo < home_n) {
      idx[w] = lo;
      homed |= 1u << w;
    } else {
      idx[w] = (HOME ? home_n : 0u) + ((unsigned int)mix64(key[w]) & emask);
    }
    v[w] = *reinterpret_cast<const ulonglong2*>(etab + idx[w]);
  }
  unsigned int made = 0;
  unsigned long long* const ctr = ctrs ? ctrs : status + ST_PAIR_INSERTS;
  if constexpr (HOME) {
    // (the lone classes of a first tile take their ids from the tile's own shard: f_table_phase_one)
    f_table_phase_one<3, TILE_THREADS, 1, LONE>(etab, emask, valid, key, idx, v, {(unsigned int)t0 + tid, orient3}, first2,
                                                slot_by_claim, ctr, cshard, cap, probe_limit, status, 2, id1, s_wave, &made,
                                                homed, home_n, lone, lone_base,
                                                tile_shard<false>(ctrs, blockIdx.x + tile0, 0u));
#pragma unroll
    for (int w = 0; w < TILE_ITEMS; ++w) {
      const long long tw = t0 + w * TILE_THREADS + tid;
      if (tw < n_tokens) __builtin_nontemporal_store(claim_word(id1[w], false, made & (1u << w)), tok_pair + tw);
    }
  } else {
    f_table_phase_one<3, 1>(etab, emask, valid, key, idx, v, {(unsigned int)t0 + i0, orient3}, first2, slot_by_claim, ctr,
                            cshard, cap, probe_limit, status, 2, id1, s_wave, &made);
    tile_i4 op;
#pragma unroll
    for (int w = 0; w < TILE_ITEMS; ++w) op[w] = claim_word(id1[w], false, made & (1u << w));
    store_items(tok_pair, t, n_tokens, op);
  }
}

#define X_CTRS (F_SHARDS + 1)  // counters of a plain pass: F_SHARDS shards + the first tiles'

// ------------------------------------------------------------------ host side
// tiles of the head launch of a table pass (0: none: small inputs): a few coverages of a genome of at most
// two_v / 2 genes, never more than 1/16 of the tiles.  Every build of a large input gets one, rebuilds with few keys
// included: the keys that almost every later window hits then hold the lowest claims in stream order, which is what
// the counting sweeps and the rank bitmaps like (measured on the cleaning sweep: 8.8 -> 8.5 ms against head launches
// for first builds only; 48 / 64 / 96 / 128 / 156 / 256 / 512 tiles: 9.27 / 9.02 / 8.69 / 8.62 / 8.46 / 8.70 / 8.84 ms).
static long long head_tiles(const amg_ctx* c, long long n_tiles) {
  if (c->sw.head_tiles_set) return c->sw.head_tiles < n_tiles ? c->sw.head_tiles : n_tiles;  // A/B switch
  if (n_tiles < 4096) return 0;
  long long h = 4ll * c->two_v / TILE;
  if (h < 64) h = 64;
  if (h > n_tiles / 16) h = n_tiles / 16;
  return h;
}
// claims from shard counters (XShard) for the inputs that get a head launch (4 M tokens and more: below that one
// counter serves a pass's workgroups in the time the pass takes anyway); AMG_CLAIM_SHARDS = 0 / 1: never / always
// (A/B + test switch)
static bool shard_claims(const amg_ctx* c, long long n_tiles) {
  if (c->sw.claim_shards >= 0) return c->sw.claim_shards != 0 && n_tiles > 0;
  return n_tiles >= 4096;
}
// a shard's share of `bound` claims: an even split, a quarter of slack, what one workgroup creates in one go; whole chunks
static unsigned int shard_share(long long bound) {
  const long long even = (bound + F_SHARDS - 1) / F_SHARDS;
  const long long share = even + even / 4 + TILE + 1;
  return (unsigned int)((share + X_CHUNK - 1) / X_CHUNK * X_CHUNK);
}
// tiles at the start of the stream that take their claims densely from ONE counter: the head launch's and three times
// as many after it.  A genome key the head launch has not seen (a dozen of 20 k on cfg 3) is created by one of the
// next tiles; from a shard counter its claim would lie far above the ids the counting sweeps keep in LDS, and its
// thousands of occurrences would each be a global atomic on one word (measured: 8 k such windows, +55 us per count).
static long long dense_tiles(long long head, long long n_tiles) {
  const long long d = 4 * head;
  return d < n_tiles ? d : n_tiles;
}

// The claim plan of one table pass (nodes or edge classes): where its claim ids come from and how many there can be.
struct PassPlan {
  long long n_tiles;
  bool rank_next;  // the caller ranks these claims next, with no other use of scratch in between: the ranking's flag bytes are zeroed
                   // behind the read-back (rank_flags_zero_behind) and the proof goes to the ranking (RankFlagsZeroed)
  bool sharded;    // claims from the shard counters (then the ids in use have holes: space())
  unsigned int cap;          // claims per counter
  long long head;            // tiles of the head launch (0: none)
  long long head_cap;        // ids of the first tiles
  size_t max_claims;         // capacity the per-claim arrays need
  unsigned long long* ctrs;  // the pass's X_CTRS counters; nullptr: one counter in the status words

  void clear_with(ClearList& cl) const { if (ctrs) cl.add(ctrs, X_CTRS * F_CTR_STRIDE * sizeof(unsigned long long)); }
  // claim ids in use lie below this when `n` were handed out, the fullest shard's `most` (head_cap ids in front)
  long long space(long long n, unsigned long long most) const {
    if (!ctrs) return n;
    const long long s = head_cap + (long long)((most + X_CHUNK - 1) / X_CHUNK) * (long long)(X_CHUNK * F_SHARDS);
    return s < (long long)max_claims ? s : (long long)max_claims;
  }
};
// who: the table next to PassCaller (amg_internal.h); half: which half of f_ctrs (0 nodes, 1 edge classes)
static int plan_pass(amg_ctx* c, long long n_tiles, long long claim_bound, PassCaller who, int half, PassPlan* p) {
  const bool filtered_edges = who == PassCaller::FilteredBuild && half == 1;
  p->n_tiles = n_tiles;
  p->rank_next = who != PassCaller::MergedLocal && !filtered_edges;
  p->sharded = !filtered_edges && shard_claims(c, n_tiles);
  p->head = n_tiles > 0 ? head_tiles(c, n_tiles) : 0;
  p->cap = p->sharded ? shard_share(claim_bound) : (unsigned int)claim_bound;
  p->head_cap = p->sharded ? dense_tiles(p->head, n_tiles) * TILE : 0;
  p->max_claims = p->sharded ? (size_t)p->head_cap + (size_t)p->cap * F_SHARDS + 1 : (size_t)claim_bound;
  if (p->sharded) AMGCHK(c->f_ctrs.ensure(2 * X_CTRS * F_CTR_STRIDE * sizeof(unsigned long long)));
  p->ctrs = p->sharded ? c->f_ctrs.as<unsigned long long>() + (size_t)half * X_CTRS * F_CTR_STRIDE : nullptr;
  return AMG_OK;
}

// The launches of a table pass: the head launch over the first p.head tiles as stage NAME "_head" (a stage of its own),
// then the main launch over the rest as stage NAME.  launch(head, first tile, tiles) does the hipLaunchKernelGGL.  The
// stage is the kernels alone: its time is what bench.py prices against the roofline.  (Names are kept as pointers.)
#define LAUNCH_HEAD_AND_MAIN(c, p, NAME, ...) launch_head_and_main(c, p, NAME, NAME "_head", __VA_ARGS__)
template <class Launch>
static void launch_head_and_main(amg_ctx* c, const PassPlan& p, const char* name, const char* name_head, Launch launch) {
  stage_begin(c, p.head > 0 ? name_head : name);
  for (int part = 0; part < 2; ++part) {
    const long long lo = part == 0 ? 0 : p.head, cnt = part == 0 ? p.head : p.n_tiles - p.head;
    if (cnt <= 0) continue;  // (no tiles: no launch)
    if (part == 1 && p.head > 0) {
      stage_end(c);
      stage_begin(c, name);
    }
    launch(part == 0, (unsigned int)lo, (unsigned int)cnt);
  }
  stage_end(c);
}

// the status words after a table pass: with shard counters (p.ctrs) their sum replaces host[count_word], the fullest
// shard's count goes to *most.  p.rank_next: the flag bytes of the ranking that follows are zeroed behind the read-back
// kernel, while the host waits, and *zeroed says so
static int read_pass_status(amg_ctx* c, const PassPlan& p, int count_word,
                            unsigned long long* host /*[ST_WORDS + X_CTRS]*/, unsigned long long* most,
                            RankFlagsZeroed* zeroed) {
  FetchList l;
  l.add_words(c->status.p, ST_WORDS);
  if (p.ctrs)
    for (int i = 0; i < X_CTRS; ++i) l.add(p.ctrs + (size_t)i * F_CTR_STRIDE);
  unsigned long long* v = host;
  ClearList fill;
  RankFlagsZeroed z;
  if (p.rank_next) AMGCHK(rank_flags_zero_behind(c, &fill, &z));
  AMGCHK(fetch(c, l, v, p.rank_next ? &fill : nullptr));
  if (zeroed) *zeroed = z;
  *most = 0;
  if (p.ctrs) {
    unsigned long long sum = 0;
    for (int i = 0; i < X_CTRS; ++i) {
      sum += v[ST_WORDS + i];
      if (i < (int)F_SHARDS && v[ST_WORDS + i] > *most) *most = v[ST_WORDS + i];
    }
    host[count_word] = sum;
  }
  return AMG_OK;
}

// bits per token of the packed tuple: 16 whenever that fits (constant shifts in the kernels); AMG_X_TIGHT_BITS=1:
// as few as the vocabulary needs (test switch: the kernels' general packing, which large vocabularies take)
static int bx_bits(const amg_ctx* c, int k) {
  const int need = ilog2_ceil((uint64_t)(c->two_v > 2 ? c->two_v : 2));
  if (need <= 16 && (long long)k * 16 <= 94 && !c->sw.tight_bits) return 16;
  return need;
}

// 16-byte slots may be used: 32-bit first-seen ((token << 3) | orientation, per shard in a merged build), no AMG_KEY_MODE=fp
static bool x_slots_allowed(const amg_ctx* c) { return !c->sw.key_fp && c->n_tokens < (1ll << 29); }

// the canonical tuple itself fits the 94 key bits of a slot (never under the weak-fingerprint hook: the 32-byte path runs)
bool bx_tuple_fits(const amg_ctx* c, int k) {
  return x_slots_allowed(c) && c->weak_fp_builds <= 0 && (long long)k * bx_bits(c, k) <= 94;
}

// the 16-byte-slot build applies: the tuple fits, or it does not and its 94-bit fingerprint is the key (x_fp94)
static bool bx_fits(const amg_ctx* c, int k) {
  return bx_tuple_fits(c, k) || (x_slots_allowed(c) && (long long)k * bx_bits(c, k) > 94);
}

bool bx_applicable(const amg_ctx* c, int k) {
  if (c->dist_mode || c->count_inline) return false;
  return bx_fits(c, k);
}

// The compile-time node kernels, ONE table for k_nodes_m and k_nodes_v: (b16, k in {3, 5, 7}, two) -> <TWO, K, B16>
#define NODE_KERNEL(KERN, HEAD, b16, k, two)                                                    \
  ((b16) && (k) == 3   ? KERN<false, 3, true, HEAD>                                             \
   : (b16) && (k) == 5 ? KERN<true, 5, true, HEAD>                                              \
   : (k) == 3          ? ((two) ? KERN<true, 3, false, HEAD> : KERN<false, 3, false, HEAD>)     \
   : (k) == 5          ? ((two) ? KERN<true, 5, false, HEAD> : KERN<false, 5, false, HEAD>)     \
                       : ((two) ? KERN<true, 7, false, HEAD> : KERN<false, 7, false, HEAD>))

// the table pass alone: claims 0 .. n_local_nodes-1 with their first-seen / slot arrays (with shard counters
// x_nspace > n_nodes: ids nobody took in between).  AMG_E_OVERFLOW + *which = OV_NODE_TABLE: table full.
// *zeroed (nullptr: not wanted): what the ranking of these claims may take for granted
int bx_nodes_upsert(amg_ctx* c, int k, Overflow* which, PassCaller who, RankFlagsZeroed* zeroed) {
  *which = OV_NONE;
  hipStream_t st = c->stream;
  const long long T = c->n_tokens;
  c->exact_keys = true;
  c->packed_nodes = false;
  c->x_bits = bx_bits(c, k);
  c->x_fp = (long long)k * c->x_bits > 94;  // the tuple does not fit the slot: its 94-bit fingerprint is the key (x_fp94)
  c->x_two = c->x_fp || (long long)k * c->x_bits > 63;
  c->x_kbits = c->x_fp ? 0 : c->x_bits;
  const long long n_tiles = (T + TILE - 1) / TILE;
  const bool compiled_k = !c->sw.generic_k && !c->x_fp && (k == 3 || k == 5 || k == 7);  // (AMG_X_GENERIC_K: A/B switch)

  // ---- plan.  Bucket region of the node table (k_nodes_m): one 8-slot line per gene rank in front of the hashed slots, for the
  // gene-mer sizes that have a compile-time kernel; AMG_NODE_BUCKETS=0: hashed slots only (k_nodes_v; A/B switch)
  const bool buckets = c->sw.node_buckets && compiled_k && n_tiles > 0;
  const size_t home_n = buckets ? (size_t)4 * (size_t)c->two_v : 0;  // 8 slots x (two_v / 2) gene ranks
  const size_t tab_slots = (size_t)c->node_slots + home_n;
  PassPlan p;
  AMGCHK(plan_pass(c, n_tiles, ((long long)tab_slots < T ? (long long)tab_slots : T) + 1, who, 0, &p));
  // ---- ensure
  AMGCHK(c->tok_slot.ensure((size_t)(T + 8) * sizeof(int)));
  AMGCHK(c->tok_node.ensure((size_t)(T + 8) * sizeof(int)));
  AMGCHK(c->tok_dir.ensure((size_t)(T + 8)));
  AMGCHK(c->node_tab.ensure(tab_slots * sizeof(Slot16)));
  AMGCHK(c->x_first.ensure(2 * p.max_claims * sizeof(unsigned int)));  // {raised by others, creator's} per claim
  AMGCHK(c->x_slot.ensure(p.max_claims * sizeof(unsigned int)));
  AMGCHK(c->x_final.ensure(p.max_claims * sizeof(int)));
  {  // ---- clear: status words, table, first-seen words and the read-end bitmap are zeroed by ONE launch
    ClearList cl;
    cl.add(c->status.p, ST_WORDS * sizeof(unsigned long long));
    cl.add(c->node_tab.p, tab_slots * sizeof(Slot16));
    cl.add(c->x_first.p, 2 * p.max_claims * sizeof(unsigned int));
    p.clear_with(cl);
    AMGCHK(bs_read_stats(c, k, &cl));
  }
  // ---- launch
  // Claim ids follow the order in which the ~2000 concurrently running tiles create keys: with many creations
  // per tile (a first build: one window in ten) the genome's keys, which almost every later window hits,
  // get claims scattered over the first few hundred thousand, and whoever counts by claim (k_count_ids, one
  // LDS range of 32 k ids per sweep) needs several sweeps.  A short head launch over the first few genome
  // coverages creates them first: their claims are then the lowest (and, with buckets, theirs are the first slots
  // of their lines).
  const bool b16 = c->x_bits == 16 && (k == 3 || k == 5);
  const XW2 xf = xw2_for(p.max_claims, T);
  if (buckets) {
    auto kern = NODE_KERNEL(k_nodes_m, false, b16, k, c->x_two), kern_head = NODE_KERNEL(k_nodes_m, true, b16, k, c->x_two);
    LAUNCH_HEAD_AND_MAIN(c, p, "node_upsert", [&](bool head, unsigned int lo, unsigned int cnt) {
      hipLaunchKernelGGL(head ? kern_head : kern, dim3(cnt), dim3(TILE_THREADS), 0, st, c->tokens.as<int>(),
                         c->bnd_bits.as<unsigned int>(), T, c->two_v, c->x_bits, c->node_tab.as<Slot16>(),
                         (unsigned int)(c->node_slots - 1), kProbeLimit, c->tok_slot.as<int>(),
                         c->tok_dir.as<signed char>(), c->status.as<unsigned long long>(),
                         c->x_first.as<unsigned int>(), c->x_slot.as<unsigned int>(), p.cap, xf, lo,
                         (unsigned int)home_n, p.ctrs, (unsigned int)p.head_cap);
    });
  } else {
    auto kern = c->x_two ? k_nodes_v<true, 0, false> : k_nodes_v<false, 0, false>;  // k at run time
    auto kern_head = c->x_two ? k_nodes_v<true, 0, false, true> : k_nodes_v<false, 0, false, true>;
    if (compiled_k)
      kern = NODE_KERNEL(k_nodes_v, false, b16, k, c->x_two), kern_head = NODE_KERNEL(k_nodes_v, true, b16, k, c->x_two);
    LAUNCH_HEAD_AND_MAIN(c, p, "node_upsert", [&](bool head, unsigned int lo, unsigned int cnt) {
      hipLaunchKernelGGL(head ? kern_head : kern, dim3(cnt), dim3(TILE_THREADS), 0, st, c->tokens.as<int>(),
                         c->bnd_bits.as<unsigned int>(), T, k, c->two_v, c->x_kbits, c->node_tab.as<Slot16>(),
                         (unsigned int)(c->node_slots - 1), kProbeLimit, c->tok_slot.as<int>(),
                         c->tok_dir.as<signed char>(), c->status.as<unsigned long long>(),
                         c->x_first.as<unsigned int>(), c->x_slot.as<unsigned int>(), p.cap, xf, lo, p.ctrs,
                         (unsigned int)p.head_cap, (unsigned long long)c->seed, c->weak_fp_builds > 0 ? 1 : 0);
    });
  }
  if (c->x_fp && n_tiles > 0) {
    // fingerprint keys: every window's tuple against its claim's first occurrence; a mismatch raises ST_COLLISION,
    // which the next read-back of the status words reports (here / bx_nodes_filtered): OV_COLLISION
    stage_begin(c, "node_verify");
    hipLaunchKernelGGL(k_x_verify_fp, dim3(nblk(T, 256)), dim3(256), 0, st, c->tokens.as<int>(), T, k, c->two_v - 1,
                       c->tok_slot.as<int>(), c->tok_dir.as<signed char>(), c->x_first.as<unsigned int>(),
                       c->status.as<unsigned long long>());
    stage_end(c);
  }
  // ---- read back, decode
  unsigned long long hs[ST_WORDS + X_CTRS], most;
  AMGCHK(read_pass_status(c, p, ST_NODE_INSERTS, hs, &most, zeroed));
  if (hs[ST_BADINPUT])
    return amg_fail(AMG_E_ARG, hs[ST_BADINPUT] == 1 ? "read_offsets must start at 0, never decrease and end at the token count"
                                                    : "a token lies outside [0, two_v)");
  if (hs[ST_PALINDROME])
    return amg_fail(AMG_E_PALINDROME, "Gene-mer and reverse complement gene-mer are identical");
  if (hs[ST_MISC]) return amg_fail(AMG_E_HIP, "node pass: a claim id was never published");
  if (hs[ST_COLLISION]) return overflowed(which, OV_COLLISION);  // (fingerprint keys: k_x_verify_fp found two gene-mers under one key)
  if (hs[ST_OVERFLOW]) return overflowed(which, OV_NODE_TABLE);
  c->n_windows = (int64_t)hs[ST_N_WINDOWS];
  c->n_short = (int64_t)hs[ST_N_SHORT];
  c->n_local_nodes = c->n_nodes = (int64_t)hs[ST_NODE_INSERTS];
  c->x_nspace = p.space(c->n_nodes, most);
  return AMG_OK;
}

// the table pass alone: tok_node from x_final, edge-class claims 0 .. n_local_pairs-1
// lone: x_ftag marks the nodes of coverage 1 (bx_node_count); their classes bypass the table
// who, zeroed: as bx_nodes_upsert's.  AMG_E_OVERFLOW + *which = OV_EDGE_TABLE: edge table full
int bx_edges_upsert(amg_ctx* c, Overflow* which, bool lone, PassCaller who, RankFlagsZeroed* zeroed) {
  *which = OV_NONE;
  hipStream_t st = c->stream;
  const long long T = c->n_tokens, D = c->n_nodes;
  const long long n_tiles = (T + TILE - 1) / TILE;
  // ---- plan.  Home slots (k_edges_v<.., true>): one per node id in front of the hashed slots; AMG_EDGE_HOME=0: none (A/B switch)
  const long long home_n = c->sw.edge_home ? ((D + 7) & ~7ll) : 0;
  // hashed slots: with home slots only the classes that do not join ids n and n + 1 (one in ten on gene-call reads)
  // need one — sized for a quarter of the nodes; an input that needs more overflows once and is rebuilt 4x larger
  const int64_t want_slots = (int64_t)slots_for((uint64_t)(home_n ? D / 4 + 1 : D));
  if (c->edge_slots < want_slots) c->edge_slots = want_slots;
  const size_t tab_slots = (size_t)c->edge_slots + (size_t)home_n;
  if (!home_n) lone = false;
  // claims: at most one per table slot, plus (lone) two classes per single node, never more than the windows
  const long long claim_bound = (long long)tab_slots + (lone ? 2 * D : 0);
  PassPlan p;
  AMGCHK(plan_pass(c, n_tiles, (claim_bound < T ? claim_bound : T) + 1, who, 1, &p));
  // ---- ensure
  AMGCHK(c->tok_pair.ensure((size_t)(T + 8) * sizeof(int)));
  AMGCHK(c->edge_tab.ensure((tab_slots + (lone ? p.max_claims : 0)) * sizeof(Slot16)));  // (lone classes: slot = tab_slots + claim)
  AMGCHK(c->x_efirst.ensure(2 * p.max_claims * sizeof(unsigned int)));
  AMGCHK(c->x_eslot.ensure(p.max_claims * sizeof(unsigned int)));
  // ---- clear
  stage_begin(c, "edge_table_clear");
  {
    ClearList cl;
    cl.add(c->edge_tab.p, tab_slots * sizeof(Slot16));
    cl.add(c->x_efirst.p, 2 * p.max_claims * sizeof(unsigned int));
    cl.add(c->status.as<unsigned long long>() + ST_PAIR_INSERTS, 2 * sizeof(unsigned long long));
    p.clear_with(cl);
    AMGCHK(clear_many(c, cl));
  }
  stage_end(c);
  // ---- launch (the head launch: see bx_nodes_upsert — the genome's classes get the lowest claims)
  const XW2 xf = xw2_for(p.max_claims, T);
  LAUNCH_HEAD_AND_MAIN(c, p, "edge_upsert", [&](bool head, unsigned int lo, unsigned int cnt) {
    auto kern = lone     ? (head ? k_edges_v<true, true, true> : k_edges_v<false, true, true>)
                : home_n ? (head ? k_edges_v<true, true> : k_edges_v<false, true>)
                         : (head ? k_edges_v<true, false> : k_edges_v<false, false>);
    hipLaunchKernelGGL(kern, dim3(cnt), dim3(TILE_THREADS), 0, st, T, c->tok_slot.as<int>(),
                       c->tok_dir.as<signed char>(), lone ? c->x_ftag.as<int>() : c->x_final.as<int>(),
                       c->tok_node.as<int>(), c->edge_tab.as<Slot16>(), (unsigned int)(c->edge_slots - 1), kProbeLimit,
                       c->status.as<unsigned long long>(), c->tok_pair.as<int>(),
                       c->x_efirst.as<unsigned int>(), c->x_eslot.as<unsigned int>(), p.cap, xf, lo,
                       (unsigned int)home_n, (unsigned int)tab_slots, p.ctrs, (unsigned int)p.head_cap);
  });
  // ---- read back, decode
  unsigned long long hs[ST_WORDS + X_CTRS], most;
  AMGCHK(read_pass_status(c, p, ST_PAIR_INSERTS, hs, &most, zeroed));
  if (hs[ST_MISC]) return amg_fail(AMG_E_HIP, "edge pass: a claim id was never published");
  if (hs[ST_COLLISION]) return overflowed(which, OV_COLLISION);  // (fingerprint keys: k_x_verify_fp found two gene-mers under one key)
  if (hs[ST_OVERFLOW]) return overflowed(which, OV_EDGE_TABLE);
  c->n_local_pairs = c->n_pairs = (int64_t)hs[ST_PAIR_INSERTS];
  c->x_espace = p.space(c->n_pairs, most);
  return AMG_OK;
}
