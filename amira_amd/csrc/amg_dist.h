// amg_dist.h — what the units of the key-owner merge share (the protocol: amg_dist.hip): record formats and codes,
// the state of a ctx's merges, the host functions of the device phases.
//   amg_dist.hip        RCCL, the driver (one function per state), the derived rebuild, the transports, statistics
//   amg_dist_local.hip  phase local: the shard's tables -> records by destination, the count message
//   amg_dist_merge.hip  phases reduce, hold and global
//   amg_dist_walk.hip   the read walks across ranks: a second, small state machine over the same rank, world and transports
#pragma once
#include <chrono>
#include <string>
#include <vector>

#include <rccl/rccl.h>  // types and prototypes only: the entry points are resolved with dlsym

#include "amg_device.h"
#include "amg_read_walk.h"
#include "amg_slot16.h"

#define REC_BYTES 24    // {u64 merge key, u64 first-seen, u32 count, u32 pad}: what travels to the owners (both kinds)
#define REPLY_WORDS 2   // {u64 global first-seen | REPLY_DROPPED, u64 total count}: what comes back per record
// held records are arrays of 32-bit words (they are the bytes of the all-gathers: 20 + 24 bytes per class + node of a
// rebuilt graph at k = 5, where 8-byte fields and padding made 24 + 40):
//   edge class: {key lo, key hi, first-seen lo, first-seen hi, count}
//   node:       {first-seen lo, first-seen hi, count, tokens: two per word while every token fits 16 bits, else one}
#define HELD_EDGE_BYTES 20
static inline bool held_tok16(int two_v) { return two_v <= 65536; }
static inline size_t held_node_bytes(int k, int two_v) { return (size_t)(4 * (3 + (held_tok16(two_v) ? (k + 1) / 2 : k))); }
static inline int held_bytes(const amg_ctx* c, int is_edge) {
  return is_edge ? HELD_EDGE_BYTES : (int)held_node_bytes(c->k, c->two_v);
}
#define REPLY_DROPPED (~0ull)
#define CNT_WORDS 4     // count message per peer: {records | code < 0, tokens of my shard, attempt, kind}
#define HC_WORDS 2      // held-count message: {records held | code < 0, attempt}
#define CODE_ERROR (-1ll)
#define CODE_COLLISION (-2ll)
#define ST_DIST_BAD 13  // status word: a reply that no gathered record answers (never expected; reported, not retried)
#define MAX_ATTEMPTS 4

__device__ __forceinline__ unsigned int owner_of(unsigned long long key, unsigned int world) {
  return (unsigned int)(mix64(key ^ 0x5851F42D4C957F2Dull) % world);
}

// x_unpack's tag of an exact-key slot (one-word keys: no tag there)
__device__ __forceinline__ unsigned int x_tag_of(const Slot16& s, int two) { return two ? (unsigned int)(s.w2 >> 32) : 0u; }

// ------------------------------------------------------------------ state of a ctx's merges
enum { S_IDLE = 0, S_LOCAL, S_COUNTS, S_REDUCE, S_HOLD, S_HCOUNTS, S_GLOBAL, S_DV_LOCAL, S_DV_ASK, S_DV_FILL, S_N };
// what amg_dist_stats reports, in its order; since the last reset
enum DistStat {
  DS_NONE = -1,
  DS_WAITS = 0,         // host waits on exchanged counts
  DS_EXCHANGES,         // exchanges
  DS_REC_PEER_BYTES,    // most bytes of records to ONE peer
  DS_REPLY_PEER_BYTES,  // the same of replies
  DS_HELD_BYTES,        // bytes contributed to the all-gathers of held records
  DS_REPEATS,           // repeated builds (merge-key collisions)
  DS_REC_BYTES,         // bytes of records sent to all peers
  DS_DERIVED,           // builds made from the previous merged graph's live part
  DS_N
};

// ---- a read walk across ranks (amg_dist_walk.hip): local phase -> header exchange -> verdict -> data exchange -> fold
enum { W_IDLE = 0, W_LOCAL, W_JUDGE, W_FOLD };
struct WalkState {
  int state = W_IDLE, which = 0;
  int32_t n = 0;
  std::vector<int32_t> min_genes;
  std::vector<uint8_t> gene_flags;
  std::vector<unsigned int> flag_words;  // the flag bitmap while the stream takes it
  int64_t hdr[8] = {0};                  // this rank's header (amg_dist_walk_hdr.h)
  int fail_ret = 0;                      // a failure of the local phase, told in the header
  std::string fail_msg;
  int64_t data_words = 0;                // 64-bit words a rank contributes to the data exchange
  DevBuf msg, msg_all;                   // this rank's header (+ the depth sums), the headers of all ranks: made at begin
  DevBuf send, recv;                     // the data exchange: this rank's part / the folded answer, the parts of all ranks
  RwKeep kept;                           // what the local phase left for the fold (amg_read_walk.h): B's keep bytes and
  RwComp comp;                           // kill marks, C's counts (the rank's part of the data exchange)
  bool have_result = false;
  std::vector<int64_t> result;           // amg_dist_walk_result
};

struct DistState {
  int rank = 0, world = 1;
  ncclComm_t comm = nullptr;
  bool always_exchange = false;  // test hook: world 1 sends its records through the transport all the same
  // one merge
  int k = 0, attempt = 0, state = S_IDLE, kind = 0;
  uint32_t mn = 1, me = 1;
  int fail_ret = 0;  // a host-side failure of this rank waiting for the next count exchange
  std::string fail_msg;
  std::vector<int64_t> send_counts, recv_counts, held_counts, tokens, one, words;
  std::vector<int64_t> x_send, x_recv;  // the counts an amg_xfer points at (element counts per peer)
  int64_t n_send = 0, n_recv = 0, n_held = 0, m_pad = 0, n_total = 0;
  int n_sources = 0;
  DevBuf cnt_send, cnt_recv, hc_send, hc_recv, offs;
  DevBuf send, recv, rep_out, rep_in, held, held_pad, gathered;
  // phase local, read up to phase global
  DevBuf loc_bucket;         // the four arrays of a Bucketing
  DevBuf loc_dest_cnt;       // records per destination (and the bins' cursors), on the device
  DevBuf loc_first;          // exact keys: merge key per claim; fingerprints: first-seen of the compaction list
  DevBuf loc_slot;           // fingerprints: table slot of the compaction list (first-seen order)
  DevBuf loc_cnt;            // local occurrences per claim / per first-seen rank
  int64_t nspace = 0;        // ids the current bucketing ran over (local records + claim ids nobody took)
  bool sorted = false;       // the local records leave in sorted order (send_order)
  DevBuf own_tab;            // phase reduce: the owner's table (OSlot)
  // the rebuild that reuses the previous merged graph (amg_derive.hip; S_DV_*)
  bool dv_ok = false;
  long long dv_D2 = 0, dv_P2 = 0, dv_mN = 0, dv_mP = 0;
  std::vector<long long> dv_bases, dv_bounds;
  const void* gathered_p = nullptr;
  const void* recv_p = nullptr;    // the records this rank owns the keys of (one rank: what it packed)
  void* rep_out_p = nullptr;       // the answers to them
  const void* rep_in_p = nullptr;  // the answers to what this rank sent (one rank: the same array)
  // statistics (amg_dist_stats) and per-phase times (amg_dist_merge_local with timing on)
  int64_t st[DS_N] = {0};
  double phase_ms[2 * S_N] = {0};
  bool time_phases = false;
  int phase_now = -1;
  std::chrono::steady_clock::time_point phase_t0;
  WalkState walk;
};

// order in which the local records leave (nullptr: local order); the bucketing ran over d->nspace ids
static inline const unsigned int* send_order(const DistState* d) {
  return d->sorted ? d->loc_bucket.as<unsigned int>() + 3 * (d->nspace + 1) : nullptr;
}

// ------------------------------------------------------------------ what the merge and the walks share (amg_dist.hip)
// entry points that need no graph yet start with this
#define NEED_CTX(c)                                              \
  do {                                                           \
    if (!(c)) return amg_fail(AMG_E_ARG, "null ctx");            \
    HIPCHK(hipSetDevice((c)->device));                           \
  } while (0)
DistState* dist_state(amg_ctx* c);                 // the ctx's state, made on first use
bool dist_on_wire(const DistState* d);             // more than one rank, or the test hook: exchanges are performed
// *x = an all-gather of `count` elements per rank; booked in the statistics (stat: its bytes as well)
void dist_xfer_ag(DistState* d, amg_xfer* x, const void* send, void* recv, int elem_bytes, int64_t count, bool stat);
int dist_rccl_perform(amg_ctx* c, DistState* d, const amg_xfer& x);  // one exchange over RCCL, on the ctx's stream
// emulated ranks: xs[r] is what rank r = ctxs[r] asked for; performed as device copies, waited for
int dist_local_exchange(amg_ctx* const* ctxs, int world, const amg_xfer* xs);

// ------------------------------------------------------------------ the device phases (all on the ctx's stream)
// amg_dist_local.hip
int nodes_local(amg_ctx* c, DistState* d);  // the shard's table pass, occurrence counts, destinations
int edges_local(amg_ctx* c, DistState* d);
void count_message(amg_ctx* c, DistState* d, int is_edge);  // d->cnt_send: counts per peer, or this rank's failure
void pack_records(amg_ctx* c, DistState* d, int is_edge);   // d->send: the records in destination order
// amg_dist_merge.hip
int reduce_reserve(amg_ctx* c, DistState* d);  // the owner's table for d->n_recv records from d->n_sources ranks
int reduce_records(amg_ctx* c, DistState* d, int is_edge);
int hold_records(amg_ctx* c, DistState* d, int is_edge);
void held_offsets(amg_ctx* c, DistState* d, const long long* held_counts_msg);  // d->offs
int nodes_global(amg_ctx* c, DistState* d);
int edges_global(amg_ctx* c, DistState* d);
