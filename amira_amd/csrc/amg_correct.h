// amg_correct.h — what the units of the read correction share: the kernels' argument structs, the size limits two
// units have to agree on, and the host's view of ONE amg_correct_reads call (switches, scratch plan, counts read
// back) with the stage functions that work on it.
//   amg_correct.hip         classify, shape, pack, and amg_correct_reads itself (the pipeline is described there)
//   amg_correct_gapped.hip  re-threading of the reads with None runs      (stage correct_gapped: its driver)
//   amg_gap_memo.hip        the path memo: every question of the None runs answered once
//   amg_gap_lean.hip        sixteen lanes per read: the reads whose every question has one answer
//   amg_gap_fast.hip        a wave per read, staged in LDS
//   amg_gap_general.hip     a thread per read, global pool and scratch: what exceeds the LDS capacities
//   amg_correct_nw.hip      position carry-over of the re-threaded reads  (stage correct_positions)
//   amg_nw_probe.hip        amg_nw_probe: that stage alone on host arrays (test entry)
//   amg_corrected.hip       the corrected set at the boundary (it gathers positions through CorrArgs' pools)
#pragma once
#include "amg_device.h"

enum { RC_SKIP = 0, RC_COPY = 1, RC_DROP = 2, RC_TRIM = 3, RC_GAPPED = 4, RC_KEEP_ORIG = 5 };

struct CorrArgs {
  const int* tokens;
  const long long* read_off;
  const int* tok_node;
  const signed char* tok_dir;
  const unsigned char* read_fix;
  const unsigned long long* win_mask;  // live windows 0..63 per read from the last removal's read walk; null: not current
  // gene positions are NOT moved with the genes when reads are corrected: a read carries an offset
  // (pos_off[r]; nullptr = its token offset) into one of two pools — the caller's arrays as handed to
  // amg_set_positions (indices < n0) or the positions the carry-over kernels produced (p1*, indices
  // from n0 on).  An untouched read keeps its offset, a trimmed one adds its start, a re-threaded one
  // points at its new positions; the corrected set is gathered only when the host asks for it.
  const long long* p0s;
  const long long* p0e;
  const long long* p1s;
  const long long* p1e;
  long long n0;
  const long long* pos_off;
  const long long* read_len;
  long long n_reads;
  int k, flip, have_pos;
  // per read
  unsigned int* gflag;            // 1: the read is re-threaded (RC_GAPPED)
  unsigned long long* max_bound;  // largest `bound` of a re-threaded read: 16 partial maxima, 16 words apart
  unsigned long long* lmask;      // live-window mask of a flagged read with <= 64 windows (0 otherwise)
  unsigned long long* n_runs;     // None runs over all re-threaded reads: 16 partial sums, 16 words apart
  unsigned char* cls;
  unsigned char* cls_final;  // starts as a copy of cls (k_corr_classify writes both); the re-threading may turn a read into RC_KEEP_ORIG
  int* r_start;
  int* r_end;
  unsigned int* bound;
  const long long* tmp_off;
  unsigned int* new_len;
  // staged genes of the re-threaded reads
  int* tmp_tok;
};

// positions of the genes that start at pool index `off`
__device__ __forceinline__ void pos_base(const CorrArgs& a, long long off, const long long*& gs, const long long*& ge) {
  if (off < a.n0) {
    gs = a.p0s + off;
    ge = a.p0e + off;
  } else {
    gs = a.p1s + (off - a.n0);
    ge = a.p1e + (off - a.n0);
  }
}

__device__ __forceinline__ long long bcast_i64(long long v, int lane) {
  const unsigned int lo = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)v, lane);
  const unsigned int hi = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)((unsigned long long)v >> 32), lane);
  return (long long)(((unsigned long long)hi << 32) | lo);
}

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// inclusive prefix sum inside a DPP row of 16 lanes
__device__ __forceinline__ int row_scan_incl(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);  // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);  // row_shr:2
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);  // row_shr:4
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);  // row_shr:8
  return v;
}
// inclusive prefix maximum over the 64 lanes of a wave (id: the identity, what a lane without a left neighbour takes)
__device__ __forceinline__ int wave_prefix_max(int g, const int id) {
  g = max(g, __builtin_amdgcn_update_dpp(id, g, 0x111, 0xf, 0xf, false));  // row_shr:1
  g = max(g, __builtin_amdgcn_update_dpp(id, g, 0x112, 0xf, 0xf, false));  // row_shr:2
  g = max(g, __builtin_amdgcn_update_dpp(id, g, 0x114, 0xf, 0xf, false));  // row_shr:4
  g = max(g, __builtin_amdgcn_update_dpp(id, g, 0x118, 0xf, 0xf, false));  // row_shr:8
  g = max(g, __builtin_amdgcn_update_dpp(id, g, 0x142, 0xa, 0xf, false));  // row_bcast:15
  g = max(g, __builtin_amdgcn_update_dpp(id, g, 0x143, 0xc, 0xf, false));  // row_bcast:31
  return g;
}

// ---- re-threading (amg_correct_gapped.hip and the amg_gap_* units)
// what the wave-per-read kernel needs to start on gapped read gi, in one 32-byte record
// (written by k_scatter_gapped) instead of a chain of dependent per-read loads
struct __attribute__((aligned(16))) GapRec {
  int r, L0, start, end;
  long long t0, dst;
  unsigned long long mask;  // live windows of a read with <= 64 windows (k_corr_classify), 0 otherwise
  long long pad;
};

// The None runs of a read with <= 64 windows, read off its live-window mask lv (start, end: its first and last live
// window).  A run ends at window i when i is not live and i + 1 is, start <= i < end (identify_path_terminals
// :1375-1386; k_corr_classify counts the same bits); the runs are numbered by ascending end bit.
__device__ __forceinline__ unsigned long long gap_run_ends(unsigned long long lv, int start, int end) {
  const unsigned long long inside =
      (end >= 63 ? ~0ull : ((1ull << (end + 1)) - 1ull)) & ~((1ull << (start & 63)) - 1ull);
  return ~lv & inside & (lv >> 1);
}
// the run that ends at window i lies between the live windows ps (the last one before i) and pe
__device__ __forceinline__ void gap_run_terminals(unsigned long long lv, int i, int& ps, int& pe) {
  ps = 63 - __clzll((long long)(lv & ((1ull << i) - 1ull)));
  pe = i + 1;
}

struct GapArgs {
  CorrArgs a;
  GView g;
  const GapRec* rec;
  const int* gapped_reads;
  long long n_gapped;
  int* pool;               // path pool (ints)
  unsigned long long pool_cap;
  unsigned long long* pool_used;  // bump pointer
  unsigned long long* status;
  int* cand;               // candidate scratch, [grid threads * cand_stride]
  unsigned int cand_stride;
  unsigned char* final_cls;
  unsigned char* need_slow;  // per gapped read: non-zero = the wave-per-read fast kernel gave up (a GS_* code: why)
  // path memo (k_gap_queries / k_gap_dfs): the same (start node, direction, end node) question is asked by every read
  // that lost the same stretch of the genome — about nine times each at 3 000x depth — and answered once
  const int* gq;             // per gapped read GF_MAXGAP query slots in run order; [0] < 0: no memo for this read
  const int4* qres;          // per query slot {pool offset, ints, paths, -}; ints < 0: the answer did not fit
  const int* qpool;          // [run = 0, len, nodes, dirs] records in DFS order
};

// capacities of the LDS-staged gapped kernels; a read beyond one of them is left to the general kernel
#define GF_MAXW 128     // windows per read
#define GF_MAXGAP 16    // None runs per read
#define GF_POOL 384     // ints of path records per read
#define GF_CAND 136     // nodes of a candidate (LDS of the block stays under 20 KB: 8 blocks per CU)
#define GF_MAXCOMBO 256
#define GM_INLINE 64   // path memo: ints of an answer that lives in its question's own stretch of the pool
#define LEAN_CHUNK 32  // gapped reads per workgroup when k_corr_gapped_fast works through k_corr_gapped_lean's left-overs
#define CLS_READS 64   // reads per wave of k_corr_classify
#define PACK_READS 64  // reads per wave of k_corr_pack
// why a read was handed down a tier: what need_slow[gi] (wave-per-read kernel -> k_corr_gapped) and the lean kernel's
// flag (k_corr_gapped_lean -> k_corr_gapped_fast) hold.  The consumers test for non-zero; the route report
// (AMG_CORR_ROUTES, amg_correct_routes.hip) tallies the codes.
enum {
  GS_NOT_TRIED = 1,   // the pre-fill 0x01010101 of AMG_NO_FAST_GAPPED: the wave-per-read kernel did not run
  GS_WINDOWS = 2,     // more than GF_MAXW windows
  GS_RUNS = 3,        // more than GF_MAXGAP None runs
  GS_MEMO_UNFIT = 4,  // a memo answer that did not fit (its pool, or GF_POOL ints inside k_gap_dfs)
  GS_RECORDS = 5,     // the read's path records exceed GF_POOL ints
  GS_COMBOS = 6,      // more than GF_MAXCOMBO candidates
  GS_CAND = 7,        // a candidate longer than GF_CAND nodes
  GS_CODES = 8
};
enum {
  GL_NO_SLOTS = 1,  // no memo slots for the read (more than 64 windows or GF_MAXGAP runs)
  GL_ANSWERS = 2,   // a question without exactly one answer (none, several, or one that did not fit)
  GL_LONG = 3,      // a single answer longer than GM_INLINE ints
  GL_OTHER = 4,     // a path of one node (or a run without a slot)
  GL_CODES = 5
};

// ---- position carry-over (amg_correct_nw.hip)
// what k_corr_nw_fast takes: N corrected genes against M original ones (k_nw_sizes decides with the same rule)
#define NWF_MAX_M 64
#define NWF_MAX_N 128
__device__ __forceinline__ bool nw_fast_ok(long long N, long long M) {
  return N <= NWF_MAX_N && M <= NWF_MAX_M && N > 0 && M > 0;
}
// what k_corr_nw keeps in LDS, and the global scratch of a pair beyond that (k_nw_sizes sizes it, k_corr_nw carves
// it, amg_nw_probe refuses too much of it): the pointer matrix, a byte per cell; behind it the op list; at the next
// 16 bytes three rolling anti-diagonals of N + 1 ints
#define NW_LDS_N 1024       // rows and columns kept in LDS (rolling anti-diagonals, op list)
#define NW_LDS_CELLS 16384  // pointer-matrix cells kept in LDS
__host__ __device__ __forceinline__ bool nw_in_lds(long long N, long long M) {
  return N <= NW_LDS_N && M <= NW_LDS_N && N * M <= NW_LDS_CELLS;
}
__host__ __device__ __forceinline__ long long nw_scratch_ops_at(long long N, long long M) { return N * M; }
__host__ __device__ __forceinline__ long long nw_scratch_diag_at(long long N, long long M) {
  return (N * M + N + M + 15) & ~15ll;
}
__host__ __device__ __forceinline__ long long nw_scratch_bytes(long long N, long long M) {
  return nw_scratch_diag_at(N, M) + ((3 * (N + 1) * 4 + 15) & ~15ll);
}

struct __attribute__((aligned(16))) NwRec {
  int r, M, N, pad;
  long long t0, dst;  // first token of the read, first staged gene of its corrected version
  long long pdst;     // where the read's new positions go in the pool of produced positions
  long long poff;     // pool index of the read's ORIGINAL positions
};

struct NwArgs {
  CorrArgs a;        // (a.cls_final: the reads' final classes)
  const NwRec* rec;  // per gapped read, written by k_nw_sizes
  long long* o_gs;   // gene positions of the corrected set: the carry-over writes its reads' entries
  long long* o_ge;   // directly (no staging copy for the pack step to move again)
  long long n_gapped;
  const long long* big_off;  // per gapped read: byte offset of its global scratch (big reads only)
  unsigned char* big_buf;
  int allow_fast;            // 0: every read takes the general kernel (debugging / A-B switch)
  int shortcuts;             // 0: k_corr_nw_fast fills a matrix for every read (AMG_NW_NO_SHORTCUT=1: test switch)
  unsigned char* route;      // per gapped read, or nullptr (amg_correct_reads): what settled it in k_corr_nw_fast, a
                             // NW_ROUTE_* code (amg_nw_probe)
};
// how a carry-over was made (amg_nw_probe's route byte; include/amg.h).  k_corr_nw_fast writes the first three, the
// others follow from the record and the sizes of k_nw_sizes
enum { NW_ROUTE_NONE = 0, NW_ROUTE_EQUAL = 1, NW_ROUTE_CERT = 2, NW_ROUTE_FILL = 3, NW_ROUTE_LDS = 4, NW_ROUTE_GLOBAL = 5 };

// ---- compaction into the corrected CSR: a read is kept when len(list_of_genes) > 0 (:1130)
struct PackArgs {
  CorrArgs a;
  const long long* new_idx;    // exscan(new_len > 0)
  const long long* new_off;    // exscan(new_len)
  const unsigned char* final_cls;
  int* o_tok;
  long long* o_off;
  int* o_orig;
  unsigned char* o_changed;
  long long* o_src;          // per corrected read: token index of its first gene in the current read set (-1: re-threaded)
  const long long* pos_new;  // per read: pool index of a re-threaded read's new positions
  long long* o_posoff;       // per corrected read: pool index of its positions
  long long* o_rl;
  long long out_reads, out_tokens;  // the corrected CSR's last offset: o_off[out_reads] = out_tokens
  unsigned long long* dead_kept;    // dead windows of the reads that keep their original genes: 16 partial sums, 16 words apart
};

// ------------------------------------------------------------------ one amg_correct_reads call, host side
// A/B, debugging and test switches of the environment.  Read at the top of EVERY call (tests flip them between two
// calls on one engine); NAME=1 switches the named thing off.
struct CorrSwitches {
  bool gap_memo;            // AMG_NO_GAP_MEMO: every read searches its own paths
  bool gap_dfs_wave;        // AMG_GAP_DFS_WAVE=1 (switches ON): the memo's questions a wave each (k_gap_dfs) at every k
  bool fast_gapped;         // AMG_NO_FAST_GAPPED: every gapped read through the general one-thread kernel
  bool lean_gapped;         // AMG_NO_LEAN_GAPPED: every gapped read through the wave-per-read kernel
  int fast_nw;              // AMG_NO_FAST_NW: every carry-over through the general kernel
  int nw_shortcuts;         // AMG_NW_NO_SHORTCUT: k_corr_nw_fast fills a matrix for every read
  const char* node_bound;   // AMG_TEST_NODE_BOUND=<n>: test hook, a node bound that does not hold (nullptr: unset)
  bool routes;              // AMG_CORR_ROUTES=1: test hook, tally which read took which route (amg_correct_routes)
  const char* gap_pool;     // AMG_TEST_GAP_POOL=<n>: test hook, ints of k_corr_gapped's path pool at the first attempt
  const char* memo_spill;   // AMG_TEST_MEMO_SPILL=<n>: test hook, ints of the memo pool behind the inline stretches
};

// The scratch plan: every array of a call that is carved out of a shared buffer, under the name the steps use.
// (The per-read arrays must survive the scans, so each group has a buffer of its own.)  The fields of one line share
// one allocation, in the order written; the plan functions of amg_correct.hip own the buffers behind them.
struct CorrScratch {
  size_t per_read = 0;  // n_reads + 2: the stride of the per-read arrays
  unsigned char *cls = nullptr, *final_cls = nullptr;
  int *r_start = nullptr, *r_end = nullptr;
  long long *nw_size = nullptr, *nw_off = nullptr;                           // in r_end's allocation, behind it at the next 16
                                                                             // bytes: per GAPPED read, global NW scratch bytes + prefix
  unsigned int *bound = nullptr, *new_len = nullptr, *flag = nullptr;        // (cleared as one range)
  long long *tmp_off = nullptr, *new_idx = nullptr, *new_off = nullptr;
  int* tmp_tok = nullptr;                                                    // staged genes of the re-threaded reads
  long long *plen = nullptr, *poffs = nullptr, *pos_new = nullptr;           // (carry-over only): per gapped read new
                                                                             // positions + prefix, per read its pool index
  // counters.  ST_MISC of the status words: the number of reads for the general carry-over kernel (k_nw_sizes)
  unsigned long long* n_general = nullptr;
  unsigned long long* n_runs = nullptr;     // gm_ctr + 16: [16 x 16 words] ([0, 16) belong to the path memo)
  unsigned long long* max_bound = nullptr;  // n_runs + 8: the largest staging bound, a partial maximum beside each partial sum
  unsigned long long* dead_kept = nullptr;  // n_runs + 256: [16 x 16 words] (k_corr_pack), then the live nodes
  bool count_alive = false;                 // k_count_alive rides along (large graphs: the next build's table)
  // OUTPUT buffers of the correction that serve as scratch under these names until the shape step is over and
  // amg_correct_reads re-ensures them for their own role; nothing below is read after that
  DevBuf* glist = nullptr;      // c_orig:    int[n_gapped] the gapped reads (also read by k_nw_sizes)
  DevBuf* cand = nullptr;       // c_gstart:  candidate scratch of k_corr_gapped
  DevBuf* pool = nullptr;       // c_gend:    its path pool
  DevBuf* need_slow = nullptr;  // c_changed: uint8[n_gapped] reads the fast kernel hands to k_corr_gapped
};

// what the host has read back, by the step whose fetch brought it
struct CorrCounts {
  long long tmp_total = 0, n_gapped = 0, total_runs = 0;  // classify
  unsigned long long max_bound = 0;
  bool carry = false;  // positions are carried over: there are gapped reads and gene positions
  long long out_reads = 0, out_tokens = 0, big_total = 0, pos_total = 0;  // shape
  unsigned long long n_general = 0;
  long long n_queries = 0;   // gapped: questions of the path memo (0 without memo)
  int pool_retries = 0;      // gapped: attempts of k_corr_gapped beyond the first
  bool lean_ran = false, fast_ran = false, memo = false;
};

// the position pools of the CURRENT reads (the only fields the gather kernels of amg_corrected.hip read); again
// after anything that may have moved pos1_s / pos1_e
static void fill_pos_args(amg_ctx* c, CorrArgs& a) {
  a.p0s = c->have_pos ? c->gene_start.as<long long>() : nullptr;
  a.p0e = c->have_pos ? c->gene_end.as<long long>() : nullptr;
  a.p1s = c->pos1_s.as<long long>();
  a.p1e = c->pos1_e.as<long long>();
  a.n0 = c->pos_n0;
  a.pos_off = (c->have_pos && !c->pos_identity) ? c->pos_off.as<long long>() : nullptr;
}

// ---- the steps that live with their kernels
// stage correct_gapped: a has tmp_tok; writes the staged genes, new_len and final_cls of the gapped reads
int corr_gapped(amg_ctx* c, const CorrSwitches& sw, const CorrScratch& S, const CorrArgs& a, CorrCounts& n);
// inside the shape step: sizes of the carry-over's scratch and products, their totals appended to `shape`
int corr_nw_sizes(amg_ctx* c, const CorrSwitches& sw, const CorrScratch& S, const CorrArgs& a, long long n_gapped,
                  FetchList& shape);
// stage correct_positions: room for what this call produces (may MOVE the pools: fill_pos_args again), then the kernels
int corr_grow_pos_pools(amg_ctx* c, const CorrCounts& n);
int corr_positions(amg_ctx* c, const CorrSwitches& sw, const CorrScratch& S, const CorrArgs& a, const CorrCounts& n,
                   unsigned char* route = nullptr);  // route: NwArgs::route (amg_nw_probe only)

// ---- the parts of stage correct_gapped, each with its kernels (corr_gapped, amg_correct_gapped.hip, runs them)
// amg_gap_memo.hip: the questions of the None runs entered and answered; *gq: per-read question slots (nullptr: no memo)
int corr_gap_memo(amg_ctx* c, const CorrSwitches& sw, const CorrArgs& a, CorrCounts& n, const int** gq);
// amg_gap_lean.hip: k_corr_gapped_lean over every gapped read; qgene: the memo's genes, left: a GL_* code per read
void corr_gapped_lean_launch(amg_ctx* c, const GapArgs& G, const int* qgene, unsigned char* left);
// amg_gap_fast.hip: k_corr_gapped_fast; left == nullptr: every gapped read, else the reads flagged there
void corr_gapped_fast_launch(amg_ctx* c, const GapArgs& G, const unsigned char* left);
// amg_gap_general.hip: room for k_corr_gapped (candidate scratch, need_slow, the first path pool), then the kernel
// over the reads flagged in need_slow; it grows the pool (G.pool, G.pool_cap) and runs again while one overflows it
struct GeneralRoom {
  unsigned int cand_stride;
  unsigned long long pool_cap;
};
int corr_general_room(amg_ctx* c, const CorrSwitches& sw, const CorrScratch& S, const CorrCounts& n, GeneralRoom& room);
int corr_gapped_general(amg_ctx* c, const CorrScratch& S, GapArgs& G, CorrCounts& n);

// ---- route report (amg_correct_routes.hip), only with CorrSwitches::routes: small tally kernels behind the steps
int routes_begin(amg_ctx* c);
// at the end of corr_gapped, while need_slow (a borrowed output buffer) and the lean kernel's flags still hold
int routes_gapped(amg_ctx* c, const CorrScratch& S, const CorrCounts& n, const unsigned char* need_slow, const int* gq);
int routes_nw(amg_ctx* c, const CorrScratch& S, const CorrCounts& n);  // from the NwRec records, sizes and final_cls
int routes_end(amg_ctx* c, const CorrCounts& n);                       // the call's one extra read-back
