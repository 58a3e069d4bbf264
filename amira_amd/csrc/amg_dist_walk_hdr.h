// amg_dist_walk_hdr.h — the header every rank of a read walk across ranks (amg_dist_walk.hip) contributes to the walk's
// first all-gather, and what the ranks conclude from the W headers they then all hold: go on, or give up TOGETHER.
// Plain C++ without a HIP header: dist_walk_check.cpp runs it on canned headers under the host sanitizers.
//
//   word 0  which        AMG_WALK_*
//        1  status       0, or the AMG_E_* code (< 0) of this rank's local phase
//        2  k            gene-mer size of the graph
//        3  n            lengths asked for (depth), 1 (component reads), 0 (AMR trimming)
//        4  n_nodes      array size of the graph, dead nodes included
//        5  n_components component reads only, else 0
//        6  hash         of the arguments: min_genes[0 .. n) and / or the gene flags as 0 / 1 bytes
//        7  two_v        twice the vocabulary
// The size of the data exchange that follows is computed from an AGREED header, never from a rank's own state.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>

#define DW_HDR_WORDS 8
#define DW_DEPTH_LENGTHS 16  // the depth walk's payload, pairs[16], travels behind its header (RW_MAX_LENGTHS)
enum { DW_H_WHICH = 0, DW_H_STATUS, DW_H_K, DW_H_N, DW_H_NODES, DW_H_COMPS, DW_H_HASH, DW_H_TWO_V };
enum { DW_DEPTH = 1, DW_AMR_TRIM = 2, DW_COMPONENT_READS = 3 };  // == AMG_WALK_* (include/amg.h)

// FNV-1a over 64-bit values, so that the hash does not depend on how the caller laid its arguments out
static inline uint64_t dw_hash_begin() { return 0xcbf29ce484222325ull; }
static inline uint64_t dw_hash_add(uint64_t h, uint64_t v) {
  for (int i = 0; i < 8; ++i) {
    h ^= (v >> (8 * i)) & 0xffull;
    h *= 0x100000001b3ull;
  }
  return h;
}
static inline uint64_t dw_hash_args(const uint8_t* gene_flags, int64_t n_flags, const int32_t* min_genes, int32_t n) {
  uint64_t h = dw_hash_begin();
  h = dw_hash_add(h, gene_flags ? (uint64_t)n_flags + 1 : 0);
  uint64_t word = 0;
  for (int64_t i = 0; gene_flags && i < n_flags; ++i) {  // 64 flags a step
    word |= (uint64_t)(gene_flags[i] != 0) << (i & 63);
    if ((i & 63) == 63 || i + 1 == n_flags) {
      h = dw_hash_add(h, word);
      word = 0;
    }
  }
  h = dw_hash_add(h, min_genes ? (uint64_t)n + 1 : 0);
  for (int32_t j = 0; min_genes && j < n; ++j) h = dw_hash_add(h, (uint64_t)(int64_t)min_genes[j]);
  return h;
}

// words of this walk's message in the FIRST all-gather: the depth walk's sums ride behind the header
static inline int dw_first_words(int which) { return which == DW_DEPTH ? DW_HDR_WORDS + DW_DEPTH_LENGTHS : DW_HDR_WORDS; }

// The verdict on `world` blocks of `stride` words (a header at the start of each), as gathered on rank `self`: 0 = the
// ranks agree and none failed; else a message in msg.  Every rank computes the same verdict from the same blocks.
static inline int dw_judge(const int64_t* blocks, int world, int stride, int self, char* msg, size_t cap) {
  static const char* const kField[DW_HDR_WORDS] = {"walk", "status", "k", "n", "n_nodes", "n_components", "arguments", "two_v"};
  if (msg && cap) msg[0] = 0;
  if (!blocks || world < 1 || stride < DW_HDR_WORDS || self < 0 || self >= world) {
    if (msg) snprintf(msg, cap, "bad header block");
    return 1;
  }
  for (int r = 0; r < world; ++r) {
    const int64_t st = blocks[(size_t)r * stride + DW_H_STATUS];
    if (st != 0) {
      if (msg) snprintf(msg, cap, "the local phase of rank %d failed (code %lld)", r, (long long)st);
      return 1;
    }
  }
  const int64_t* mine = blocks + (size_t)self * stride;
  for (int r = 0; r < world; ++r)
    for (int f = 0; f < DW_HDR_WORDS; ++f)
      if (blocks[(size_t)r * stride + f] != mine[f]) {
        if (msg) {
          if (f == DW_H_HASH)
            snprintf(msg, cap, "rank %d was called with other %s than rank %d", r, kField[f], self);
          else
            snprintf(msg, cap, "rank %d has %s = %lld, rank %d has %lld", r, kField[f], (long long)blocks[(size_t)r * stride + f],
                     self, (long long)mine[f]);
        }
        return 1;
      }
  const int64_t which = mine[DW_H_WHICH];
  if (which < DW_DEPTH || which > DW_COMPONENT_READS || mine[DW_H_NODES] < 0 || mine[DW_H_COMPS] < 0 ||
      mine[DW_H_NODES] >= (1ll << 31) || mine[DW_H_COMPS] > mine[DW_H_NODES]) {
    if (msg) snprintf(msg, cap, "a header no walk makes");
    return 1;
  }
  return 0;
}

// 64-bit words every rank contributes to the DATA exchange of an agreed header (0: there is none — the depth walk's sums
// came with the header, a graph without nodes has nothing to trim, one without components nothing to count)
static inline int64_t dw_data_words(const int64_t* hdr) {
  switch (hdr[DW_H_WHICH]) {
    case DW_AMR_TRIM: return (hdr[DW_H_NODES] + 63) / 64;  // one keep bit per node
    case DW_COMPONENT_READS: return 2 * hdr[DW_H_COMPS];   // n_reads[], n_long[]
    default: return 0;
  }
}
