// amg_read_walk.h — the local phases of the read walks (amg_read_walk.hip): each walks the reads THIS ctx holds and
// leaves its partial answer on the device, on the ctx's stream.  amg_depth_by_length, amg_remove_non_amr_nodes and
// amg_component_amr_reads read it back as the answer; on a merged graph (amg_dist_walk.hip) it is one rank's part.
//
// B and C return device pointers into the ctx's scratch.  They hold until the caller's fold (finish_kill, the read-back)
// as long as nothing else runs on the ctx in between but amg_copy_* and, across ranks, the walk's own calls
// (amg_dist_walk_next / _result): any other entry point may take the scratch for itself.  finish_kill refuses marks
// that were overtaken that way.
#pragma once
#include <vector>

#include "amg_internal.h"

#define RW_MAX_LENGTHS 16                    // read lengths one depth walk answers for
#define RW_DEPTH_WORDS (RW_MAX_LENGTHS + 1)  // what it writes: pairs[16], then the alive nodes

// A: out[RW_DEPTH_WORDS] (device, zeroed here): pairs[j] for j < n, out[RW_MAX_LENGTHS] = alive nodes
int rw_depth_local(amg_ctx* c, const int32_t* min_genes, int32_t n, unsigned long long* out);
// B: keep[n_nodes], a byte per node on which a read with a live AMR window has a live window, and zeroed kill marks for
// the caller to mark the nodes not kept in.  `words` holds the flag bitmap until the stream has taken it (keep it until
// the next wait).  n_nodes > 0.
struct RwKeep {
  const unsigned char* keep = nullptr;
  KillMarks marks;
};
int rw_keep_local(amg_ctx* c, const uint8_t* gene_flags, std::vector<unsigned int>* words, RwKeep* out);
// C: n_reads[n_components] and, behind it, n_long[n_components] (64-bit; one range of 2 n_components words).
// ensure_components first; n_components > 0; `words` as above.
struct RwComp {
  const unsigned long long *n_reads = nullptr, *n_long = nullptr;
  long long n_components = 0;
};
int rw_comp_local(amg_ctx* c, const uint8_t* gene_flags, int32_t min_genes, std::vector<unsigned int>* words, RwComp* out);
