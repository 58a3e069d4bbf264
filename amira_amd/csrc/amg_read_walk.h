// amg_read_walk.h — the local phases of the read walks (amg_read_walk.hip): each walks the reads THIS ctx holds and
// leaves its partial answer on the device, on the ctx's stream.  amg_depth_by_length, amg_remove_non_amr_nodes and
// amg_component_amr_reads read it back as the answer; on a merged graph (amg_dist_walk.hip) it is one rank's part.
#pragma once
#include <vector>

#include "amg_internal.h"

#define RW_MAX_LENGTHS 16                    // read lengths one depth walk answers for
#define RW_DEPTH_WORDS (RW_MAX_LENGTHS + 1)  // what it writes: pairs[16], then the alive nodes

// A: out[RW_DEPTH_WORDS] (device, zeroed here): pairs[j] for j < n, out[RW_MAX_LENGTHS] = alive nodes
int rw_depth_local(amg_ctx* c, const int32_t* min_genes, int32_t n, unsigned long long* out);
// B: s4 = keep[n_nodes], a byte per node on which a read with a live AMR window has a live window; s0 = n_nodes + 8
// zeroed bytes for the kill marks of finish_kill.  Uses s1 and s5; `words` holds the flag bitmap until the stream has
// taken it (keep it until the next wait).  n_nodes > 0.
int rw_keep_local(amg_ctx* c, const uint8_t* gene_flags, std::vector<unsigned int>* words);
// C: s4 = n_reads[n_components], then n_long[n_components] (64-bit).  ensure_components first; n_components > 0; `words`
// as above.
int rw_comp_local(amg_ctx* c, const uint8_t* gene_flags, int32_t min_genes, std::vector<unsigned int>* words);
