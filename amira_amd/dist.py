"""Multi-GPU build: read shards + key-owner table merge, the reference's
build_multiprocessed_graph + merge_graphs (graph_utils.py:94-124) as ONE graph on every rank.

The merge lives behind the C ABI (include/amg.h "multi-GPU"; amira_amd/csrc/amg_dist.hip): libamg runs the device
phases AND the exchanges between them — RCCL all-to-alls to the key owners and back, an all-gather of the records each
rank holds — on the engine's own stream, with two host waits per kind of record.  What is left here:

  dist_build           one process per GPU under torch.distributed.  Backend "nccl" (= RCCL): the engine gets its own
                       communicator (the unique id travels through the process group once) and `amg_dist_merge` does the
                       rest.  Backend "gloo" (functional tests: ranks that share one GPU, no RCCL): the exchanges libamg
                       asks for (`amg_dist_merge_next`) are performed here, staged through the host.
  dist_build_loopback  W emulated ranks in ONE process on one GPU (`amg_dist_merge_local`): tests, tools/scaling_model.py.

What the reference asks of EVERY read of a graph before the first cleaning sweep and at k selection — the depth by read
length, AMR trimming, the AMR reads per component (amg_dist_walk*, amira_amd/csrc/amg_dist_walk.hip) — runs on the merged
graph over the same transports: dist_depth_by_length, dist_remove_non_amr_nodes, dist_component_amr_reads,
dist_mean_node_coverages and dist_choose_kmer_size take the rank's engine (and its process group), their *_loopback
twins the engines of all emulated ranks.
"""
import numpy as np

from . import _ffi
from .engine import Engine


def _group_info(group):
    import torch.distributed as dist
    return dist.get_world_size(group), dist.get_rank(group), dist.get_backend(group)


def ensure_transport(engine, group=None):
    """the engine as a rank of `group`: "rccl" — its own RCCL communicator, made once per (engine, group) — or "host"
    (gloo: the caller of libamg performs the exchanges)"""
    import torch.distributed as dist
    world, rank, backend = _group_info(group)
    mode = "host" if backend == "gloo" else "rccl"
    have = getattr(engine, "_dist", None)
    if have == (world, rank, mode, id(group)):
        return mode
    if mode == "rccl":
        # the 128 bytes that name the communicator: made on the group's first rank, handed round by the group itself
        box = [Engine.dist_unique_id() if rank == 0 else None]
        dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        engine.dist_init(box[0], rank, world)
    else:
        engine.dist_init_external(rank, world)
    engine._dist = (world, rank, mode, id(group))
    return mode


def perform_host(engine, x, group=None):
    """one exchange of a merged build (an _ffi.Xfer: device pointers, host counts) over a transport that moves HOST
    memory (gloo): device -> host, the collective, host -> device"""
    import torch
    import torch.distributed as dist
    world = dist.get_world_size(group)
    eb = int(x.elem_bytes)
    if x.kind == _ffi.XFER_ALL_TO_ALL:
        sc = [int(x.send_counts[p]) * eb for p in range(world)]
        rc = [int(x.recv_counts[p]) * eb for p in range(world)]
        send = np.empty(sum(sc), np.uint8)
        engine.copy_d2h(x.send, send)
        recv = torch.empty(sum(rc), dtype=torch.uint8)
        dist.all_to_all_single(recv, torch.from_numpy(send), rc, sc, group=group)
        engine.copy_h2d(x.recv, recv.numpy())
    elif x.kind == _ffi.XFER_ALL_GATHER:
        n = int(x.count) * eb
        send = np.empty(n, np.uint8)
        engine.copy_d2h(x.send, send)
        recv = torch.empty(world * n, dtype=torch.uint8)
        dist.all_gather_into_tensor(recv, torch.from_numpy(send), group=group)
        engine.copy_h2d(x.recv, recv.numpy())
    else:
        raise ValueError(f"unknown exchange kind {x.kind}")


def dist_build(engine, k, group=None, min_node_cov=1, min_edge_cov=1):
    """Collective: call on every rank with its own engine (reads already set, rank r holding the reads after rank
    r - 1's).  min_node_cov / min_edge_cov > 1 fuse filter_graph into the merge.  Failures of any rank reach every rank
    (AmgError); a merge-key collision makes all ranks repeat the build with the next seed, inside libamg."""
    if ensure_transport(engine, group) == "rccl":
        engine.dist_merge(k, min_node_cov, min_edge_cov)
        return
    engine.dist_merge_begin(k, min_node_cov, min_edge_cov)
    while True:
        x = engine.dist_merge_next()
        if x is None:
            return
        perform_host(engine, x, group)


def dist_build_loopback(engines, k, min_node_cov=1, min_edge_cov=1):
    """Emulate len(engines) ranks in ONE process (tests on a single GPU, the scaling model): the device phases are
    exactly those of dist_build, the exchanges device copies."""
    Engine.dist_merge_local(engines, k, min_node_cov, min_edge_cov)


# ---- the read walks on a merged graph (collective: every rank calls with the same arguments)
def _walk(target, which, flags=None, min_genes=None, group=None):
    """one walk over the reads of all ranks; target: this rank's engine (process group `group`), or the list of the
    engines of all emulated ranks (loop-back).  Returns the answer as amg_dist_walk* lay it out."""
    if isinstance(target, (list, tuple)):
        return target[0].dist_walk_local(list(target), which, flags, min_genes)   # (a static method of Engine)
    if ensure_transport(target, group) == "rccl":
        return target.dist_walk(which, flags, min_genes)
    target.dist_walk_begin(which, flags, min_genes)
    while True:
        x = target.dist_walk_next()
        if x is None:
            return target.dist_walk_result()
        perform_host(target, x, group)


def _depth_by_length(target, min_genes, group=None):
    out = _walk(target, _ffi.WALK_DEPTH, None, min_genes, group)
    return out[:-1], int(out[-1])


def _remove_non_amr_nodes(target, gene_flags, group=None):
    return int(_walk(target, _ffi.WALK_AMR_TRIM, gene_flags, None, group)[0])


def _component_amr_reads(target, gene_flags, min_genes, group=None):
    out = _walk(target, _ffi.WALK_COMPONENT_READS, gene_flags, [int(min_genes)], group)
    nc = len(out) // 2
    return out[:nc], out[nc:]


def _mean_node_coverages(target, group=None):
    from .graph_utils import mean_of_ints
    ks = list(range(3, 16, 2))
    pairs, n_alive = _depth_by_length(target, ks, group)
    return {k: mean_of_ints(p, n_alive) for k, p in zip(ks, pairs.tolist())}


def _choose_kmer_size(target, overall_mean_node_coverage, gene_flags, group=None):
    from .graph_utils import components_valid
    geneMer_size = 3
    if overall_mean_node_coverage >= 20:
        for k in range(3, 16, 2):
            if isinstance(target, (list, tuple)):
                dist_build_loopback(list(target), k)
            else:
                dist_build(target, k, group)
            n_reads, n_long = _component_amr_reads(target, gene_flags, 2 * k - 1, group)
            if components_valid(n_reads.tolist(), n_long.tolist()):
                geneMer_size = k
            else:
                break
    return geneMer_size


def dist_depth_by_length(engine, min_genes, group=None):
    """Engine.depth_by_length over the reads of all ranks: (pairs, n_alive), the same on every rank"""
    return _depth_by_length(engine, min_genes, group)


def dist_depth_by_length_loopback(engines, min_genes):
    return _depth_by_length(engines, min_genes)


def dist_remove_non_amr_nodes(engine, gene_flags, group=None):
    """Engine.remove_non_amr_nodes (remove_non_AMR_associated_nodes, construct_graph.py:2941-2959) on the merged graph:
    a node stays when a read of ANY rank with a live window on a gene of interest reaches it.  Every rank ends with the
    same graph and returns the same number of removed nodes; its own reads' windows are masked and its own reads marked
    for correction."""
    return _remove_non_amr_nodes(engine, gene_flags, group)


def dist_remove_non_amr_nodes_loopback(engines, gene_flags):
    return _remove_non_amr_nodes(engines, gene_flags)


def dist_component_amr_reads(engine, gene_flags, min_genes, group=None):
    """Engine.component_amr_reads over the reads of all ranks: (n_reads, n_long), entry c for the component with id c + 1"""
    return _component_amr_reads(engine, gene_flags, min_genes, group)


def dist_component_amr_reads_loopback(engines, gene_flags, min_genes):
    return _component_amr_reads(engines, gene_flags, min_genes)


def dist_mean_node_coverages(engine, group=None):
    """the dict get_overall_mean_node_coverages (graph_utils.py:299-313) returns for the graph of all ranks' reads:
    {k: mean over the alive nodes of the node's reads with >= k genes} for k = 3, 5, .., 15, values as statistics.mean
    gives them (graph_utils.mean_of_ints)"""
    return _mean_node_coverages(engine, group)


def dist_mean_node_coverages_loopback(engines):
    return _mean_node_coverages(engines)


def dist_choose_kmer_size(engine, overall_mean_node_coverage, gene_flags, group=None):
    """choose_kmer_size (graph_utils.py:258-296) on read shards: with a mean coverage of at least 20, merged builds at
    k = 3, 5, .., 15, after each the AMR reads per component with min_genes = 2k - 1; k is taken while in every component
    with such reads at least 80 % of them are that long, and the first k that fails ends the search (the reference's
    early break).  gene_flags: a byte per gene rank.  The engines are left with the LAST graph tried, not the chosen
    one: the caller builds again at the k returned, as the reference's main() does after choosing."""
    return _choose_kmer_size(engine, overall_mean_node_coverage, gene_flags, group)


def dist_choose_kmer_size_loopback(engines, overall_mean_node_coverage, gene_flags):
    return _choose_kmer_size(engines, overall_mean_node_coverage, gene_flags)
