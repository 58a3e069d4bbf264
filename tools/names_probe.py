#!/usr/bin/env python3
"""What the 256-bit node / edge names cost on the host and on the device, and where the two cross.

    python tools/names_probe.py [--out profiles/names_host_vs_device.json] [--max-nodes 1000000]

For graphs of about 10^3, 10^4, 10^5 and 10^6 nodes at k = 5 (and 10^5 at k = 15) — reads cut from a random gene
sequence, so nearly every window is a node of its own and there are two directed edges per adjacency — it times

  (a) the host recipe, item by item, as the object view made every name before the device did: a node from its row of
      tokens (tuple of signed gene hashes, pickle.dumps, sha256, int), an edge from its two node names (two such
      hashes and a min), WITHOUT the Node / Edge objects the view also built for an edge;
  (b) the device call and the conversion of its digests to Python ints (Engine.node_names / edge_names +
      ints_of_digests): what a view pays;
  (c) the kernels alone by the ctx's stage events, with their share of an integer-issue roof: 1 500 vector integer
      operations per SHA-256 block (64 rounds of about 16 with funnel-shift rotates, bit-select and three-operand
      adds and xors, 48 schedule steps of about 10) against 256 CUs x 64 lanes x 2.4 GHz.  The message bytes a lane
      assembles are not counted: the share says how near the whole kernel is to SHA alone at full issue rate.

Small batches (16 ... 4 096 ids of the 10^5 graph, best of 5) show where (b) drops below (a): graph_view.NAMES_BATCH_MIN
and NAMES_ONE_BY_ONE are that size rounded up to a power of two.  One JSON document on stdout and in --out.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

VALU_LANE_OPS_PER_S = 256 * 64 * 2.4e9
OPS_PER_BLOCK = 1500


def blocks(k):
    """SHA-256 blocks of a name of k entries of the usual 34 or 35 bytes"""
    return (35 * k + 15 + 9 + 63) // 64


def linear_reads(seed, n_nodes, k, V=20000, read_len=60):
    """tokens / offsets of reads cut from one random gene sequence, overlapping by k - 1 genes: about n_nodes nodes"""
    rng = np.random.default_rng(seed)
    total = n_nodes + k - 1
    seq = rng.integers(0, 2 * V, total).astype(np.int32)
    for i in range(1, total):            # no gene next to its own reverse: no window is its own reverse complement
        while seq[i] == 2 * V - 1 - seq[i - 1]:
            seq[i] = rng.integers(0, 2 * V)
    starts = list(range(0, total - k + 1, read_len - k + 1))
    reads = [seq[a:a + read_len] for a in starts]
    offs = np.zeros(len(reads) + 1, np.int64)
    np.cumsum([len(r) for r in reads], out=offs[1:])
    return np.concatenate(reads), offs, 2 * V


def best_of(fn, reps):
    best = None
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t
        best = dt if best is None or dt < best else best
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "names_host_vs_device.json"))
    ap.add_argument("--max-nodes", type=int, default=1000000)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    from amira_amd import Engine
    from amira_amd.construct_gene import hashlib_hash
    from amira_amd.graph_view import ints_of_digests, node_hash_of_tokens
    from amira_amd.names import names_ok
    from amira_amd.tokens import Vocabulary

    V = 20000
    vocab = Vocabulary([f"g{i}" for i in range(V)])
    names = vocab.gene_names(args.device)
    out = {"probe": "names", "names_ok": names_ok(), "valu_lane_ops_per_s": VALU_LANE_OPS_PER_S,
           "ops_per_sha_block": OPS_PER_BLOCK, "graphs": [], "small_batches": []}
    eng = Engine(args.device)
    try:
        cases = [(n, 5) for n in (1000, 10000, 100000, 1000000) if n <= args.max_nodes] + [(100000, 15)]
        for n_nodes, k in cases:
            toks, offs, two_v = linear_reads(n_nodes + k, n_nodes, k, V)
            eng.set_reads(toks, offs, two_v)
            eng.build(k)
            nodes, edges = eng.nodes(), eng.edges()
            D, E = len(nodes["coverage"]), len(edges["coverage"])
            reps = 3 if D <= 100000 else 1
            # (a) the host recipe
            rows = nodes["tokens"].tolist()
            t_host_nodes, host_names = best_of(lambda: [node_hash_of_tokens(vocab, r) for r in rows], reps)
            ends = list(zip(edges["src"].tolist(), edges["tgt"].tolist(), edges["sdir"].tolist(), edges["tdir"].tolist()))

            def host_edges():
                got = []
                for s, t, sd, td in ends:
                    a, b = host_names[s] * sd, host_names[t] * td
                    got.append(min(hashlib_hash((a, b)), hashlib_hash((-a, -b))))
                return got
            t_host_edges, host_edge_names = best_of(host_edges, reps)
            # (b) the device call and the ints
            eng.node_names(names, np.arange(min(D, 64)))   # (first launch of the process: code object load)
            t_dev_nodes, dev_names = best_of(lambda: ints_of_digests(eng.node_names(names)[0]), 3)
            t_dev_edges, dev_edge_names = best_of(lambda: ints_of_digests(eng.edge_names(names)[0]), 3)
            assert dev_names == host_names and dev_edge_names == host_edge_names
            t_call_nodes, _ = best_of(lambda: eng.node_names(names), 3)
            # (c) the kernels alone
            kern = {}
            for what, call in (("names_nodes", eng.node_names), ("names_edges", eng.edge_names)):
                best = None
                for _ in range(3):
                    eng.set_timing(False)
                    eng.set_timing(True)     # (drops the stages of the build: a names call then records its own)
                    call(names)
                    ms = sum(v for n, v in eng.timings() if n == what)
                    best = ms if best is None or ms < best else best
                kern[what] = best
            node_ops = D * blocks(k) * OPS_PER_BLOCK
            edge_ops = E * (2 * blocks(k) + 2 * blocks(2)) * OPS_PER_BLOCK
            out["graphs"].append({
                "k": k, "nodes": D, "edges": E,
                "host_us_per_node": t_host_nodes / D * 1e6, "host_us_per_edge": t_host_edges / max(E, 1) * 1e6,
                "host_ms_nodes": t_host_nodes * 1e3, "host_ms_edges": t_host_edges * 1e3,
                "device_ms_nodes": t_dev_nodes * 1e3, "device_ms_edges": t_dev_edges * 1e3,
                "device_us_per_node": t_dev_nodes / D * 1e6, "device_us_per_edge": t_dev_edges / max(E, 1) * 1e6,
                "device_call_ms_nodes_without_ints": t_call_nodes * 1e3,
                "kernel_ms_nodes": kern["names_nodes"], "kernel_ms_edges": kern["names_edges"],
                "sha_blocks_per_node": blocks(k), "sha_blocks_per_edge": 2 * blocks(k) + 2 * blocks(2),
                "int_roof_share_nodes": node_ops / VALU_LANE_OPS_PER_S / (kern["names_nodes"] * 1e-3) if kern["names_nodes"] else None,
                "int_roof_share_edges": edge_ops / VALU_LANE_OPS_PER_S / (kern["names_edges"] * 1e-3) if kern["names_edges"] else None,
            })
            if (n_nodes, k) == (100000, 5):
                rng = np.random.default_rng(1)
                for n in (16, 32, 64, 128, 256, 512, 1024, 4096):
                    ids = rng.choice(D, n, replace=False)
                    eids = rng.choice(E, n, replace=False)
                    sub = [rows[i] for i in ids.tolist()]
                    t_h, _ = best_of(lambda: [node_hash_of_tokens(vocab, r) for r in sub], 5)
                    t_d, _ = best_of(lambda: ints_of_digests(eng.node_names(names, ids)[0]), 5)
                    sube = [ends[e] for e in eids.tolist()]

                    def few_edges():
                        for s, t, sd, td in sube:
                            a, b = host_names[s] * sd, host_names[t] * td
                            min(hashlib_hash((a, b)), hashlib_hash((-a, -b)))
                    t_he, _ = best_of(few_edges, 5)
                    t_de, _ = best_of(lambda: ints_of_digests(eng.edge_names(names, eids)[0]), 5)
                    out["small_batches"].append({"n": n, "host_us_nodes": t_h * 1e6, "device_us_nodes": t_d * 1e6,
                                                 "host_us_edges": t_he * 1e6, "device_us_edges": t_de * 1e6})
    finally:
        eng.close()
    crossing = next((b["n"] for b in out["small_batches"]
                     if all(c["device_us_nodes"] < c["host_us_nodes"] and c["device_us_edges"] < c["host_us_edges"]
                            for c in out["small_batches"] if c["n"] >= b["n"])), None)
    out["device_below_host_from_n"] = crossing
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
