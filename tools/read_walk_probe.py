#!/usr/bin/env python
"""Times the three driver calls that walk the reads of a built graph — get_overall_mean_node_coverages,
GeneMerGraph.remove_non_AMR_associated_nodes, choose_kmer_size — through the drop-in, on the cfg-3 workload of bench.py
(1 M reads x 60 genes, 20 000-gene vocabulary, 2 % wrong genes, k = 5) with 25 genes of interest.

One process measures one tree: --root names the checkout whose amira_amd is imported (default: this one), so that the
same file times a parent checkout built beside it.  Each call gets a warm-up and --repeats timed runs (host clock around
a call that ends with its result on the host); the line per call gives median, min and max.  A call that changes the
graph (the trimming) gets a freshly built graph per run, built outside the timed window.  Where the tree has the device
entry points, the kernels' own times (amg_last_timings) are reported beside the call.

    python tools/read_walk_probe.py [--root DIR] [--reads N] [--calls depth,trim,choose] [--repeats 5] [--out FILE]

Prints one JSON line per call (and appends it to --out).  Not a test and not the benchmark."""
import argparse
import json
import os
import statistics
import sys
import time

CFG3 = dict(L=60, V=20_000, k=5, err=0.02, seed=20250905 + 3)   # bench.py WORKLOADS["cfg3"]
N_GENES_OF_INTEREST = 25


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--calls", default="depth,trim,choose")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import numpy as np
    from amira_amd import GeneMerGraph, graph_utils as gu, synth
    from amira_amd.io import TokenizedReads
    from amira_amd.tokens import Vocabulary

    w, N = CFG3, args.reads
    ids, sts = synth.block_reads(w["seed"], 0, N, w["L"], w["V"], w["err"], n_amr=0)     # as bench.make_tokens
    names = synth.gene_names(w["V"], 0)
    vocab = Vocabulary(names)
    rank = np.array([vocab.rank[n] for n in names], dtype=np.int64)[ids]
    toks = np.where(sts == 1, vocab.V + rank, vocab.V - 1 - rank).astype(np.int32).reshape(-1)
    offs = np.arange(N + 1, dtype=np.int64) * w["L"]
    read_ids = synth.read_names(0, N)
    genes = [names[i * (w["V"] // N_GENES_OF_INTEREST) + 7] for i in range(N_GENES_OF_INTEREST)]

    def reads():
        return TokenizedReads(vocab, toks, offs, read_ids)

    def report(call, times, **more):
        ms = sorted(1e3 * t for t in times)
        line = {"call": call, "root": os.path.abspath(args.root), "reads": N, "genes_of_interest": len(genes),
                "repeats": len(ms), "median_ms": round(statistics.median(ms), 3), "min_ms": round(ms[0], 3),
                "max_ms": round(ms[-1], 3), **more}
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(text + "\n")

    def timed(fn):
        t = time.perf_counter()
        r = fn()
        return time.perf_counter() - t, r

    def kernel_ms(graph):
        return {name: round(ms, 4) for name, ms in graph._engine.timings()}

    calls = args.calls.split(",")
    device_calls = hasattr(GeneMerGraph, "_gene_flags")   # this tree answers on the device
    if "depth" in calls:
        g = GeneMerGraph(reads(), w["k"])
        times, result = [], None
        for i in range(args.warmup + args.repeats):
            dt, result = timed(lambda: gu.get_overall_mean_node_coverages(g))
            if i >= args.warmup:
                times.append(dt)
        more = {"result_k3": float(result[3])}
        if device_calls:
            more["kernels_ms"] = kernel_ms(g)
        report("get_overall_mean_node_coverages", times, **more)
        g.close()
    if "trim" in calls:
        times, left, kern = [], None, None
        for i in range(args.warmup + args.repeats):
            g = GeneMerGraph(reads(), w["k"])
            g._engine.sync()
            dt, _ = timed(lambda: g.remove_non_AMR_associated_nodes(genes))
            if i >= args.warmup:
                times.append(dt)
            if device_calls:
                kern = kernel_ms(g)
            left = g.get_total_number_of_nodes()
            g.close()
        more = {"nodes_left": left}
        if kern is not None:
            more["kernels_ms"] = kern
        report("remove_non_AMR_associated_nodes", times, **more)
    if "choose" in calls:
        times, result = [], None
        for i in range(args.warmup + args.repeats):
            dt, result = timed(lambda: gu.choose_kmer_size(25, reads(), 1, None, genes))
            if i >= args.warmup:
                times.append(dt)
        more = {"result": result}
        if device_calls:
            # the walk of one graph by itself: its kernels' own time and the call's
            g = GeneMerGraph(reads(), w["k"])
            flags = g._gene_flags(genes)
            walk = []
            for i in range(args.warmup + args.repeats):
                dt, _ = timed(lambda: g._engine.component_amr_reads(flags, 2 * w["k"] - 1))
                if i >= args.warmup:
                    walk.append(1e3 * dt)
            more["component_amr_reads_k5_median_ms"] = round(statistics.median(walk), 3)
            more["kernels_ms"] = kernel_ms(g)
            g.close()
        report("choose_kmer_size", times, **more)


if __name__ == "__main__":
    main()
