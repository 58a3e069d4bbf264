#!/usr/bin/env python
"""Times the read walks of a merged graph on EMULATED ranks (amg_dist_walk_local: W engines of one process on one GPU, the
exchanges as device copies) beside the single-engine calls on the unsharded graph, on the cfg-3 workload of bench.py
(1 M reads x 60 genes, 20 000-gene vocabulary, 2 % wrong genes, k = 5) with 25 genes of interest.

What the figures are: the W local walks run one after the other on one GPU, so the loop-back time is the SUM of the ranks'
device work plus the exchanges' copies and host waits — an upper bound for nothing and a model of nothing; it shows what
the state machine and the folds add to the walks.  No run across GPUs is made here.

Each call gets --warmup runs and --repeats timed runs, single engine and loop-back alternating (host clock around calls
that end with their answer on the host); the trimming gets freshly built graphs per run, built outside the timed window.

    python tools/dist_walk_probe.py [--reads N] [--world W] [--repeats 9] [--out FILE]

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
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--world", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    from amira_amd import Engine, dist, synth
    from amira_amd.tokens import Vocabulary

    w, N, W = CFG3, args.reads, args.world
    ids, sts = synth.block_reads(w["seed"], 0, N, w["L"], w["V"], w["err"], n_amr=0)     # as bench.make_tokens
    names = synth.gene_names(w["V"], 0)
    vocab = Vocabulary(names)
    rank = np.array([vocab.rank[n] for n in names], dtype=np.int64)[ids]
    toks = np.where(sts == 1, vocab.V + rank, vocab.V - 1 - rank).astype(np.int32).reshape(-1)
    offs = np.arange(N + 1, dtype=np.int64) * w["L"]
    flags = np.zeros(vocab.V, np.uint8)
    for i in range(N_GENES_OF_INTEREST):
        flags[vocab.rank[names[i * (w["V"] // N_GENES_OF_INTEREST) + 7]]] = 1
    k, lengths = w["k"], list(range(3, 16, 2))

    single = Engine(0)
    single.set_reads(toks, offs, vocab.two_v)
    ranks = []
    for r in range(W):
        lo, hi = (r * N) // W, ((r + 1) * N) // W
        e = Engine(0)
        e.set_reads(toks[offs[lo]:offs[hi]], offs[lo:hi + 1] - offs[lo], vocab.two_v)
        ranks.append(e)

    def build_both():
        single.build(k)
        dist.dist_build_loopback(ranks, k)
        single.sync()
        for e in ranks:
            e.sync()

    def timed(fn):
        t = time.perf_counter()
        r = fn()
        return 1e3 * (time.perf_counter() - t), r

    def spread(ms):
        ms = sorted(ms)
        return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(ms[0], 3), "max_ms": round(ms[-1], 3)}

    def report(call, one, many, same, **more):
        line = {"call": call, "reads": N, "emulated_ranks": W, "repeats": len(one), "single_engine": spread(one),
                "loopback": spread(many), "answers_equal": bool(same), **more}
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(text + "\n")

    build_both()
    for call, f_one, f_many in (
            ("depth_by_length", lambda: single.depth_by_length(lengths),
             lambda: dist.dist_depth_by_length_loopback(ranks, lengths)),
            ("component_amr_reads", lambda: single.component_amr_reads(flags, 2 * k - 1),
             lambda: dist.dist_component_amr_reads_loopback(ranks, flags, 2 * k - 1))):
        one, many, same = [], [], True
        for i in range(args.warmup + args.repeats):
            (t1, a), (t2, b) = timed(f_one), timed(f_many)
            same = same and np.array_equal(np.asarray(a[0]), np.asarray(b[0])) and np.array_equal(np.asarray(a[1]), np.asarray(b[1]))
            if i >= args.warmup:
                one.append(t1)
                many.append(t2)
        report(call, one, many, same)
    one, many, same, removed = [], [], True, None
    for i in range(args.warmup + args.repeats):
        if i:
            build_both()
        (t1, a), (t2, b) = timed(lambda: single.remove_non_amr_nodes(flags)), timed(
            lambda: dist.dist_remove_non_amr_nodes_loopback(ranks, flags))
        same, removed = same and a == b, a
        if i >= args.warmup:
            one.append(t1)
            many.append(t2)
    report("remove_non_amr_nodes", one, many, same, nodes_removed=removed)
    for e in ranks + [single]:
        e.close()


if __name__ == "__main__":
    main()
