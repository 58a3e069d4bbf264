#!/usr/bin/env python
"""Times the two read selections of main() between its passes, each with the build of the selected reads that
follows it, through the drop-in on the cfg-3 workload of bench.py (1 M reads x 60 genes, 20 000-gene vocabulary, 2 %
wrong genes, k = 5) after build_filtered_graph(reads, 5, positions, 3, 1) from array-backed inputs:

    junk    remove_junk_reads(0.8), then GeneMerGraph(kept reads, 5, kept positions)
    valid   get_valid_reads_only(), then GeneMerGraph(valid reads, 5)

One process measures one tree: --root names the checkout whose amira_amd is imported (default: this one), so that the
same file times a parent checkout built beside it; run the two alternately from one shell loop.  Each timed window
starts with the filtered graph built and the stream idle and ends with the next graph built (host clock; the
selection's own part is reported as well).  Where the tree selects on the device, the kernels' own stage times
(amg_last_timings: select_classify, select_pack) come with the bytes they must move — 4 B per window read, 4 B read +
4 B written per gene of the set — and, for comparison, the correct_pack stage of an amg_correct_reads on the same
graph.

    python tools/probes/select_reads_time.py [--root DIR] [--reads N] [--calls junk,valid] [--repeats 5] [--warmup 1] [--warmup-valid N] [--out FILE]

Prints one JSON line per call (and appends it to --out).  Not a test and not the benchmark."""
import argparse
import json
import os
import statistics
import sys
import time

CFG3 = dict(L=60, V=20_000, k=5, err=0.02, seed=20250905 + 3)   # bench.py WORKLOADS["cfg3"]


def main():
    here = os.path.dirname(os.path.abspath(__file__))
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(here)))
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--calls", default="junk,valid")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--warmup-valid", type=int, help="warm-up runs of `valid` alone (a tree whose get_valid_reads_only "
                    "spends tens of seconds per run in the interpreter gains nothing from one)")
    ap.add_argument("--out")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import numpy as np
    from amira_amd import GeneMerGraph, graph_utils as gu, synth
    from amira_amd.engine import Engine
    from amira_amd.io import TokenizedPositions, TokenizedReads
    from amira_amd.tokens import Vocabulary

    w, N = CFG3, args.reads
    ids, sts = synth.block_reads(w["seed"], 0, N, w["L"], w["V"], w["err"], n_amr=0)     # as bench.make_tokens
    names = synth.gene_names(w["V"], 0)
    vocab = Vocabulary(names)
    rank = np.array([vocab.rank[n] for n in names], dtype=np.int64)[ids]
    toks = np.where(sts == 1, vocab.V + rank, vocab.V - 1 - rank).astype(np.int32).reshape(-1)
    offs = np.arange(N + 1, dtype=np.int64) * w["L"]
    read_ids = synth.read_names(0, N)
    gs = np.tile(np.arange(w["L"], dtype=np.int64) * 1000, N)     # synth.positions_for
    ge = gs + 899
    on_device = hasattr(Engine, "select_reads")   # this tree selects on the device

    def filtered_graph():
        g = gu.build_filtered_graph(TokenizedReads(vocab, toks, offs, read_ids), w["k"],
                                    TokenizedPositions(read_ids, offs, gs, ge), 3, 1)
        g._engine.sync()
        return g

    def report(call, times, select_times, **more):
        ms, sel = sorted(1e3 * t for t in times), sorted(1e3 * t for t in select_times)
        line = {"call": call, "root": os.path.abspath(args.root), "reads": N, "on_device": on_device, "repeats": len(ms),
                "median_ms": round(statistics.median(ms), 3), "min_ms": round(ms[0], 3), "max_ms": round(ms[-1], 3),
                "selection_median_ms": round(statistics.median(sel), 3), "selection_min_ms": round(sel[0], 3),
                "selection_max_ms": round(sel[-1], 3), **more}
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            with open(args.out, "a") as fh:
                fh.write(text + "\n")

    def stages(engine, prefix):
        return [[name, round(ms, 4)] for name, ms in engine.timings() if name.startswith(prefix)]   # (in stage order)

    for call in args.calls.split(","):
        times, select_times, more = [], [], {}
        warmup = args.warmup_valid if call == "valid" and args.warmup_valid is not None else args.warmup
        for i in range(warmup + args.repeats):
            g = filtered_graph()
            t0 = time.perf_counter()
            if call == "junk":
                kept, kept_pos, rejected, _ = g.remove_junk_reads(0.8)
                t1 = time.perf_counter()
                g2 = GeneMerGraph(kept, w["k"], kept_pos)
            else:
                kept, rejected = g.get_valid_reads_only(), ()
                t1 = time.perf_counter()
                g2 = GeneMerGraph(kept, w["k"])
            g2._engine.sync()
            t2 = time.perf_counter()
            if i >= warmup:
                times.append(t2 - t0)
                select_times.append(t1 - t0)
            more = {"kept_reads": len(kept), "rejected_reads": len(rejected),
                    "next_graph_nodes": g2.get_total_number_of_nodes()}
            if on_device and i == warmup + args.repeats - 1:
                # the kernels' own times on this graph, beside the bytes they must move
                g._settle_leases()   # (the kept reads leave the engine before its corrected set is overwritten)
                eng = g._engine
                k = w["k"]
                mode = 1 if call == "junk" else 0
                table = [round(x * (1 - 0.8)) for x in range(w["L"] - k + 2)] if call == "junk" else None
                _, n_r, n_t = eng.select_reads(mode, False, table, want_verdict=False)
                more["select_stages_ms"] = stages(eng, "select_")
                more["classify_bytes"] = 4 * N * (w["L"] - k + 1)
                more["pack_bytes"] = 8 * n_t
                eng.set_read_lengths(np.full(N, w["L"] * 1000 + 100, np.int64))   # synth.fake_fastq_lengths
                eng.correct_reads()
                more["parent_correct_pack_ms_same_graph"] = stages(eng, "correct_pack")
            g2.close()
            g.close()
            del kept, rejected, g2, g
        report(call, times, select_times, **more)


if __name__ == "__main__":
    main()
