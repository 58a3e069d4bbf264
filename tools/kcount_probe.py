#!/usr/bin/env python3
"""What the device k-mer counts (amg_kcount.hip) cost on the benchmark's bubble-popping read set.

    python tools/kcount_probe.py [--reads 50000] [--k 15]

Builds the reads the `bubbles` leg of bench.py builds (bench._bubble_inputs: 50 000 reads, about 242 M bases), counts
their canonical k-mers and prints ONE JSON line: bases, windows, distinct keys, slots; milliseconds for the upload,
the count pass, the histogram and the medians of 200 read sets; windows per second; the count pass with and without
the in-wave fold of equal neighbouring keys, on this set and on a set with a hot key (two homopolymer rows); the
numpy oracle on a 1 % sample of the reads, extrapolated, as a CPU yardstick.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def count_pass(engine, resident, k, fold, reps=3):
    """best device time of the insert kernel over `reps` tables, and the last table's sizes"""
    from amira_amd.engine import KmerCounts
    os.environ["AMG_KCOUNT_FOLD"] = "1" if fold else "0"
    best, wall, sizes = None, None, None
    try:
        for _ in range(reps):
            t = time.perf_counter()
            kc = KmerCounts(engine, resident, k)
            dt = (time.perf_counter() - t) * 1e3
            ms = dict(engine.timings()).get("kcount_insert")
            sizes = kc.sizes()
            kc.close()
            if ms is not None and (best is None or ms < best):
                best, wall = ms, dt
    finally:
        del os.environ["AMG_KCOUNT_FOLD"]
    return best, wall, sizes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50000)
    ap.add_argument("--k", type=int, default=15)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    import bench
    import kcount_oracle as O
    from amira_amd import Engine
    from amira_amd.engine import KmerCounts, Sequences

    _, _, fq = bench._bubble_inputs(4242, args.reads, 60, 20000, 0.02)
    seqs = [v["sequence"] for v in fq.values()]
    out = {"probe": "kcount", "reads": len(seqs), "k": args.k, "bases": int(sum(len(s) for s in seqs))}
    engine = Engine(args.device)
    try:
        engine.set_timing(True)
        t = time.perf_counter()
        resident = Sequences(seqs, args.device)
        out["upload_ms"] = round((time.perf_counter() - t) * 1e3, 2)
        folded, wall, sizes = count_pass(engine, resident, args.k, True)
        plain, _, _ = count_pass(engine, resident, args.k, False)
        out.update(windows=sizes["windows"], distinct=sizes["distinct"], slots=sizes["slots"],
                   count_ms=round(folded, 3), count_ms_no_fold=round(plain, 3), count_call_ms=round(wall, 2),
                   windows_per_s=sizes["windows"] / (folded * 1e-3))
        # what the pass must move: a byte per base (a stream) and a 64-byte sector per probe, one probe per window
        # at the least (random access: this term bounds the pass, not the stream)
        out["count_min_bytes"] = out["bases"] + 64 * sizes["windows"]
        out["count_min_gbs"] = out["count_min_bytes"] / (folded * 1e-3) / 1e9
        out["hbm_peak_gbs"] = bench.HBM_PEAK_GBS
        kc = KmerCounts(engine, resident, args.k)
        try:
            for rep in range(2):
                t = time.perf_counter()
                histo = kc.histo()
                out["histo_call_ms"] = round((time.perf_counter() - t) * 1e3, 3)
                out["histo_ms"] = round(dict(engine.timings())["kcount_histo"], 3)
            out["histo_bins"] = len(histo)
            per_set = max(1, len(seqs) // 200)
            sets = [list(range(i * per_set, min(len(seqs), (i + 1) * per_set))) for i in range(200)]
            for rep in range(2):
                t = time.perf_counter()
                n, lo, hi = kc.medians(sets, 2)
                out["medians_200_sets_ms"] = round((time.perf_counter() - t) * 1e3, 2)
            out["medians_counts"] = int(n.sum())
        finally:
            kc.close()
        resident.close()
        # the repeat-rich case: two homopolymer rows among random ones
        rng = np.random.default_rng(77)
        hot = ["A" * 2_000_000, "T" * 2_000_000] + O.random_sequences(rng, 2000, 1000, 3000)
        resident = Sequences(hot, args.device)
        folded, _, sizes = count_pass(engine, resident, args.k, True)
        plain, _, _ = count_pass(engine, resident, args.k, False)
        out["hot_key"] = {"bases": int(sum(len(s) for s in hot)), "windows": sizes["windows"],
                          "count_ms": round(folded, 3), "count_ms_no_fold": round(plain, 3)}
        resident.close()
    finally:
        engine.close()
    sample = seqs[:: 100]
    t = time.perf_counter()
    table = O.Table(sample, args.k)
    dt = time.perf_counter() - t
    out["numpy_oracle_1pct"] = {"reads": len(sample), "windows": table.windows, "ms": round(dt * 1e3, 1),
                                "extrapolated_ms_all_reads": round(dt * 1e3 * len(seqs) / max(1, len(sample)), 1),
                                "note": "numpy on one core, a 1 % sample, scaled by reads: a yardstick, not a measurement "
                                        "of the whole set"}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
