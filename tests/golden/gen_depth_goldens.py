#!/usr/bin/env python3
"""Generate tests/golden/depth_goldens.json from the REAL reference (build container only).

    python tests/golden/gen_depth_goldens.py

Imports /root/reference/amira with the import-only shims gen_goldens.py uses and runs its kmer_cutoff_estimation,
estimate_kmer_depth and estimate_depth (result_utils.py:975-1022, :1083-1086) on histograms and count lists made here
by the host oracle of the k-mer counts (tests/kcount_oracle.py).  Only inputs and the returned numbers are written:
nothing of the reference travels, and no test reads /root/reference.  An input on which a reference function raises
gives no golden for that function (it is named on stderr).
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "shims"), "/root/reference", HERE, os.path.dirname(HERE)]

import kcount_oracle as O  # noqa: E402
import procedures as P  # noqa: E402

from amira.result_utils import estimate_depth, estimate_kmer_depth, kmer_cutoff_estimation  # noqa: E402  (the reference)


def hand_made():
    few = {v: c for v, c in zip(range(1, 14), (9000, 2100, 400, 90, 60, 140, 320, 510, 380, 150, 40, 8, 2))}
    two_peaks = {v: int(50000 * 0.35 ** v + 900 * 2.718281828 ** (-((v - 22) ** 2) / 30.0)
                        + 300 * 2.718281828 ** (-((v - 44) ** 2) / 60.0)) + 1 for v in range(1, 80)}
    gaps = {v: c for v, c in two_peaks.items() if v % 7 != 3}
    gaps[10001] = 5
    return {"few_bins": few, "two_peaks": two_peaks, "gaps_and_overflow_bin": gaps}


def main():
    histos = dict(hand_made())
    for name, reads in (("synthetic", O.synthetic_reads()), ("test_1", P.real_fastq())):
        table = O.Table([v["sequence"] for v in reads.values()], 15)
        histos[name] = table.histo()
        histos[name + "_filtered"] = table.histo(int(kmer_cutoff_estimation(histos[name])))
        if name == "synthetic":
            names = list(reads)
            lists = {"synthetic_first_40": table.set_counts([reads[r]["sequence"] for r in names[:40]], 9),
                     "synthetic_one_read": table.set_counts([reads[names[3]]["sequence"]], 0)}
    out = {"_meta": {"reference": "Danderson123/Amira v0.11.0", "python": sys.version.split()[0],
                     "scipy": __import__("scipy").__version__},
           "cutoff": [], "depth": [], "median": []}
    for name, h in histos.items():
        pairs = [[int(v), int(c)] for v, c in h.items()]   # (insertion order: kmer_cutoff_estimation walks the keys as given)
        for what, fn in (("cutoff", kmer_cutoff_estimation), ("depth", lambda x: estimate_kmer_depth(x, "unused", False))):
            try:
                out[what].append({"name": name, "histo": pairs, "result": int(fn(dict(h)))})
            except Exception as e:  # noqa: BLE001
                print(f"left out: {what} of {name}: {e!r}", file=sys.stderr)
    lists["even_with_half"] = [3, 4, 9, 10]
    lists["single"] = [7]
    for name, counts in lists.items():
        counts = [int(c) for c in counts]
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "q.kmer_counts.txt")
            with open(path, "w") as fh:
                fh.write("".join(f"ACGT {c}\n" for c in counts) + "ACGT 0\nshort\n")
            out["median"].append({"name": name, "counts": counts, "result": estimate_depth(path)})
    with open(os.path.join(HERE, "depth_goldens.json"), "w") as fh:
        json.dump(out, fh, separators=(",", ":"))
    print({k: [(e["name"], e["result"]) for e in out[k]] for k in ("cutoff", "depth", "median")}, file=sys.stderr)


if __name__ == "__main__":
    main()
