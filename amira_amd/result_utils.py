"""`write_pandora_gene_calls` under the reference's own name and signature (result_utils.py:1260-1264): the corrected
gene calls and their positions out as the two JSON files the reference dumps — byte for byte what `json.dumps` writes
for the same mappings (tests/test_calls_cpu.py).  Array-backed mappings (amira_amd.io.TokenizedReads /
TokenizedPositions, what GeneMerGraph.correct_reads and the drivers hand back) are written natively from their arrays,
the two files side by side; plain dicts take the reference's own two lines.

Copy numbers (`estimate_copy_numbers` :1089-1159 and what it calls, :975-1086) under the reference's names too: the
reference counts 15-mers by running the external tool jellyfish four times; here the counts live in a table on the
device (amira_amd.engine.KmerCounts, amg_kcount.hip) and the two fits run on its histograms with the reference's scipy
calls in the reference's order.  INTEGRATION.md lists where the two differ in what they write.

Everything else of the reference's result_utils.py (racon / minimap2 / samtools post-processing, TSV output) is
outside the hot path.
"""
import json
import os
import statistics
import sys
import threading

import numpy as np

from .io import TokenizedPositions, TokenizedReads, write_gene_calls, write_gene_positions


def write_pandora_gene_calls(output_dir, gene_position_dict, annotatedReads, outfile_1, outfile_2):
    """result_utils.py:1260-1264: json.dumps(annotatedReads) -> outfile_1, json.dumps(gene_position_dict) -> outfile_2
    (output_dir is not used there either)."""
    jobs = []
    # (reads bubble popping rewrote and positions a correction redirected are spelled into the arrays first: .settled())
    if isinstance(annotatedReads, TokenizedReads):
        r = annotatedReads.settled()
        jobs.append(lambda: write_gene_calls(outfile_1, r.vocab, r.tokens, r.read_offsets, r.read_ids))
    else:
        jobs.append(lambda: _dump(outfile_1, annotatedReads))
    if isinstance(gene_position_dict, TokenizedPositions):
        p = gene_position_dict.settled()
        jobs.append(lambda: write_gene_positions(outfile_2, p.gene_start, p.gene_end, p.read_offsets, p.read_ids))
    else:
        jobs.append(lambda: _dump(outfile_2, gene_position_dict))
    # the two files are independent: their writers run side by side (the native writers release the interpreter lock
    # and use the host's cores; each alone leaves most of a large box idle)
    errs = []

    def run(job):
        try:
            job()
        except BaseException as e:  # noqa: BLE001 - re-raised below, in the caller's thread
            errs.append(e)

    t = threading.Thread(target=run, args=(jobs[1],))
    t.start()
    run(jobs[0])
    t.join()
    if errs:
        raise errs[0]


def _dump(path, mapping):
    if isinstance(mapping, (TokenizedReads, TokenizedPositions)):
        mapping = {k: _listed(mapping[k]) for k in mapping}
    with open(path, "w") as o:
        o.write(json.dumps(mapping))


def _listed(v):
    return [list(x) if isinstance(x, tuple) else x for x in v]


# ------------------------------------------------------------------ copy numbers from k-mer counts
def import_jellyfish_histo(histo_path):
    """result_utils.py:1025-1034: a `value count` line per non-empty bin -> {value: count}"""
    bins = {}
    with open(histo_path) as fh:
        for line in fh.read().split("\n"):
            if line:
                fields = line.split(" ")
                bins[int(fields[0])] = int(fields[1])
    return bins


def write_jellyfish_histo(histo_path, bins):
    """the file import_jellyfish_histo reads: the non-empty bins in ascending order"""
    with open(histo_path, "w") as fh:
        fh.write("".join(f"{v} {bins[v]}\n" for v in sorted(bins)))


def load_kmer_counts(counts_file):
    """result_utils.py:1037-1047: the non-zero counts of a `kmer count` file (what `jellyfish query` prints)"""
    counts = []
    with open(counts_file) as fh:
        for line in fh:
            fields = line.split()
            if len(fields) == 2 and int(fields[1]) != 0:
                counts.append(int(fields[1]))
    return counts


def estimate_depth(counts_file):
    """result_utils.py:1083-1086"""
    return statistics.median(load_kmer_counts(counts_file))


def kmer_cutoff_estimation(kmer_counts):
    """result_utils.py:975-1004: a mixture of Poisson(1) (errors, weight w) and Poisson(c) (the genome) fitted to the
    histogram by BFGS from (0.1, 10); the cutoff is the first count at which the genome's share is the larger one"""
    from scipy.optimize import minimize
    from scipy.stats import poisson
    values = np.array(list(kmer_counts.keys()))
    keys_at = np.array(list(kmer_counts.values()))

    def cost(params):
        w, c = params
        if w < 0 or w > 1 or c <= 0:
            return np.inf
        errors = poisson.pmf(values, mu=1)
        genome = poisson.pmf(values, mu=c)
        both = w * errors + (1 - w) * genome
        both[both == 0] = 1e-10
        return -np.sum(keys_at * np.log(both))

    w, c = minimize(cost, [0.1, 10], method="BFGS").x
    for v in values:
        if poisson.pmf(v, mu=c) * (1 - w) > poisson.pmf(v, mu=1) * w:
            return v
    return 0


def estimate_kmer_depth(kmer_counts, histogram_path, debug=False):
    """result_utils.py:1007-1022: the count at the highest peak of the smoothed log histogram"""
    from scipy.signal import find_peaks, savgol_filter
    values, keys_at = zip(*sorted(kmer_counts.items()))
    logs = np.log(np.array(keys_at) + 1)
    smooth = savgol_filter(logs, min(30, len(logs) // 2 * 2 + 1), 3)
    peaks, _ = find_peaks(smooth)
    depth = values[peaks[np.argmax(smooth[peaks])]]
    if debug is True:
        import matplotlib.pyplot as plt
        plt.bar(values, logs)
        plt.plot(values, smooth, color="red", label="Smoothed counts")
        plt.axvline(depth, color="red")
        plt.xlim(0, 500)
        plt.savefig(histogram_path.replace(".filtered.histo", ".png"), dpi=600)
    return depth


def _fastq_sequences(path):
    """{read id: {"sequence": ...}} of a FASTQ file, gzipped or not"""
    import gzip
    opener = gzip.open if path.endswith(".gz") else open
    reads = {}
    with opener(path, "rt") as fh:
        while True:
            head = fh.readline()
            if not head:
                break
            reads[head[1:].split()[0]] = {"sequence": fh.readline().rstrip("\n")}
            fh.readline()
            fh.readline()
    return reads


def estimate_overall_read_depth(full_reads, k, threads, debug, outdir, fastq_content=None, device=0):
    """result_utils.py:1050-1080 without jellyfish: the k-mers of fastq_content's sequences (None: of the file
    full_reads) are counted on the device; <base>.histo and <base>.filtered.histo are written as the reference writes
    them.  Returns the depth and, where the reference returns the path of the filtered .jf file, the KmerCounts
    handle: .min_count is the cutoff its readers apply, .row_of the table row of every read with a sequence.  The
    caller closes it (close_kmer_counts)."""
    from .engine import KmerCounts, Sequences, acquire_engine, release_engine
    if fastq_content is None:
        fastq_content = _fastq_sequences(full_reads)
    base = os.path.basename(os.path.splitext(os.path.splitext(os.path.basename(full_reads))[0])[0])
    sys.stderr.write("\nAmira: counting k-mers on the device.\n")
    row_of, sequences = {}, []
    for read in fastq_content:
        seq = fastq_content[read]["sequence"]
        if seq != "":
            row_of[read] = len(sequences)
            sequences.append(seq)
    engine = acquire_engine(device)
    resident = counts = None
    try:
        resident = Sequences(sequences, device)
        counts = KmerCounts(engine, resident, k)
        histo = counts.histo()
        write_jellyfish_histo(os.path.join(outdir, base) + ".histo", histo)
        cutoff = kmer_cutoff_estimation(import_jellyfish_histo(os.path.join(outdir, base) + ".histo"))
        sys.stderr.write(f"\nAmira: filtering k-mers with count below cutoff ({cutoff}).\n")
        filtered_path = os.path.join(outdir, base) + ".filtered.histo"
        write_jellyfish_histo(filtered_path, counts.histo(int(cutoff)))
        depth = estimate_kmer_depth(import_jellyfish_histo(filtered_path), filtered_path, debug)
    except BaseException:
        if counts is not None:
            counts.close()
        if resident is not None:
            resident.close()
        release_engine(engine)
        raise
    counts.min_count, counts.row_of = int(cutoff), row_of
    return depth, counts


def close_kmer_counts(counts):
    """gives back what estimate_overall_read_depth's handle holds: the table, the resident sequences, the engine"""
    from .engine import release_engine
    counts.close()
    counts.sequences.close()
    release_engine(counts.engine)


def estimate_copy_numbers(fastq_content, path_reads, amira_alleles, fastq_file, output_dir, threads, samtools_path,
                          raw_read_depth, debug):
    """result_utils.py:1089-1159.  Per path of path_reads the depth is the median of the non-zero counts (after the
    cutoff) of all 15-mer occurrences of the path's reads, taken on the device; every allele of amira_alleles on the
    path gets depth / overall depth, and that divided by the number of its gene's alleles on the path.
    path_id_mapping.json is written; the per-path FASTQ and count files are not (nothing reads them).  threads,
    samtools_path and raw_read_depth are unused, as in the reference."""
    outdir = os.path.join(output_dir, "AMR_allele_fastqs", "path_reads")
    os.makedirs(outdir, exist_ok=True)
    paths = list(path_reads.keys())
    path_mapping = {i + 1: list(path) for i, path in enumerate(paths)}
    with open(os.path.join(outdir, "path_id_mapping.json"), "w") as o:
        o.write(json.dumps(path_mapping))
    read_depth, counts = estimate_overall_read_depth(fastq_file, 15, threads, debug, output_dir,
                                                     fastq_content=fastq_content)
    try:
        sys.stderr.write(f"\nAmira: estimated k-mer depth = {read_depth}.\n")
        # (a read listed twice is one read of the path's set, and a read without a sequence none)
        sets = [[counts.row_of[r] for r in dict.fromkeys(path_reads[path]) if fastq_content[r]["sequence"] != ""]
                for path in paths]
        n, lo, hi = counts.medians(sets, counts.min_count)
    finally:
        close_kmer_counts(counts)
    normalised_depths, mean_depth_per_reference = {}, {}
    for i, path_id in enumerate(path_mapping):
        genes = path_mapping[path_id]
        alleles_of = {}
        for g in genes:
            if g[1:] in amira_alleles:
                gene = "_".join(g[1:].split("_")[:-1])
                alleles_of[gene] = alleles_of.get(gene, 0) + 1
        if n[i] == 0:
            raise statistics.StatisticsError("no median for empty data")
        # statistics.median: the middle element of an odd number of counts, the mean of the two middle ones otherwise
        depth = int(lo[i]) if n[i] % 2 else (int(lo[i]) + int(hi[i])) / 2
        for g in genes:
            allele = g[1:]
            if allele not in amira_alleles:
                continue
            gene = "_".join(allele.split("_")[:-1])
            normalised_depths[allele] = depth / (read_depth * alleles_of[gene])
            mean_depth_per_reference[allele] = depth / read_depth
    return normalised_depths, mean_depth_per_reference
