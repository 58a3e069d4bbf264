"""The device k-mer counts (amg_kcount.hip through amira_amd.engine.KmerCounts) against the numpy oracle
(tests/kcount_oracle.py), and estimate_copy_numbers on top of them against a plain restatement that reads the
oracle's counts."""
import functools
import json
import os
import statistics

import numpy as np
import pytest

import kcount_oracle as O
import procedures as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from amira_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def counted(eng, seqs, k, slots_log2=0):
    """(KmerCounts, Sequences) of seqs"""
    from amira_amd.engine import KmerCounts, Sequences
    resident = Sequences(seqs, 0)
    try:
        return KmerCounts(eng, resident, k, slots_log2), resident
    except BaseException:
        resident.close()
        raise


def close(kc, resident):
    kc.close()
    resident.close()


def check_against_oracle(kc, seqs, k, table=None):
    """query on every sequence == the oracle's lookup; sizes() == the oracle's totals"""
    table = table or O.Table(seqs, k)
    got = kc.query(seqs)
    assert len(got) == len(seqs)
    total = 0
    for s, g in zip(seqs, got):
        want = table.lookup(s)
        assert np.array_equal(g == -1, want == -1), s[:60]
        assert np.array_equal(g, want), s[:60]
        total += int(g[g > 0].sum())
    sizes = kc.sizes()
    assert (sizes["k"], sizes["windows"], sizes["distinct"]) == (k, table.windows, table.distinct)
    assert sizes["slots"] & (sizes["slots"] - 1) == 0 and sizes["slots"] >= table.distinct
    assert total > 0
    return table


@functools.lru_cache(maxsize=None)
def random_rows():
    return tuple(O.random_sequences(np.random.default_rng(2024), 200, 0, 3000))


def acgt(rng, n):
    return "".join("ACGT"[x] for x in rng.integers(0, 4, n))


@functools.lru_cache(maxsize=None)
def hot_rows():
    rng = np.random.default_rng(77)
    return tuple(["A" * 20000, "T" * 20000] + O.random_sequences(rng, 50, 0, 3000))


@functools.lru_cache(maxsize=None)
def hot_table():
    return O.Table(hot_rows(), 15)


@pytest.mark.parametrize("k", [1, 3, 4, 15, 16, 17, 31])   # (16 and 31: 32 and 62 bits of the two-bit pack)
def test_counts_equal_the_oracle(eng, k):
    rng = np.random.default_rng(k)
    seqs = list(random_rows()) + ["", "ACG", "N" * 50]
    seqs += [acgt(rng, n) for n in (1023, 1024, 1025, 1024 + k - 1)]   # the tile seams
    # two neighbours whose concatenation holds windows that neither holds
    seqs += ["ACGGTC" * 6 + "GATTACA", "TTGACA" * 6 + "CCATG"]
    kc, resident = counted(eng, seqs, k)
    try:
        check_against_oracle(kc, seqs, k)
    finally:
        close(kc, resident)


def test_both_strands_are_one_key_and_palindromes_count_once(eng):
    rng = np.random.default_rng(5)
    s = acgt(rng, 2500)
    one, r1 = counted(eng, [s], 15)
    two, r2 = counted(eng, [s, O.revcomp(s)], 15)
    try:
        a, b = one.query([s])[0], two.query([s])[0]
        assert (a > 0).sum() == len(s) - 14
        assert np.array_equal(np.where(a > 0, 2 * a, a), b)
        assert np.array_equal(two.query([O.revcomp(s)])[0][: len(s) - 14], b[: len(s) - 14][::-1])
    finally:
        close(one, r1)
        close(two, r2)
    rep = "ACGT" * 300
    kc, resident = counted(eng, [rep], 4)
    try:
        got = kc.query(["ACGT"])[0]
        assert got[0] == 300 and list(got[1:]) == [-1, -1, -1]   # not 600: the k-mer is its own reverse complement
        check_against_oracle(kc, [rep], 4)
    finally:
        close(kc, resident)


@pytest.mark.parametrize("fold", ["1", "0"])
def test_hot_key(eng, monkeypatch, fold):
    """tens of thousands of equal neighbouring windows, with the in-wave fold and with one add per window"""
    monkeypatch.setenv("AMG_KCOUNT_FOLD", fold)
    seqs = list(hot_rows())
    kc, resident = counted(eng, seqs, 15)
    try:
        assert kc.query(["A" * 15])[0][0] == 2 * (20000 - 14)
        assert kc.query(["t" * 15])[0][0] == 2 * (20000 - 14)
        check_against_oracle(kc, seqs, 15, hot_table())
        assert kc.histo()[10001] == 1
    finally:
        close(kc, resident)


def all_3mers():
    return ["".join((a, b, c)) for a in "ACGT" for b in "ACGT" for c in "ACGT"]


def test_exact_fill_and_overflow(eng):
    from amira_amd._ffi import AmgError, E_NOMEM
    rows = ["N".join(all_3mers()), acgt(np.random.default_rng(3), 500)]   # all 32 canonical 3-mers, none a palindrome
    assert O.Table(rows, 3).distinct == 32
    kc, resident = counted(eng, rows, 3, slots_log2=5)
    try:
        assert kc.sizes()["slots"] == 32
        check_against_oracle(kc, rows, 3)
        assert list(kc.query(["N" * 100])[0]) == [-1] * 100
    finally:
        close(kc, resident)
    # a full table and windows whose keys are not in it: the lookup ends after one round
    half = sorted({min(w, O.revcomp(w)) for w in all_3mers()})[:16]
    absent = sorted({min(w, O.revcomp(w)) for w in all_3mers()})[16:]
    kc, resident = counted(eng, half, 3, slots_log2=4)
    try:
        assert kc.sizes()["distinct"] == kc.sizes()["slots"] == 16
        assert [int(g[0]) for g in kc.query(half)] == [1] * 16
        assert [int(g[0]) for g in kc.query(absent)] == [0] * 16
        assert [int(g[0]) for g in kc.query([O.revcomp(w) for w in absent])] == [0] * 16
    finally:
        close(kc, resident)
    # 32 keys do not fit 16 slots: an error, not a spin, and the engine is as good as before
    with pytest.raises(AmgError) as ei:
        counted(eng, rows, 3, slots_log2=4)
    assert ei.value.code == E_NOMEM and "table full" in str(ei.value)
    kc, resident = counted(eng, rows, 3)
    try:
        assert kc.sizes()["slots"] == 64
        check_against_oracle(kc, rows, 3)
    finally:
        close(kc, resident)
    kc, resident = counted(eng, ["ACGTTGCANNAC", "ca"], 1, slots_log2=1)
    try:
        assert kc.sizes()["slots"] == 2 and kc.sizes()["distinct"] == 2
        check_against_oracle(kc, ["ACGTTGCANNAC", "ca"], 1)
    finally:
        close(kc, resident)


@pytest.mark.parametrize("case", ["hot", "random"])
def test_histogram_equals_the_oracle(eng, case):
    seqs = list(hot_rows()) if case == "hot" else list(random_rows())
    table = hot_table() if case == "hot" else O.Table(seqs, 15)
    kc, resident = counted(eng, seqs, 15)
    try:
        for m in (0, 1, 2, 5, 10002):
            assert kc.histo(m) == table.histo(m), m
        assert sum(kc.histo(0).values()) == kc.sizes()["distinct"] == table.distinct
        if case == "hot":
            assert kc.histo(10002) == {10001: 1}
    finally:
        close(kc, resident)


def want_medians(table, seqs, sets, m):
    n, lo, hi = [], [], []
    for rows in sets:
        a = table.set_counts([seqs[r] for r in rows], m)
        n.append(len(a))
        lo.append(int(a[(len(a) - 1) // 2]) if len(a) else 0)
        hi.append(int(a[len(a) // 2]) if len(a) else 0)
    return n, lo, hi


def test_medians_of_small_sets(eng):
    # k = 3: AAA (rows 0 and 5) 4 times, ACG (rows 1 and 6) 3 times, everything else once
    seqs = ["AAAAA", "ACG", "NNNN", "", "CCCA", "TTT", "ACGACG"]
    sets = [[0], [0, 1], [1, 5], [], [2, 3], [0, 6], [4, 6, 1]]
    table = O.Table(seqs, 3)
    kc, resident = counted(eng, seqs, 3)
    try:
        for m in (0, 2):
            n, lo, hi = kc.medians(sets, m)
            assert (n.tolist(), lo.tolist(), hi.tolist()) == want_medians(table, seqs, sets, m), m
        n, lo, hi = kc.medians(sets)
        assert n.tolist() == [3, 4, 2, 0, 0, 7, 7]          # odd, even, empty, only N, row 0 in three sets
        assert (lo[2], hi[2]) == (3, 4)                      # the two middle counts differ: a median of 3.5
        assert kc.medians([])[0].tolist() == []
    finally:
        close(kc, resident)


@functools.lru_cache(maxsize=None)
def median_case():
    rng = np.random.default_rng(9)
    seqs = O.random_sequences(rng, 40, 200, 3000) + ["N" * 300, ""]
    sets = [list(range(0, 7)), [3, 8, 9, 10], [3], [], [40, 41], list(range(3, 40)), [11, 12, 12, 13]]
    return seqs, sets, O.Table(seqs, 7)


def test_medians_of_read_sets(eng):
    seqs, sets, table = median_case()
    kc, resident = counted(eng, seqs, 7)
    try:
        for m in (0, 7):
            want = want_medians(table, seqs, sets, m)
            n, lo, hi = kc.medians(sets, m)
            assert (n.tolist(), lo.tolist(), hi.tolist()) == want, m
        # 7 removes a part of every set that holds anything
        all_n, some_n = want_medians(table, seqs, sets, 0)[0], want_medians(table, seqs, sets, 7)[0]
        assert all(0 < b < a for a, b in zip(all_n, some_n) if a) and sum(all_n) > 0
        assert {a % 2 for a in all_n if a} == {0, 1} or {a % 2 for a in some_n if a} == {0, 1}
    finally:
        close(kc, resident)


# ------------------------------------------------------------------ sequence boundaries against the tiles of base_tile
TILE = 1024    # BT_TILE (amg_bases.h): window starts per workgroup


def _cut(text, cuts):
    cuts = [0] + sorted(set(cuts)) + [len(text)]
    return [text[a:b] for a, b in zip(cuts, cuts[1:])]


@pytest.mark.parametrize("k", [1, 8, 9, 16, 17, 31])   # (either side of every step of the words per k-mer)
def test_query_across_tile_seams(eng, k):
    """host segments, nothing gathered: the cuts of test_gpu_minhash.py's
    test_segment_boundaries_on_the_edges_of_a_tile.  The table holds the UNCUT text, so a window that ran over a cut
    would be found in it"""
    text = acgt(np.random.default_rng(1100 + k), 3 * TILE + 77)
    pieces = _cut(text, [1023, 1024, 1025, 2 * TILE - k, 2 * TILE - k + 1, 2 * TILE, 3 * TILE - 1])
    assert np.cumsum([len(s) for s in pieces])[:-1].tolist() == sorted({1023, 1024, 1025, 2048 - k, 2049 - k, 2048, 3071})
    table = O.Table([text], k)
    kc, resident = counted(eng, [text], k)
    try:
        got = kc.query(pieces)
        for piece, g in zip(pieces, got):
            want = table.lookup(piece)
            assert np.array_equal(g == -1, want == -1), (k, len(piece))
            assert np.array_equal(g, want), (k, len(piece))
        whole = kc.query([text])[0]
        assert np.array_equal(whole, table.lookup(text))
        windows, uncut = sum(int((g != -1).sum()) for g in got), int((whole != -1).sum())
        assert uncut == len(text) - k + 1 and (windows < uncut if k > 1 else windows == uncut)
    finally:
        close(kc, resident)


@functools.lru_cache(maxsize=None)
def gather_case():
    """rows cut out of one text so that the rows listed side by side in a set are neighbours in the text too, and
    another row covers the place where they meet: a window that ran from one row into the next would be counted"""
    lengths = [1023, 1, 0, 1024, 1025, 700, 0, 0, 324 + 1024, 5]
    starts = [1025, 1947, 0, 2048, 0, 1700, 0, 0, 600, 2046]
    text = acgt(np.random.default_rng(1200), 3 * TILE + 77)
    rows = [text[a: a + n] for a, n in zip(starts, lengths)]
    sets = [[4, 0, 3], [8, 8, 1], [2, 6, 7], [9, 5, 4, 3, 0]]
    return text, rows, sets


@pytest.mark.parametrize("k", [3, 15])
def test_medians_through_the_gather_across_tile_seams(eng, k):
    text, rows, sets = gather_case()
    # the stream the kernel walks: the listed rows of all sets end to end
    ends = np.cumsum([len(rows[r]) for rows_of in sets for r in rows_of]).tolist()
    assert {1023, 1024, 1025} & set(ends) and any(e > 0 and e % TILE == 0 for e in ends)   # (a row's last base = a tile's)
    assert ends.count(ends[5]) > 1                                                          # empty rows in the stream
    table = O.Table(rows, k)
    # rows 4 | 0 | 3 of the first set meet at 1025 and 2048 of the text: the windows across are in the table (rows 8, 5)
    assert (table.lookup(text[1025 - k + 1: 1025 + k - 1])[: k - 1] > 0).all()
    assert (table.lookup(text[2048 - k + 1: 2048 + k - 1])[: k - 1] > 0).all()
    kc, resident = counted(eng, rows, k)
    try:
        for m in (0, 2):
            want = want_medians(table, rows, sets, m)
            n, lo, hi = kc.medians(sets, m)
            assert (n.tolist(), lo.tolist(), hi.tolist()) == want, (k, m)
        assert want_medians(table, rows, sets, 0)[0][2] == 0 and min(want_medians(table, rows, sets, 0)[0][:2]) > 2000
    finally:
        close(kc, resident)


@pytest.mark.parametrize("k", [2, 3])
def test_hundreds_of_tiny_rows_in_one_tile_before_a_long_one(eng, k):
    """test_gpu_minhash.py's case of the same name through the other two entries: every thread's search goes over
    hundreds of offsets"""
    rng = np.random.default_rng(1300 + k)
    rows = [acgt(rng, n) for n in rng.choice(4, 700, p=[0.3, 0.3, 0.2, 0.2])]
    assert sum(len(s) for s in rows) < TILE and {len(s) for s in rows} == {0, 1, 2, 3}
    rows.append(acgt(rng, 1500))
    kc, resident = counted(eng, rows, k)
    try:
        table = check_against_oracle(kc, rows, k)
        sets = [list(range(len(rows)))]
        want = want_medians(table, rows, sets, 0)
        n, lo, hi = kc.medians(sets)
        assert (n.tolist(), lo.tolist(), hi.tolist()) == want and want[0][0] == table.windows > 1500 - k
    finally:
        close(kc, resident)


def test_a_call_refused_for_its_size_is_halved(eng):
    from amira_amd._ffi import AmgError, E_NOMEM
    from amira_amd.engine import KmerCounts
    seqs, sets, table = median_case()
    calls = []

    class Watched(KmerCounts):
        def _medians(self, sets_, a, b, *rest):
            calls.append((a, b))
            return super()._medians(sets_, a, b, *rest)

    kc, resident = counted(eng, seqs, 7)
    kc.__class__ = Watched
    try:
        whole = [x.tolist() for x in kc.medians(sets)]
        assert calls == [(0, len(sets))]
        del calls[:]
        largest = max(whole[0])
        assert sum(whole[0]) > largest   # the unsplit call is over the limit, every single set within it
        split = [x.tolist() for x in kc.medians(sets, max_pairs=largest)]
        assert split == whole == [list(x) for x in want_medians(table, seqs, sets, 0)]
        assert len(calls) > 1 and calls[0] == (0, len(sets))
        with pytest.raises(AmgError) as ei:   # one set cannot be split
            kc.medians([sets[5]], max_pairs=largest - 1)
        assert ei.value.code == E_NOMEM and "split the sets" in str(ei.value)
    finally:
        close(kc, resident)


def test_real_reads(eng, tmp_path):
    from amira_amd import result_utils as R
    fq = P.real_fastq()
    seqs = [v["sequence"] for v in fq.values()]
    table = O.Table(seqs, 15)
    kc, resident = counted(eng, seqs, 15)
    try:
        assert kc.histo() == table.histo()
        assert kc.sizes()["windows"] == table.windows
    finally:
        close(kc, resident)
    depth, counts = R.estimate_overall_read_depth("/somewhere/test_1.fastq.gz", 15, 1, False, str(tmp_path),
                                                  fastq_content=fq)
    try:
        cutoff = int(R.kmer_cutoff_estimation(table.histo()))
        assert counts.min_count == cutoff > 1
        assert depth == R.estimate_kmer_depth(table.histo(cutoff), "unused", False)
        assert R.import_jellyfish_histo(str(tmp_path / "test_1.histo")) == table.histo()
        assert R.import_jellyfish_histo(str(tmp_path / "test_1.filtered.histo")) == table.histo(cutoff)
    finally:
        R.close_kmer_counts(counts)


def restated_copy_numbers(fastq_content, path_reads, amira_alleles):
    """estimate_copy_numbers with the oracle's counts in jellyfish's place"""
    from amira_amd import result_utils as R
    table = O.Table([v["sequence"] for v in fastq_content.values()], 15)
    cutoff = int(R.kmer_cutoff_estimation(table.histo()))
    read_depth = R.estimate_kmer_depth(table.histo(cutoff), "unused", False)
    normalised, mean = {}, {}
    for path, reads in path_reads.items():
        subset = {r: fastq_content[r] for r in reads if fastq_content[r]["sequence"] != ""}
        depth = statistics.median(table.set_counts([v["sequence"] for v in subset.values()], cutoff).tolist())
        copies = {}
        for g in path:
            if g[1:] in amira_alleles:
                gene = "_".join(g[1:].split("_")[:-1])
                copies[gene] = copies.get(gene, 0) + 1
        for g in path:
            if g[1:] in amira_alleles:
                gene = "_".join(g[1:].split("_")[:-1])
                normalised[g[1:]] = depth / (read_depth * copies[gene])
                mean[g[1:]] = depth / read_depth
    return normalised, mean


def test_estimate_copy_numbers_end_to_end(tmp_path):
    from amira_amd import result_utils as R
    fq = O.synthetic_reads()
    fq["no_sequence"] = {"sequence": ""}
    names = list(fq)
    path_reads = {
        ("+geneA", "-blaX_1", "+geneB"): names[0:60],
        ("+blaX_1", "+geneC", "+blaX_2", "-blaY_1"): names[40:121] + ["no_sequence"],   # two alleles of blaX
        ("-geneD", "+blaZ_7"): names[100:103] + names[100:102],
        ("+blaW_1",): names[1:240:2],
    }
    alleles = {"blaX_1": 0, "blaX_2": 0, "blaY_1": 0, "blaZ_7": 0, "blaW_1": 0, "blaV_1": 0}
    os.makedirs(tmp_path / "AMR_allele_fastqs")
    got = R.estimate_copy_numbers(fq, path_reads, alleles, str(tmp_path / "reads.fastq.gz"), str(tmp_path), 1, None,
                                  None, False)
    want = restated_copy_numbers(fq, path_reads, alleles)
    assert got == want
    assert set(got[0]) == {"blaX_1", "blaX_2", "blaY_1", "blaZ_7", "blaW_1"}
    assert got[0]["blaX_2"] * 2 == got[1]["blaX_2"] and got[0]["blaY_1"] == got[1]["blaY_1"]
    mapping = json.load(open(tmp_path / "AMR_allele_fastqs" / "path_reads" / "path_id_mapping.json"))
    assert mapping == {str(i + 1): list(p) for i, p in enumerate(path_reads)}
    table = O.Table([v["sequence"] for v in fq.values()], 15)
    assert R.import_jellyfish_histo(str(tmp_path / "reads.histo")) == table.histo()
    filtered = R.import_jellyfish_histo(str(tmp_path / "reads.filtered.histo"))
    assert filtered == table.histo(int(R.kmer_cutoff_estimation(table.histo())))
    # a path without a k-mer left ends where the reference's statistics.median ends
    with pytest.raises(statistics.StatisticsError):
        R.estimate_copy_numbers(fq, {("+blaX_1",): ["no_sequence"]}, alleles, str(tmp_path / "reads.fastq.gz"),
                                str(tmp_path), 1, None, None, False)
