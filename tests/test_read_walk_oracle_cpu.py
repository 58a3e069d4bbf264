"""tests/read_walk_oracle.py (the numpy restatement the GPU tests compare the read-walk kernels with) against the
pure-Python amira_oracle on small random read sets: pins the restatement to the reference's meaning without a GPU —
get_overall_mean_node_coverages (graph_utils.py:299-313), remove_non_AMR_associated_nodes (construct_graph.py:2941-2959)
and the per-component validity inside choose_kmer_size (graph_utils.py:258-296)."""
import numpy as np
import pytest

import read_walk_oracle as RW
from helpers import oracle_arrays


def random_reads(seed):
    """reads over two or three separate genomes (so that there are several components), some genes planted as genes of
    interest, with wrong genes here and there, reads of either strand and of 1 .. 14 genes (some shorter than k)"""
    rng = np.random.default_rng(seed)
    n_chrom = 2 + seed % 2
    chroms, nxt = [], 0
    for _ in range(n_chrom):
        n = int(rng.integers(12, 30))
        chroms.append([f"g{nxt + i}" for i in range(n)])
        nxt += n
    amr = [chroms[0][3], chroms[-1][5], "absent_gene"]   # the second chromosome of three holds none
    reads = {}
    for r in range(int(rng.integers(40, 80))):
        ch = chroms[int(rng.integers(n_chrom))]
        length = int(rng.integers(1, 15))
        start = int(rng.integers(len(ch)))
        genes = [ch[(start + i) % len(ch)] for i in range(length)]
        signs = ["+"] * length
        for i in range(length):
            if rng.random() < 0.04:
                genes[i] = f"g{int(rng.integers(nxt))}"
        if rng.random() < 0.5:
            genes, signs = genes[::-1], ["-"] * length
        reads[f"read{r}"] = [s + g for s, g in zip(signs, genes)]
    return reads, amr


def arrays_of(reads, k, filtered):
    from amira_amd.tokens import tokenize
    from amira_oracle import GeneMerGraph
    vocab, tokens, read_off, read_ids = tokenize(reads)
    g = GeneMerGraph({r: list(v) for r, v in reads.items()}, k, None)
    if filtered:
        g.filter_graph(2, 1)   # masked windows; the oracle's arrays number the surviving nodes
    arr = oracle_arrays(g, vocab, read_ids, read_off, k)
    return g, vocab, tokens, read_off, read_ids, arr


def flags_of(vocab, genes):
    flags = np.zeros(vocab.two_v // 2, np.uint8)
    for name in genes:
        if name in vocab.rank:
            flags[vocab.rank[name]] = 1
    return flags


CASES = [(seed, k, filtered) for seed in range(8) for k in (3, 5) for filtered in (False, True)]


@pytest.mark.parametrize("seed,k,filtered", CASES)
def test_depth_equals_the_oracle_driver(seed, k, filtered):
    from amira_oracle import driver
    reads, _ = random_reads(seed)
    g, _, _, read_off, _, arr = arrays_of(reads, k, filtered)
    alive = np.ones(len(arr["coverage"]), np.uint8)
    ks = list(range(3, 16, 2))
    pairs, n_alive = RW.depth_by_length(read_off, arr["tok_node"], alive, k, ks)
    got = {m: RW.mean_of(p, n_alive) for m, p in zip(ks, pairs)}
    want = driver.get_overall_mean_node_coverages(g)
    assert got == want
    assert {m: type(v) for m, v in got.items()} == {m: type(v) for m, v in want.items()}


@pytest.mark.parametrize("seed,k,filtered", CASES)
def test_non_amr_nodes_equal_the_oracle_removal(seed, k, filtered):
    reads, amr = random_reads(seed)
    g, vocab, tokens, read_off, _, arr = arrays_of(reads, k, filtered)
    alive = np.ones(len(arr["coverage"]), np.uint8)
    before = list(g.get_nodes())
    want_ids = RW.non_amr_nodes(tokens, read_off, arr["tok_node"], alive, k, flags_of(vocab, amr))
    g.remove_non_AMR_associated_nodes(amr)
    after = set(g.get_nodes())
    assert [i for i, h in enumerate(before) if h not in after] == want_ids.tolist()


@pytest.mark.parametrize("seed,k,filtered", CASES)
def test_component_validity_equals_the_oracle_driver(seed, k, filtered):
    reads, amr = random_reads(seed)
    g, vocab, tokens, read_off, _, arr = arrays_of(reads, k, filtered)
    alive = np.ones(len(arr["coverage"]), np.uint8)
    n_comp = int(arr["component"].max()) if len(arr["component"]) else 0
    n_reads, n_long = RW.component_amr_reads(tokens, read_off, arr["tok_node"], alive, arr["component"], n_comp, k,
                                             flags_of(vocab, amr), 2 * k - 1)
    # driver.choose_kmer_size's `valid` (oracle/amira_oracle/driver.py), on the oracle's own objects
    hashes = {n.__hash__() for name in amr for n in g.get_nodes_containing(name)}
    for c in g.components():
        members = [n.__hash__() for n in g.get_nodes_in_component(c)]
        rs = g.collect_reads_in_path([h for h in members if h in hashes])
        lens = [len(g.get_reads()[r]) for r in rs]
        assert n_reads[c - 1] == len(lens), c
        assert n_long[c - 1] == len([x for x in lens if x >= 2 * k - 1]), c
        want = True if not lens else len([x for x in lens if x >= 2 * k - 1]) / len(lens) >= 0.8
        assert RW.components_valid(n_reads, n_long)[c - 1] == want
    # labels without a surviving node have no read
    live_labels = set(g.components())
    assert all(n_reads[c - 1] == 0 for c in range(1, n_comp + 1) if c not in live_labels)
