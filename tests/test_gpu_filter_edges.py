"""GPU: the coverage filter's alive bytes (k_filter_nodes, k_filter_edges: four edges a thread, the last E mod 4 edges
one by one) against the rule spelt in numpy on the graph as it was BEFORE the call:
  a node stays if it was alive and its coverage >= min_node_cov;
  an edge stays if it was alive, both its ends stay, and (min_edge_cov <= 1 or its coverage >= min_edge_cov).
The read sets are chosen so that their directed-edge counts cover all four residues mod 4."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

K = 3
# residue of the number of directed edges mod 4 -> (seed, tandem reads).  Directed edges come in pairs except a
# self-loop's, so a tandem read (one gene five times: one node, one edge) makes the count odd.  Asserted in the tests: a
# changed generator must choose its seeds again.
READS_OF_RESIDUE = {0: (1, 0), 1: (1, 1), 2: (2, 0), 3: (2, 1)}


@functools.lru_cache(maxsize=None)
def read_set(seed, tandem):
    rng = np.random.default_rng(seed)
    V = 30
    flip = 2 * V - 1
    genome = rng.integers(0, 2 * V, 400)
    for i in range(1, len(genome)):  # no gene next to its own complement: no window is its own reverse complement
        while genome[i] == flip - genome[i - 1]:
            genome[i] = rng.integers(0, 2 * V)
    reads = []
    for _ in range(500 + seed):
        n = int(rng.integers(3, 25))
        a = int(rng.integers(0, len(genome) - n))
        r = genome[a:a + n].copy()
        if rng.random() < 0.3:  # one substitution: nodes and edges of low coverage
            j = int(rng.integers(0, n))
            r[j] = rng.integers(0, 2 * V)
            while (j > 0 and r[j] == flip - r[j - 1]) or (j + 1 < n and r[j] == flip - r[j + 1]):
                r[j] = rng.integers(0, 2 * V)
        reads.append(r if rng.random() < 0.5 else flip - r[::-1])
    for j in range(tandem):
        reads.insert(len(reads) // 2, np.full(5, 7 + j))
    toks = np.concatenate(reads).astype(np.int32)
    offs = np.zeros(len(reads) + 1, np.int64)
    np.cumsum([len(r) for r in reads], out=offs[1:])
    return toks, offs, 2 * V


@pytest.fixture(scope="module")
def eng():
    from amira_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def expected(nodes, edges, min_node_cov, min_edge_cov):
    n_keep = (nodes["alive"] != 0) & (nodes["coverage"] >= min_node_cov)
    e_keep = (edges["alive"] != 0) & n_keep[edges["src"]] & n_keep[edges["tgt"]]
    if min_edge_cov > 1:
        e_keep &= edges["coverage"] >= min_edge_cov
    return n_keep, e_keep


def filter_and_check(eng, thr):
    nodes, edges = eng.nodes(), eng.edges()
    n_keep, e_keep = expected(nodes, edges, *thr)
    eng.filter(*thr)
    after_n, after_e = eng.nodes()["alive"], eng.edges()["alive"]
    assert np.array_equal(after_n != 0, n_keep)
    assert np.array_equal(after_e != 0, e_keep)
    assert np.array_equal(after_e, np.where(e_keep, edges["alive"], 0))  # the bytes themselves: kept as they were, or 0
    return e_keep


@pytest.mark.parametrize("thr", [(3, 1), (1, 1), (2, 3)])
@pytest.mark.parametrize("residue", [0, 1, 2, 3])
def test_filter(eng, residue, thr):
    toks, offs, two_v = read_set(*READS_OF_RESIDUE[residue])
    eng.set_reads(toks, offs, two_v)
    eng.build(K)
    E = eng.counts()["n_edges"]
    assert E % 4 == residue and E > 1024     # more than one workgroup's edges, and the tail of this residue
    e_keep = filter_and_check(eng, thr)
    assert e_keep.all() if thr == (1, 1) else 0 < e_keep.sum() < E


@pytest.mark.parametrize("residue", [1, 3])
def test_filter_twice(eng, residue):
    """a byte that is 0 stays 0: edges removed by id, both ends alive, are not brought back by a filter that removes
    nothing, and a second filter starts from what the first left"""
    toks, offs, two_v = read_set(*READS_OF_RESIDUE[residue])
    eng.set_reads(toks, offs, two_v)
    eng.build(K)
    E = eng.counts()["n_edges"]
    gone = np.unique(np.concatenate([[0, 5, 6, 7, E - 1], np.arange(1024, 1028)])).astype(np.int32)  # a tail edge, a whole quad
    eng.remove_edges(gone)
    first = filter_and_check(eng, (1, 1))
    assert first.sum() == E - len(gone) and not first[gone].any()
    second = filter_and_check(eng, (3, 1))
    third = filter_and_check(eng, (2, 3))
    assert not (second & ~first).any() and not (third & ~second).any() and 0 < third.sum() < first.sum()
