"""The HIP-backed drop-in (amira_amd.GeneMerGraph & co.) against goldens produced by the
REAL reference: the same procedures (tests/golden/procedures.py) that generated
goldens.json run against the product through its reference-compatible Python API."""
import json
import os
import types

import pytest

import procedures as P
from seed0 import run_case_seed0

pytestmark = pytest.mark.gpu
GOLD = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "goldens.json")))


def _product():
    import amira_amd
    from amira_amd.graph_utils import choose_kmer_size, get_overall_mean_node_coverages, iterative_bubble_popping
    from amira_amd.pre_processing import process_pandora_json
    from amira_amd.result_utils import write_pandora_gene_calls
    return types.SimpleNamespace(GeneMerGraph=amira_amd.GeneMerGraph, Gene=amira_amd.Gene,
                                 GeneMer=amira_amd.GeneMer, choose_kmer_size=choose_kmer_size,
                                 get_overall_mean_node_coverages=get_overall_mean_node_coverages,
                                 iterative_bubble_popping=iterative_bubble_popping,
                                 process_pandora_json=process_pandora_json,
                                 write_pandora_gene_calls=write_pandora_gene_calls)


class _RewriteCounters:
    """the product with its graphs' engines watched: how far `pop_rewrite_stats` moved while a procedure ran (engines
    are pooled, so every engine counts from where it stood when a graph of the procedure first had it)"""

    def __init__(self, product):
        self._seen = {}
        make = product.GeneMerGraph

        def graph(*args, **kwargs):
            g = make(*args, **kwargs)
            self._seen.setdefault(id(g._engine), (g._engine, dict(g._engine.pop_rewrite_stats)))
            return g

        self.impl = types.SimpleNamespace(**{**vars(product), "GeneMerGraph": graph})

    def moved(self):
        return {key: sum(engine.pop_rewrite_stats[key] - first[key] for engine, first in self._seen.values())
                for key in ("calls", "rewritten", "declined")}


@pytest.mark.parametrize("name", list(P.CASES))
def test_product_matches_reference(name):
    proc, args, _ = P.CASES[name]
    if proc in (P.p_planted, P.p_cluster_fixture, P.p_front_end) and os.environ.get("PYTHONHASHSEED") != "0":
        got = run_case_seed0("product", name)  # set-order dependent in the reference: seed 0
    elif proc is P.p_bubbles_random and name in P.NOT_VACUOUS:
        # the large gene-mer sizes: the reads were rewritten by the device's call, not by the loop it may fall back to
        watched = _RewriteCounters(_product())
        got = json.loads(json.dumps(P.run_case(watched.impl, name)))
        moved = watched.moved()
        assert moved["calls"] >= 1 and moved["rewritten"] >= 1 and moved["declined"] == 0, moved
    else:
        got = json.loads(json.dumps(proc(_product(), *args)))
    assert got == GOLD[name]


@pytest.mark.parametrize("name", ["planted_small", "planted_dense_k5"])
def test_clustering_one_gene_per_native_call(name, monkeypatch):
    """read-path clustering takes the genes of interest a bounded number at a time (64): one at a time gives the same"""
    monkeypatch.setenv("AMG_CLUSTER_GENES_PER_CALL", "1")
    assert run_case_seed0("product", name) == GOLD[name]


def test_reference_api_surface():
    """spot checks in the style of the reference's own unit tests (tests/test_gene_mer_graph.py)."""
    import amira_amd
    from amira_amd import Gene, GeneMer, GeneMerGraph, Read
    g = GeneMerGraph({"read1": ["+gene1", "-gene2", "+gene3", "-gene4"],
                      "read2": ["+gene1", "-gene2", "+gene3"]}, 3)
    assert g.get_total_number_of_nodes() == 2 and g.get_total_number_of_edges() == 2
    assert g.get_total_number_of_reads() == 2 and g.get_kmerSize() == 3
    covs = sorted(n.get_node_coverage() for n in g.all_nodes())
    assert covs == [1, 2]
    gm = Read("read2", ["+gene1", "-gene2", "+gene3"]).get_geneMers(3)[0][0]
    node = g.get_node(gm)
    assert node.get_node_coverage() == 2 and node.get_list_of_reads() == ["read1", "read2"]
    assert node.__hash__() == gm.__hash__() == g.get_readNodes()["read2"][0]
    assert g.get_readNodeDirections()["read2"] == [gm.get_geneMerDirection()]
    assert [n.__hash__() for n in g.get_nodes_containing("gene4")] == [g.get_readNodes()["read1"][1]]
    with pytest.raises(AssertionError):
        g.get_nodes_containing("+gene4")
    with pytest.raises(AssertionError):
        GeneMerGraph({"r": ["+a", "-a"]}, 2)          # palindrome (construct_gene_mer.py:23-25)
    with pytest.raises(AssertionError):
        GeneMerGraph({"r": ["gene_without_strand", "+b", "+c"]}, 3)
    with pytest.raises(AssertionError):
        g.get_node(GeneMer([Gene("+x"), Gene("+y"), Gene("+z")]))
    short = GeneMerGraph({"s": ["+a", "-b"], "t": ["+a", "-b", "+c"]}, 3)
    assert short.get_short_read_annotations() == {"s": ["+a", "-b"]}
    assert list(short.get_readNodes()) == ["t"]
    assert amira_amd.build_graph({"t": ["+a", "-b", "+c"]}, 3).get_total_number_of_nodes() == 1
