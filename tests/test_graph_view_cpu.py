"""The object view (amira_amd.graph_view._View) without a device: built from a stub array source that serves the CPU
oracle's graph in the engine's conventions (helpers.oracle_arrays), and compared with that oracle graph — order of
nodes and edges, every node's fields and lazy lists, the per-read lists, the lookups that must not complete the node
dict, dead nodes and edges, disposal, and which arrays are fetched when."""
import functools

import numpy as np
import pytest

import procedures as P
from helpers import oracle_arrays

CASES = [("eight", 3), ("nine", 5)]
LAZY_FETCHES = {"read_node_ids", "read_dirs", "node_reads"}


def _csr(lists, dtype=np.int32):
    off = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([len(x) for x in lists], out=off[1:])
    return off, np.asarray([x for row in lists for x in row], dtype)


class Source:
    """what a _View asks an Engine for, over the arrays of an oracle graph; `calls` records the fetches"""

    def __init__(self, arr, dead_nodes=(), dead_edges=()):
        self.arr, self.calls = arr, []
        self.node_alive = np.ones(len(arr["coverage"]), np.uint8)
        self.node_alive[list(dead_nodes)] = 0
        self.edge_alive = np.ones(len(arr["src"]), np.uint8)
        self.edge_alive[list(dead_edges)] = 0

    def nodes(self):
        self.calls.append("nodes")
        return {**{n: self.arr[n] for n in ("tokens", "coverage", "component", "first_dir")}, "alive": self.node_alive}

    def edges(self):
        self.calls.append("edges")
        return {**{n: self.arr[n] for n in ("src", "tgt", "sdir", "tdir")}, "coverage": self.arr["ecov"],
                "alive": self.edge_alive}

    def node_adj(self):
        self.calls.append("node_adj")
        return _csr(self.arr["adj"])

    def read_node_ids(self):
        self.calls.append("read_node_ids")
        return self.arr["tok_node"]

    def read_dirs(self):
        self.calls.append("read_dirs")
        return self.arr["tok_dir"]

    def node_reads(self):
        self.calls.append("node_reads")
        return _csr(self.arr["node_reads"])

    def read_node_ids_of(self, starts, counts):
        self.calls.append("read_node_ids_of")
        cuts = np.zeros(len(starts) + 1, np.int64)
        np.cumsum(counts, out=cuts[1:])
        parts = [self.arr["tok_node"][a:a + n] for a, n in zip(starts, counts)]
        return (np.concatenate(parts) if parts else np.zeros(0, np.int32)), cuts


@functools.lru_cache(maxsize=None)
def _case(name, k):
    """the oracle graph of a fixture and what a view of it is built from (shared by the tests, never changed)"""
    from amira_amd.tokens import tokenize
    from amira_oracle import GeneMerGraph as Oracle
    calls, pos = P.fixture(name)
    vocab, _, offs, ids = tokenize(calls)
    o = Oracle(dict(calls), k, {r: list(v) for r, v in pos.items()})
    gs = np.asarray([x[0] for r in ids for x in pos[r]], np.int64)
    ge = np.asarray([x[1] for r in ids for x in pos[r]], np.int64)
    return o, oracle_arrays(o, vocab, ids, offs, k), vocab, ids, offs, (gs, ge), calls


def _view(name, k, positions=True, **dead):
    from amira_amd.graph_view import _RowIndex, _View
    o, arr, vocab, ids, offs, flat, calls = _case(name, k)
    src = Source(arr, **dead)
    return _View(src, vocab, k, ids, offs, flat if positions else None, {}, _RowIndex(calls, ids), {}), src, o


def _genes(gene_mer_genes):
    return [(g.get_strand(), g.get_name()) for g in gene_mer_genes]


@pytest.mark.parametrize("name,k", CASES)
def test_nodes_edges_and_read_lists_match_the_oracle(name, k):
    v, src, o = _view(name, k)
    assert list(v.nodes) == list(o.get_nodes()) and list(v.edges) == list(o.get_edges())
    assert not LAZY_FETCHES & set(src.calls)           # making the view and every node and edge fetched none of them
    for h, want in o.get_nodes().items():
        got = v.nodes[h]
        assert got.get_node_coverage() == want.get_node_coverage() and got.get_component() == want.get_component()
        assert _genes(got.get_canonical_geneMer()) == _genes(want.get_canonical_geneMer())
        assert _genes(got.get_reverse_geneMer()) == _genes(want.get_reverse_geneMer())
        assert got.get_geneMer().get_geneMerDirection() == want.get_geneMer().get_geneMerDirection()
        assert list(got.get_reads()) == list(want.get_reads())
        assert got.get_forward_edge_hashes() == want.get_forward_edge_hashes()
        assert got.get_backward_edge_hashes() == want.get_backward_edge_hashes()
    for h, want in o.get_edges().items():
        got = v.edge_by_hash(h)
        assert (got.get_sourceNode().__hash__(), got.get_targetNode().__hash__(), got.get_sourceNodeDirection(),
                got.get_targetNodeDirection(), got.get_edge_coverage()) == (
            want.get_sourceNode().__hash__(), want.get_targetNode().__hash__(), want.get_sourceNodeDirection(),
            want.get_targetNodeDirection(), want.get_edge_coverage())
    assert list(v.readNodes) == list(o.get_readNodes()) and len(v.readNodes) == len(o.get_readNodes())
    for rid, want in o.get_readNodes().items():
        assert v.readNodes[rid] == want
        assert v.readNodeDirections[rid] == o.get_readNodeDirections()[rid]
        assert v.readNodePositions[rid] == o.get_readNodePositions()[rid]
    short = next(iter(o.get_short_read_annotations()), None)
    assert short is None or (short not in v.readNodes and short not in list(v.readNodes))
    assert "no such read" not in v.readNodes


@pytest.mark.parametrize("name,k", CASES)
def test_without_positions_every_window_has_none(name, k):
    v, _, o = _view(name, k, positions=False)
    for rid, want in list(o.get_readNodes().items())[:50]:
        assert v.readNodePositions[rid] == [None] * len(want)


@pytest.mark.parametrize("name,k", CASES)
def test_per_read_fetches_first_one_by_one_then_the_whole_array(name, k):
    v, src, o = _view(name, k)
    reads = list(o.get_readNodes())
    for rid in reads:
        assert v.readNodes[rid] == o.get_readNodes()[rid]
    assert src.calls.count("read_node_ids_of") == min(64, len(reads))
    assert src.calls.count("read_node_ids") == (1 if len(reads) > 64 else 0)
    assert not {"read_dirs", "node_reads"} & set(src.calls) and not v._nodes_complete


@pytest.mark.parametrize("name,k", CASES)
def test_lookups_on_a_fresh_view_do_not_complete_the_node_dict(name, k):
    v, _, o = _view(name, k)
    hashes = list(o.get_nodes())
    D = len(hashes)
    some = list(range(0, D, 3))
    v.ensure_hashes(some + [-1, -2])
    assert [v.node_hash[i] for i in some] == [hashes[i] for i in some] and v.node_hash[1] is None
    assert v.hash_at(1) == hashes[1] and v.hash_at(0) == hashes[0]
    assert [v.node_of_hash[hashes[i]] for i in some] == some and hashes[1] in v.node_of_hash
    first = v.node_by_hash(hashes[3])               # hashed, object not made yet
    assert first.__hash__() == hashes[3] and v.node_at(3) is first and v.node_by_hash(hashes[3]) is first
    assert v.node_at(4).__hash__() == hashes[4] and v.node_by_hash(hashes[4]) is v.node_at(4)
    ids = np.asarray([2, 5, 5, D - 1], np.int64)
    t = v.node_hash_table(ids)
    assert len(t) == D + 2 and t[-1] is None and t[-2] is None and t[ids].tolist() == [hashes[i] for i in ids.tolist()]
    assert not v._nodes_complete and list(v._nodes) == [hashes[3], hashes[4]]
    before = {i: v.node_hash[i] for i in range(D) if v.node_hash[i] is not None}
    assert v.node_by_hash(hashes[7]).__hash__() == hashes[7]     # a hash the view cannot know yet: makes them all
    assert v._nodes_complete and list(v.nodes) == hashes and v.nodes[hashes[3]] is first
    assert all(v.node_hash[i] == h and v.hash_at(i) == h and v.node_of_hash[h] == i for i, h in before.items())
    assert v.node_by_hash(12345) is None and v.node_of_hash.get(12345, "absent") == "absent"
    full = v.node_hash_table()
    assert full is t and full[:D].tolist() == hashes and full[-1] is None and full[-2] is None
    fresh, _, _ = _view(name, k)
    assert fresh.node_hash_table()[:D].tolist() == hashes and fresh._nodes_complete


@pytest.mark.parametrize("name,k", CASES)
def test_dead_nodes_and_edges_are_absent(name, k):
    o, arr = _case(name, k)[:2]
    dead_nodes = set(range(0, len(arr["coverage"]), 7))
    # every fifth edge, and — as on the device, where a removed node takes its edges along — the edges of dead nodes
    dead_edges = set(range(0, len(arr["src"]), 5)) | {
        e for e in range(len(arr["src"])) if int(arr["src"][e]) in dead_nodes or int(arr["tgt"][e]) in dead_nodes}
    v, _, _ = _view(name, k, dead_nodes=dead_nodes, dead_edges=dead_edges)
    node_hashes, edge_hashes = list(o.get_nodes()), list(o.get_edges())
    gone = {edge_hashes[e] for e in dead_edges}
    assert all(v.node_at(i) is None and v.hash_at(i) is None for i in dead_nodes)
    live = [i for i in range(len(node_hashes)) if i not in dead_nodes]
    for i in live[::3]:                                     # lazily made edge lists, before `edges` is asked for
        node, want = v.node_at(i), o.get_nodes()[node_hashes[i]]
        assert node.get_forward_edge_hashes() == [h for h in want.get_forward_edge_hashes() if h not in gone]
        assert node.get_backward_edge_hashes() == [h for h in want.get_backward_edge_hashes() if h not in gone]
    assert list(v.nodes) == [node_hashes[i] for i in live]
    assert list(v.edges) == [h for h in edge_hashes if h not in gone]
    assert all(v.node_by_hash(node_hashes[i]) is None for i in dead_nodes)
    assert any(len(o.get_nodes()[node_hashes[i]].get_forward_edge_hashes()) > len(v.node_at(i).get_forward_edge_hashes())
               for i in live)                               # (the case has live nodes that lost a forward edge)


def test_after_dispose_made_lists_answer_and_unmade_ones_say_closed():
    v, _, o = _view("eight", 3)
    hashes = list(o.get_nodes())
    looked, unlooked = v.node_at(0), v.node_at(1)
    fw, bw, reads = (list(looked.get_forward_edge_hashes()), list(looked.get_backward_edge_hashes()),
                     list(looked.get_reads()))
    rid = next(iter(o.get_readNodes()))
    made = v.readNodes[rid]
    v.dispose()
    assert looked.get_forward_edge_hashes() == fw and looked.get_backward_edge_hashes() == bw
    assert list(looked.get_reads()) == reads == list(o.get_nodes()[hashes[0]].get_reads())
    assert made == o.get_readNodes()[rid]
    for ask in (unlooked.get_forward_edge_hashes, unlooked.get_backward_edge_hashes, unlooked.get_list_of_reads):
        with pytest.raises(RuntimeError, match="the graph has been closed"):
            ask()
    assert v.readNodes is None and v.node_of_hash is None and v.arrays.source is None
