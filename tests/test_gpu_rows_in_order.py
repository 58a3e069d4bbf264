"""Adjacency rows on every tier boundary of the ordering code (amira_amd/csrc/amg_rows.h): rows of 1 and 2 edge ids are
placed inline, rows of 3 .. 64 by a wave, rows of 65 .. 1024 by a workgroup that ranks by counting, longer rows through
a bitmap over the edge ids.  The full lists (amg_adjacency.hip) against numpy, the live lists (amg_live_rows.hip) through
the junction search of bubble popping, which returns its paths in list order, against the host's reference-shaped
search: made from the live edges, patched after nodes died, and through every transition of the lists' state."""
import numpy as np
import pytest

import procedures as P
from derive_cases import apply_step, build_orders
from helpers import check_corrected, compare_engine_to_oracle, flat_positions, oracle_arrays
from test_gpu_bubbles import _paths_per_start

pytestmark = pytest.mark.gpu

BOUNDARIES = (1, 2, 3, 63, 64, 65, 1024, 1025)


@pytest.fixture(scope="module")
def eng():
    from amira_amd import Engine
    e = Engine(0)
    yield e
    e.close()


# ------------------------------------------------------------------ 1. the full lists
@pytest.mark.parametrize("sort", [False, True])
def test_full_lists_on_every_tier_boundary(eng, monkeypatch, sort):
    """eight hubs, hub h one gene-mer (a_h, b_h, c_h) followed by n_h different successors, n_h = 1, 2, 3, 63, 64, 65,
    1024, 1025: Engine.node_adj() is the stable sort of the edges by row, by the ticket route and by the library sort
    (AMG_ADJ_SORT=1)"""
    from amira_amd import tokenize
    if sort:
        monkeypatch.setenv("AMG_ADJ_SORT", "1")
    reads = {}
    for h, n in enumerate(BOUNDARIES):
        for i in range(n):
            reads[f"r{h}_{i:04d}"] = [f"+a{h}", f"+b{h}", f"+c{h}", f"+x{h}_{i}", f"+y{h}_{i}", f"+z{h}_{i}"]
    vocab, toks, offs, _ = tokenize(reads)
    eng.set_reads(toks, offs, vocab.two_v)
    eng.build(3)
    e = eng.edges()
    n_nodes = eng.counts()["n_nodes"]
    row = 2 * e["src"].astype(np.int64) + np.where(e["sdir"] > 0, 0, 1)
    want_off = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=2 * n_nodes))])
    want_ids = np.argsort(row, kind="stable")
    assert set(BOUNDARIES) <= set(np.diff(want_off).tolist())
    off, ids = eng.node_adj()
    assert np.array_equal(off, want_off)
    assert np.array_equal(ids, want_ids)


# ------------------------------------------------------------------ 2. and 3. the live lists
N_BRANCH = 1100


class _Fan:
    """the graph of N_BRANCH reads [+a, +b, +c, +x_i, +d, +e, +f], k = 3: the gene-mer (a, b, c) — the hub — has one
    live edge per branch, in read order; (d, e, f) is reached from every branch and is the stop junction"""

    def __init__(self):
        from amira_amd import GeneMerGraph
        self.k = 3
        self.g = g = GeneMerGraph({f"r{i:04d}": ["+a", "+b", "+c", f"+x{i}", "+d", "+e", "+f"] for i in range(N_BRANCH)},
                                  self.k)
        tokens = g._v().arrays["nodes"]["tokens"]
        names = [frozenset(g._vocab.name_of(t) for t in row) for row in tokens.tolist()]
        self.branch_of = {}    # node id of (b, c, x_i) -> i
        for n, genes in enumerate(names):
            if genes >= {"b", "c"} and len(genes) == 3 and not genes & {"a", "d"}:
                self.branch_of[n] = int(next(x for x in genes if x.startswith("x"))[1:])
        self.second = {i: n for n, i in self.branch_of.items()}
        assert sorted(self.second) == list(range(N_BRANCH))
        (hub,) = g.get_nodes_containing("a")
        forward = len(hub.get_forward_edge_hashes()) > len(hub.get_backward_edge_hashes())
        self.hub = (hub.__hash__(), 1 if forward else -1)
        self.hub_id = names.index(frozenset("abc"))

    def hub_edges(self):
        """per branch, in list order: (i, hash of the hub's edge to (b, c, x_i), hash of that edge's twin)"""
        g = self.g
        hub = g.get_node_by_hash(self.hub[0])
        out = []
        for h in (hub.get_forward_edge_hashes() if self.hub[1] == 1 else hub.get_backward_edge_hashes()):
            target = g.get_edge_by_hash(h).get_targetNode()
            (twin,) = [t for t in target.get_forward_edge_hashes() + target.get_backward_edge_hashes()
                       if g.get_edge_by_hash(t).get_targetNode() == hub]
            out.append((self.branch_of[g._node_id(target)], h, twin))
        return out

    def check(self, live):
        """the device's paths per start junction are the host's; the hub lists one path per live branch, in list order"""
        g = self.g
        found = g._engine.junction_paths(4 * self.k)
        assert found["flags"] == 0
        v = g._v()
        v.ensure_hashes(np.unique(np.concatenate([found["path_node"], found["junction_node"]])).tolist())
        junction = [(v.node_hash[n], s) for n, s in zip(found["junction_node"].tolist(), found["junction_dir"].tolist())]
        off, ids, dirs = found["path_off"].tolist(), found["path_node"].tolist(), found["path_dir"].tolist()
        got, second = {}, []
        for p, j in enumerate(found["path_start"].tolist()):
            got.setdefault(junction[j], []).append([(v.node_hash[i], s) for i, s in zip(ids[off[p]:off[p + 1]],
                                                                                         dirs[off[p]:off[p + 1]])])
            if junction[j] == self.hub:
                assert ids[off[p]] == self.hub_id
                second.append(self.branch_of[ids[off[p] + 1]])
        assert got == _paths_per_start(g, 4 * self.k)
        assert second == sorted(live) and len(second) == len(live)


def _thin(live, target):
    """victims that leave `target` of `live` (a list in list order): every other surviving one from the front, again
    and again — never a tail alone, so that what survives is not a prefix of the row"""
    live, victims = list(live), []
    while len(live) > target:
        gone = live[0::2][:len(live) - target]
        victims += gone
        live = sorted(set(live) - set(gone))
    return victims, live


def test_live_lists_made_on_every_tier_boundary():
    """edges out of the hub are removed (remove_edge: the lists are made again from the live edges every time) until
    1025, 1024, 65, 64, 63, 3 and 2 are live, victims spread over the row; the stop junction's backward row keeps its
    1 100 entries throughout (the bitmap route).  Each victim goes with its twin, as the reference's own removals do:
    with the twin alone left, the host's search, which asks for the direction between the last two nodes of a path, has
    no answer for a path that arrives at the hub over it."""
    fan = _Fan()
    edges = {i: (h, twin) for i, h, twin in fan.hub_edges()}
    live = sorted(edges)
    assert live == list(range(N_BRANCH))
    for target in (1025, 1024, 65, 64, 63, 3, 2):
        victims, live = _thin(live, target)
        for i in victims:
            fan.g.remove_edge(edges[i][0])
            fan.g.remove_edge(edges[i][1])
        assert len(live) == target and live != list(range(target))
        fan.check(live)


@pytest.mark.parametrize("patch", [True, False])
def test_live_lists_patched_on_every_tier_boundary(monkeypatch, patch):
    """the lists exist; successor nodes of the hub are removed to take the hub's row 1100 -> 1025 -> 1024 -> 65 -> 64 ->
    3 -> 2: the lists are brought up to date in place (k_lr_patch), or made again with AMG_NO_LADJ_PATCH=1.  The nodes of
    a step go in one call of remove_node's device entry (amg_remove_nodes, through _remove_node_ids): remove_node itself
    drops the host view per node and looks the node up in a view made again, a second per node on this graph and a
    thousand nodes to remove; the state of the lists moves the same way per call as per node."""
    if not patch:
        monkeypatch.setenv("AMG_NO_LADJ_PATCH", "1")
    fan = _Fan()
    live = list(range(N_BRANCH))
    assert fan.g._engine.junction_paths(4 * fan.k)["flags"] == 0
    for target in (1025, 1024, 65, 64, 3, 2):
        victims, live = _thin(live, target)
        fan.g._remove_node_ids([fan.second[i] for i in victims])
        fan.check(live)


# ------------------------------------------------------------------ 4. the state of the lists
def _low_tenth(values):
    """a threshold that the lowest tenth of the coverages does not reach"""
    values = sorted(values)
    return values[len(values) // 10] + 1


def _node_threshold(g):
    return [("filter", _low_tenth(n.get_node_coverage() for n in g.get_nodes().values()), 1)]


def _edge_threshold(g):
    return [("filter", 3, max(2, _low_tenth(e.get_edge_coverage() for e in g.get_edges().values())))]


def _listed_nodes_then_edges(g):
    return [("nodes", _every_ninth_node), ("edges", _every_eleventh_edge_pair)]


def _every_ninth_node(g):
    live = list(g.get_nodes())
    return live[len(live) // 4: 3 * len(live) // 4: 9]


def _every_eleventh_edge_pair(g):
    out = []
    for h in list(g.get_edges())[5::11]:
        e = g.get_edges()[h]
        a, b = g.get_edge_hashes_between_nodes(e.get_sourceNode(), e.get_targetNode())
        if not isinstance(a, list) and not isinstance(b, list):
            out += [a, b]
    return list(dict.fromkeys(out))


@pytest.mark.parametrize("patch", [True, False])
@pytest.mark.parametrize("steps", [
    _node_threshold,             # nodes die: the lists are behind the nodes, or absent
    _edge_threshold,             # an edge threshold above 1: absent
    _listed_nodes_then_edges,    # listed edges go while the lists are behind the nodes: absent
], ids=["node-threshold", "edge-threshold", "edges-while-behind-nodes"])
def test_list_state_through_every_transition(eng, monkeypatch, steps, patch):
    """filter -> correct_reads (re-threading: the lists are current) -> `steps` -> correct_reads again, which walks the
    lists that the state promises — patched, or made again — against the oracle; with and without AMG_NO_LADJ_PATCH=1"""
    from amira_amd import tokenize
    from amira_oracle import GeneMerGraph
    if not patch:
        monkeypatch.setenv("AMG_NO_LADJ_PATCH", "1")
    reads, pos, fq = P.synth_inputs(17, 800, 40, 150, 0.05)
    k = 5
    vocab, toks, offs, read_ids = tokenize(reads)
    eng.set_reads(toks, offs, vocab.two_v)
    gs, ge = flat_positions(read_ids, reads, pos)
    eng.set_positions(gs, ge, np.asarray([len(fq[r]["sequence"]) for r in read_ids], dtype=np.int64))
    eng.build(k)
    g = GeneMerGraph(reads, k, {r: list(v) for r, v in pos.items()})
    order, eorder = build_orders(g)
    apply_step(g, ("filter", 3, 1), order, eorder, eng)
    # (the reference's correct_reads rewrites the gene positions it was given: the first correction has an oracle graph
    # of its own)
    g0 = GeneMerGraph(reads, k, {r: list(v) for r, v in pos.items()})
    g0.filter_graph(3, 1)
    check_corrected(eng, vocab, read_ids, *g0.correct_reads(fq))
    assert "live_adjacency" in [s for s, _ in eng.timings()]
    before = eng.counts()
    for step in steps(g):
        apply_step(g, step, order, eorder, eng)
    after = eng.counts()
    assert 0 < after["n_live_edges"] < before["n_live_edges"]
    compare_engine_to_oracle(eng, oracle_arrays(g, vocab, read_ids, offs, k), live_only=True)
    check_corrected(eng, vocab, read_ids, *g.correct_reads(fq))
    assert "live_adjacency" in [s for s, _ in eng.timings()]
