"""GPU: the junction path search of bubble popping (amg_junction_paths, amira_amd/csrc/amg_bubbles.hip: k_bj_flag,
k_bj_rows, k_bj_dfs on wave_dfs of amg_wave_dfs.h) on ARBITRARY graphs and at its limits, against
tests/junction_search.py, which tests/test_junction_search_cpu.py holds to the Python oracle.

Every graph goes in as reads at gene-mer size 1 (tests/graph_shapes.py) and is first held to the sequential C oracle
(compare_engine_to_sweep): a difference in the search is then not a difference in the build.  Then every array of
Engine.junction_paths and its flags equal the reference exactly.

  depth      a ladder whose two paths have 64 nodes: the stack fills all 64 lanes; distances either side of every bound
  arguments  what the two calls refuse and what they leave behind
  random     40 nodes, 60 pairs, self-loops, random strands; with pairs repeated in their other class (flag bit 0)
  starts     8 400 junctions: more than one scan tile between count, scan and emit
  live       the search on lists made from a filtered graph, patched after nodes died, and made again
  budget     AMG_TEST_BJ_STEPS on its boundary (flag bit 1); the real bound of 2^24 steps is not run
  caller     GeneMerGraph declines the device's answer where the reference fails"""
import ctypes as C

import numpy as np
import pytest

import graph_shapes as G
import junction_search as JS
import token_oracle
from helpers import compare_engine_to_sweep

pytestmark = pytest.mark.gpu

BJ_MULTI, BJ_BUDGET = 1, 2


@pytest.fixture(scope="module")
def eng():
    from amira_amd import Engine
    e = Engine(0)
    yield e
    e.close()


class Ref:
    """a graph, its C oracle (built, unchanged) and the reference's answers by distance, shared between the tests"""

    def __init__(self, shape, seed):
        self.shape, self.D, self.tokens = shape, shape.D, G.shape_tokens(shape, seed)
        self.sweep = self.new_sweep()
        self.edges, self.nodes = self.sweep.edges(), self.sweep.nodes()
        self._found = {}

    def new_sweep(self):
        s = token_oracle.Sweep(*self.tokens)
        s.build(1)
        return s

    def found(self, distance):
        if distance not in self._found:
            self._found[distance] = JS.search(self.edges, self.edges["alive"], self.nodes["alive"], distance)
        return self._found[distance]


_REFS = {}


def ref_of(key, make, seed=1):
    if key not in _REFS:
        _REFS[key] = Ref(make(), seed)
    return _REFS[key]


def build(eng, ref, what):
    eng.set_reads(*ref.tokens)
    eng.build(1)
    compare_engine_to_sweep(eng, ref.sweep, what)


def same(got, want, what, flags=0):
    assert got["flags"] == flags, (what, got["flags"], flags)
    for key in JS.ARRAYS:
        a, b = got[key], getattr(want, key)
        assert a.dtype == b.dtype and np.array_equal(a, b), (what, key, len(a), len(b))


# ------------------------------------------------------------------ 1. depth
@pytest.mark.parametrize("strand_seed", [None, 5])
def test_ladder_of_64(eng, strand_seed):
    ref = ref_of(("ladder", strand_seed), lambda: JS.ladder(62, 62, 3, strand_seed)[0])
    build(eng, ref, ("ladder", strand_seed))
    for d in (2, 3, 20, 21, 63, 64):
        want = ref.found(d)
        same(eng.junction_paths(d), want, ("ladder", strand_seed, d))
        assert len(want.junction_node) == 2
        if d < 64:
            assert len(want.path_start) == 0
    # two paths of 64 nodes, found from either end
    assert np.diff(want.path_off).tolist() == [64] * 4 and want.path_start.tolist() == [0, 0, 1, 1]
    assert want.enters.tolist() == [1 + 62 + 62 + 2] * 2


def test_uneven_ladder(eng):
    ref = ref_of("ladder 61 62", lambda: JS.ladder(61, 62)[0])
    build(eng, ref, "ladder 61 62")
    for d in (62, 63, 64):
        same(eng.junction_paths(d), ref.found(d), ("ladder 61 62", d))
    assert len(ref.found(62).path_start) == 0
    assert len(ref.found(63).path_start) == 0 and ref.found(63).stops_per_start.tolist() == [1, 1]   # one record: no bubble
    assert np.diff(ref.found(64).path_off).tolist() == [63, 64, 63, 64]


# ------------------------------------------------------------------ 2. arguments
def test_arguments(eng):
    from amira_amd import Engine, _ffi
    from amira_amd._ffi import ptr
    lib = _ffi.lib
    ref = ref_of(("distinct", 40, 0), lambda: JS.distinct_pairs(40, 0), 0)
    build(eng, ref, "arguments")
    want = ref.found(6)
    same(eng.junction_paths(6), want, "before")
    assert len(want.path_start) > 0
    sizes = (C.c_int64 * 4)(-7, -7, -7, -7)
    for bad in (1, 65, 0, -1):
        assert lib.amg_junction_paths(eng._h, bad, sizes) == _ffi.E_ARG
    assert lib.amg_junction_paths(eng._h, 6, None) == _ffi.E_ARG
    assert list(sizes) == [-7] * 4
    # the last result is still there
    out = {k: np.full_like(getattr(want, k), -1) for k in JS.ARRAYS}
    assert lib.amg_get_junction_paths(eng._h, *[ptr(out[k]) for k in JS.ARRAYS]) == 0
    same(dict(out, flags=0), want, "after refused calls")
    # every output pointer NULL; one array alone
    assert lib.amg_get_junction_paths(eng._h, None, None, None, None, None, None) == 0
    alone = np.full_like(want.path_off, -1)
    assert lib.amg_get_junction_paths(eng._h, None, None, None, ptr(alone), None, None) == 0
    assert np.array_equal(alone, want.path_off)
    # a context that has not searched
    fresh = Engine(0)
    try:
        assert lib.amg_get_junction_paths(fresh._h, None, None, None, None, None, None) == -3      # AMG_E_STATE
    finally:
        fresh.close()


# ------------------------------------------------------------------ 3. random graphs
def _distances(D):
    return [d for dd, d in JS.DISTINCT if dd == D] + ([64] if D == 40 else [])


@pytest.mark.parametrize("D", [40, 30])
def test_random_graphs(eng, D):
    kept = 0
    for seed in JS.SEEDS:
        ref = ref_of(("distinct", D, seed), lambda: JS.distinct_pairs(D, seed), seed)
        build(eng, ref, ("distinct", D, seed))
        for d in _distances(D):
            want = ref.found(d)
            assert not want.multi
            same(eng.junction_paths(d), want, ("distinct", D, seed, d))
            kept += len(want.path_start)
        if D == 40:     # the larger bound changes nothing beyond the longest simple path
            same(eng.junction_paths(40), ref.found(64), ("distinct", D, seed, "40 = 64"))
    assert kept > 1000
    if D == 40:         # paths that only the distances past 20 reach
        assert any(int(np.diff(ref_of(("distinct", 40, s), None).found(64).path_off).max()) > 21 for s in JS.SEEDS)


@pytest.mark.parametrize("D", [40, 30])
def test_random_graphs_with_repeated_pairs(eng, D):
    """bit 0 follows `multi`; the paths come back with it set and are still the reference's"""
    seen = set()
    for seed in JS.SEEDS:
        ref = ref_of(("repeated", D, seed), lambda: JS.repeated_pairs(D, seed), seed)
        build(eng, ref, ("repeated", D, seed))
        for d in _distances(D):
            want = ref.found(d)
            same(eng.junction_paths(d), want, ("repeated", D, seed, d), BJ_MULTI if want.multi else 0)
            seen.add(want.multi)
    assert seen == {True, False}


def test_two_edges_to_a_dead_end(eng):
    """two edges between two nodes that no path ends over at a junction: bit 0 stays clear.  (Node 0 is the dead end:
    a search that looked at the node before its START would look at lane 63's node, which is node 0.)"""
    answers = set()
    for turn in (0, 1):
        ref = ref_of(("dead end", turn), lambda: JS.dead_end_pair(turn))
        build(eng, ref, ("dead end", turn))
        e = ref.edges
        assert int(((e["src"] == 0) & (e["tgt"] == 1)).sum()) == 2 and int(((e["src"] == 1) & (e["tgt"] == 0)).sum()) == 2
        for d in (2, 3, 4, 64):
            want = ref.found(d)
            same(eng.junction_paths(d), want, ("dead end", turn, d), BJ_MULTI if want.multi else 0)
        answers.add(want.multi)
        assert (0 in want.junction_node.tolist()) == want.multi and len(want.path_start) >= 2
    assert answers == {True, False}


# ------------------------------------------------------------------ 4. many starts
N_BUBBLES = 4200


def test_more_junctions_than_a_scan_tile(eng):
    ref = ref_of("bubble chain", lambda: JS.bubble_chain(N_BUBBLES))
    build(eng, ref, "bubble chain")
    near, far = ref.found(4), ref.found(12)
    assert len(near.junction_node) == 2 * N_BUBBLES > 8192
    assert near.path_off[-1] != far.path_off[-1] and len(near.path_start) == 4 * N_BUBBLES < len(far.path_start)
    assert far.stops_per_start.max() == 3       # a search spans three bubbles
    same(eng.junction_paths(4), near, "bubble chain 4")
    same(eng.junction_paths(12), far, "bubble chain 12")


# ------------------------------------------------------------------ 5. live graphs
LIVE_DISTANCES = (6, 10)


def test_lists_made_from_a_filtered_graph(eng):
    lost_first, fell = 0, 0
    for seed in JS.SEEDS:
        ref = ref_of(("weighted", seed), lambda: JS.weighted_pairs(seed), seed)
        orc = ref.new_sweep()
        orc.filter(2, 2)
        eng.set_reads(*ref.tokens)
        eng.build(1)
        eng.filter(2, 2)
        compare_engine_to_sweep(eng, orc, ("filtered", seed))
        ea, na = orc.edges()["alive"], orc.nodes()["alive"]
        orc.close()
        assert 0 < int(ea.sum()) < len(ea)
        for d in LIVE_DISTANCES:
            same(eng.junction_paths(d), JS.search(ref.edges, ea, na, d), ("filtered", seed, d))
        a, b = JS.row_changes(ref.edges, ref.D, (ref.edges["alive"], ref.nodes["alive"]), (ea, na))
        lost_first, fell = lost_first + len(a), fell + len(b)
    assert lost_first > 0 and fell > 0


@pytest.mark.parametrize("patch", [True, False])
def test_lists_after_nodes_died(eng, monkeypatch, patch):
    """search (the lists exist), remove a seeded fifth of the nodes, search again: the lists are patched in place, or
    with AMG_NO_LADJ_PATCH=1 made again"""
    if not patch:
        monkeypatch.setenv("AMG_NO_LADJ_PATCH", "1")
    lost_first, fell = 0, 0
    for seed in JS.SEEDS:
        ref = ref_of(("weighted", seed), lambda: JS.weighted_pairs(seed), seed)
        build(eng, ref, ("weighted", seed))
        same(eng.junction_paths(10), ref.found(10), ("before", seed))
        victims = np.sort(np.random.default_rng(700 + seed).permutation(ref.D)[:ref.D // 5])
        eng.remove_nodes(victims)
        ea, na = JS.live_after(ref.edges, ref.D, dead_nodes=victims)
        assert np.array_equal(eng.nodes()["alive"], na) and np.array_equal(eng.edges()["alive"], ea)
        for d in LIVE_DISTANCES:
            same(eng.junction_paths(d), JS.search(ref.edges, ea, na, d), ("after", patch, seed, d))
        a, b = JS.row_changes(ref.edges, ref.D, (ref.edges["alive"], ref.nodes["alive"]), (ea, na))
        lost_first, fell = lost_first + len(a), fell + len(b)
    assert lost_first > 0 and fell > 0


# ------------------------------------------------------------------ 6. the step budget
def test_budget_on_its_boundary(eng, monkeypatch):
    ref = ref_of("layered", lambda: JS.layered(8, 3))
    build(eng, ref, "layered")
    want = ref.found(12)
    most = int(want.enters.max())
    assert most == sum(3 ** i for i in range(9)) and 10_000 > most > 9_000 and most < 1 << 24
    assert len(want.path_start) > 1000
    monkeypatch.setenv("AMG_TEST_BJ_STEPS", str(most))
    same(eng.junction_paths(12), want, "budget = the longest search")
    monkeypatch.setenv("AMG_TEST_BJ_STEPS", str(most - 1))
    sizes = (C.c_int64 * 4)()
    from amira_amd import _ffi
    _ffi.check(_ffi.lib.amg_junction_paths(eng._h, 12, sizes))
    assert list(sizes) == [len(want.junction_node), 0, 0, BJ_BUDGET]
    cut = eng.junction_paths(12)
    assert cut["flags"] == BJ_BUDGET and cut["path_off"].tolist() == [0] and len(cut["path_start"]) == 0
    assert len(cut["path_node"]) == 0 and len(cut["path_dir"]) == 0
    assert np.array_equal(cut["junction_node"], want.junction_node) and np.array_equal(cut["junction_dir"], want.junction_dir)
    monkeypatch.delenv("AMG_TEST_BJ_STEPS")
    same(eng.junction_paths(12), want, "no budget set")
    # beyond the bound and below it: never more than 2^24, at least 1
    monkeypatch.setenv("AMG_TEST_BJ_STEPS", str(1 << 40))
    same(eng.junction_paths(12), want, "budget above 2^24")
    monkeypatch.setenv("AMG_TEST_BJ_STEPS", "0")
    assert eng.junction_paths(12)["flags"] == BJ_BUDGET     # (one step: the start, and every start has a second node)


def test_budget_and_repeated_pair_set_both_bits(eng, monkeypatch):
    ref = ref_of(("repeated", 40, 0), lambda: JS.repeated_pairs(40, 0), 0)
    want = ref.found(10)
    assert want.multi and int(want.enters.max()) > 2 and int((want.enters == want.enters.max()).sum()) >= 1
    build(eng, ref, "repeated 40 0")
    monkeypatch.setenv("AMG_TEST_BJ_STEPS", str(int(want.enters.max()) - 1))
    cut = eng.junction_paths(10)
    assert cut["flags"] == BJ_MULTI | BJ_BUDGET and cut["path_off"].tolist() == [0]
    assert np.array_equal(cut["junction_node"], want.junction_node)
    monkeypatch.setenv("AMG_TEST_BJ_STEPS", str(int(want.enters.max())))
    same(eng.junction_paths(10), want, "repeated 40 0, budget = the longest search", BJ_MULTI)


# ------------------------------------------------------------------ 7. the caller
def test_graph_declines_where_the_reference_fails():
    from amira_amd import GeneMerGraph
    from amira_oracle import GeneMerGraph as Oracle
    shape = JS.repeated_pairs(40, 0)
    ref = ref_of(("repeated", 40, 0), lambda: shape, 0)
    assert ref.found(4).multi                   # (the graph asks for 4 k)
    reads = G.shape_reads(shape, 0)
    g = GeneMerGraph(reads, 1)
    try:
        found = g._engine.junction_paths(4)
        same(found, ref.found(4), "through the graph", BJ_MULTI)
        assert g._junction_paths_on_device() is None
        with pytest.raises(AttributeError):
            for junctions in g.identify_potential_bubble_starts().values():
                g.get_all_paths_between_junctions_in_component(junctions, 4, 1)
    finally:
        g.close()
    o = Oracle(reads, 1)
    with pytest.raises(AttributeError):
        for junctions in o.identify_potential_bubble_starts().values():
            o.get_all_paths_between_junctions_in_component(junctions, 4, 1)
