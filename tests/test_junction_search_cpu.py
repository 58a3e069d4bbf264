"""CPU: what gives tests/junction_search.py its standing as the reference of tests/test_gpu_junction_search.py.

On every family of graphs of that file, at its smallest size, junction_search.search on the C oracle's edge arrays
(token_oracle.Sweep) is held to the Python oracle (amira_oracle.GeneMerGraph on the same reads as strings, node n
holding gene n): the junction lists, the paths per (start, stop) pair as lists and in order, the canonical forms per
component, and `multi` against the AttributeError the oracle raises when it asks for THE edge between two nodes that
have several.  The conditions that keep the random families from going vacuous are computed from the reference alone."""
import numpy as np
import pytest

import graph_shapes as G
import junction_search as JS
import token_oracle


class Case:
    """one graph: the C oracle's arrays, the Python oracle's graph, and the node ids of its hashes"""

    def __init__(self, shape, seed):
        from amira_oracle import GeneMerGraph
        self.shape, self.D = shape, shape.D
        s = token_oracle.Sweep(*G.shape_tokens(shape, seed))
        s.build(1)
        self.edges, self.nodes = s.edges(), s.nodes()
        s.close()
        assert np.array_equal(self.nodes["tokens"][:, 0], self.D - 1 - np.arange(self.D))   # node n holds gene n
        self.g = g = GeneMerGraph(G.shape_reads(shape, seed), 1)
        self.hash_of = {}
        for node in g.all_nodes():
            (gene,) = [x.get_name() for x in node.get_canonical_geneMer()]
            self.hash_of[int(gene[1:])] = node.__hash__()
        assert sorted(self.hash_of) == list(range(self.D))
        self.component, _ = G.labels(shape.D, shape.pairs)

    def search(self, distance):
        return JS.search(self.edges, self.edges["alive"], self.nodes["alive"], distance)

    def oracle_sets(self, distance):
        """{component: the oracle's set of canonical paths}, or None where it raises AttributeError"""
        try:
            return {c: set(self.g.get_all_paths_between_junctions_in_component(junctions, distance, 1))
                    for c, junctions in self.g.identify_potential_bubble_starts().items()}
        except AttributeError:
            return None


def _canonical(p):
    return tuple(sorted([p, [(h, -d) for h, d in reversed(p)]])[0])


def check(case, distance, found=None):
    """everything the oracle can say about the search at this distance; returns (found, kept paths)"""
    g, h = case.g, case.hash_of
    found = case.search(distance) if found is None else found
    junctions = [(h[n], s) for n, s in zip(found.junction_node.tolist(), found.junction_dir.tolist())]
    # the junction lists, by component and in order
    starts = g.identify_potential_bubble_starts()
    by_component = {}
    for (n, s), j in zip(zip(found.junction_node.tolist(), found.junction_dir.tolist()), junctions):
        by_component.setdefault(int(case.component[n]), []).append(j)
    assert by_component == starts
    sets = case.oracle_sets(distance)
    assert found.multi == (sets is None), (distance, found.multi)
    if sets is None:
        return found, None
    # the paths per (start, stop) pair: the valid ones, as lists and in order
    got = {}
    for j, p in JS.paths_of(found):
        got.setdefault(junctions[j], []).append([(h[n], s) for n, s in p])
    want = {}
    for component_junctions in starts.values():
        for start in component_junctions:
            for stop in component_junctions:
                if start[0] == stop[0]:
                    continue
                paths = g.new_find_paths_between_nodes(start[0], stop[0], distance, start[1])
                valid = [p for p in paths if p[0] == start
                         and (p[-1][0], g.get_direction_between_two_nodes(p[-2][0], p[-1][0])) == stop]
                if len(valid) > 1:
                    want.setdefault(start, []).extend(valid)
    assert got == want
    # the canonical forms per component
    for component, component_junctions in starts.items():
        mine = {_canonical(p) for start, ps in got.items() if start in component_junctions for p in ps}
        assert mine == sets[component]
    return found, sum(len(x) for x in got.values())


# ------------------------------------------------------------------ the fixed families
def test_ladder_depth_64():
    shape, S, T = JS.ladder()
    case = Case(shape, 1)
    for d in (2, 3, 20, 21, 63):
        found, n = check(case, d)
        assert n == 0 and len(found.junction_node) == 2
    found, n = check(case, 64)
    assert n == 4 and np.diff(found.path_off).tolist() == [64] * 4    # two paths, met from either end
    assert {_canonical(p) for _, p in JS.paths_of(found)}.__len__() == 2
    # (a gene on '+' is its node taken in direction -1: the canonical gene-mer of size 1 is the '-' token)
    assert found.junction_node.tolist() == [S, T] and found.junction_dir.tolist() == [-1, 1]


def test_ladder_on_random_strands_is_the_same_ladder():
    plain, S, T = JS.ladder()
    turned, _, _ = JS.ladder(strand_seed=5)
    assert 0 < int((turned.strands < 0).sum()) < turned.strands.size
    a, b = Case(plain, 1), Case(turned, 1)
    for d in (21, 63, 64):
        fa, na = check(a, d)
        fb, nb = check(b, d)
        assert na == nb and np.array_equal(fa.junction_node, fb.junction_node)
        assert np.array_equal(fa.enters, fb.enters) and np.array_equal(np.diff(fa.path_off), np.diff(fb.path_off))
    assert len(set(fb.path_dir.tolist())) == 2 and len(set(fa.path_dir[:64].tolist())) == 1


def test_uneven_ladder():
    shape, S, T = JS.ladder(61, 62)
    case = Case(shape, 1)
    assert check(case, 62)[1] == 0
    found, n = check(case, 63)
    assert n == 0 and found.enters.max() > 63       # one record a start: no bubble
    found, n = check(case, 64)
    assert n == 4 and sorted(np.diff(found.path_off).tolist()) == [63, 63, 64, 64]


@pytest.mark.parametrize("distance", [4, 12])
def test_bubble_chain(distance):
    case = Case(JS.bubble_chain(6), 1)
    found, n = check(case, distance)
    assert len(found.junction_node) == 12
    assert n == (12 * 2 if distance == 4 else 2 * (4 * 14 + 6 + 2))   # 2 + 4 + 8 from a start with three bubbles ahead


def test_layered():
    case = Case(JS.layered(4, 3), 1)
    found, n = check(case, 6)
    assert found.enters.max() == 1 + 3 + 9 + 27 + 81 and n > 0
    whole = JS.search(*_arrays(JS.layered(8, 3)), 10)
    assert whole.enters.max() == sum(3 ** i for i in range(9)) < 1 << 24


def _arrays(shape, seed=1):
    s = token_oracle.Sweep(*G.shape_tokens(shape, seed))
    s.build(1)
    e, n = s.edges(), s.nodes()
    s.close()
    return e, e["alive"], n["alive"]


# ------------------------------------------------------------------ the random families
_SEEN = {"both_sides": 0, "other_side_only": 0, "three_stops": 0, "loop_junctions": 0, "kept": []}


@pytest.mark.parametrize("D,distance", JS.DISTINCT)
def test_distinct_pairs(D, distance):
    for seed in JS.SEEDS:
        case = Case(JS.distinct_pairs(D, seed), seed)
        found, n = check(case, distance)
        assert not found.multi and n is not None
        assert 20 <= len(found.junction_node) <= 60
        _SEEN["kept"].append(n)
        _SEEN["both_sides"] += int((np.diff(found.junction_node) == 0).sum())
        _SEEN["other_side_only"] += found.other_side_only
        _SEEN["three_stops"] += int((found.stops_per_start >= 3).sum())
        _SEEN["loop_junctions"] += len(JS.self_loop_junctions(case.edges, case.edges["alive"], case.nodes["alive"]))


def test_distinct_pairs_are_not_vacuous():
    """(after the tests above, in file order; alone it computes what it needs from the reference)"""
    if not _SEEN["kept"]:
        for D, distance in JS.DISTINCT:
            for seed in JS.SEEDS:
                e, ea, na = _arrays(JS.distinct_pairs(D, seed), seed)
                found = JS.search(e, ea, na, distance)
                _SEEN["kept"].append(len(found.path_start))
                _SEEN["both_sides"] += int((np.diff(found.junction_node) == 0).sum())
                _SEEN["other_side_only"] += found.other_side_only
                _SEEN["three_stops"] += int((found.stops_per_start >= 3).sum())
                _SEEN["loop_junctions"] += len(JS.self_loop_junctions(e, ea, na))
    print(_SEEN)
    assert _SEEN["both_sides"] > 0          # a start that is a junction on both sides
    assert _SEEN["other_side_only"] > 0     # a node entered through its side that is no junction, the other one is
    assert _SEEN["three_stops"] > 0         # a search that crosses junctions and records several stops
    assert _SEEN["loop_junctions"] > 0      # a row that is a junction only through a self-loop
    assert max(_SEEN["kept"]) > 100 and min(_SEEN["kept"]) < max(_SEEN["kept"])


def test_repeated_pairs_follow_the_oracles_exception():
    """`multi` against the oracle's AttributeError, either way.  On a graph built from reads it cannot depend on the
    distance: the two edges between a and b share a row at one of the two, say a (junction_search.random_pairs), so
    (a, that side) is a start whose search enters b as its second node at every distance from 2 on, and b is a
    junction or it is not.  (true at one distance and false at the one below needs an edge without its twin.)  So the
    answer of the distance below is asserted to be the same, and to be the oracle's."""
    multi = {True: 0, False: 0}
    for D, distance in JS.DISTINCT:
        for seed in JS.SEEDS:
            case = Case(JS.repeated_pairs(D, seed), seed)
            found, _ = check(case, distance)
            multi[found.multi] += 1
            if distance > 2:
                below, _ = check(case, distance - 1)
                assert below.multi == found.multi
    print(multi)
    assert multi[True] > 0 and multi[False] > 0


def test_two_edges_to_a_dead_end():
    answers = set()
    for turn in (0, 1):
        case = Case(JS.dead_end_pair(turn), 1)
        for d in (2, 3, 4):
            found, _ = check(case, d)
        answers.add(found.multi)
        assert (0 in found.junction_node.tolist()) == found.multi
    assert answers == {True, False}


def test_liveness_after_removals():
    e = {"src": np.array([0, 1, 1, 2]), "tgt": np.array([1, 0, 2, 1]), "sdir": np.array([1, -1, 1, -1]),
         "tdir": np.array([1, -1, 1, -1])}
    ea, na = JS.live_after(e, 3, dead_nodes=[2])
    assert ea.tolist() == [1, 1, 0, 0] and na.tolist() == [1, 1, 0]
    ea, na = JS.live_after(e, 3, dead_edges=[0])
    assert ea.tolist() == [0, 1, 1, 1] and na.tolist() == [1, 1, 1]
    off, ids = JS.live_rows(e, ea, 3)
    assert off.tolist() == [0, 0, 0, 1, 2, 2, 3] and ids.tolist() == [2, 1, 3]
