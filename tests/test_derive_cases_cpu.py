"""The case set of tests/derive_cases.py against the oracle alone: every class has the property it was built for,
predicted_derivable says what the class was built to be, and for the derivable classes the theorem the derived rebuild
(amg_derive.hip) rests on holds on oracle data — the graph of the corrected reads IS the graph before the correction
restricted to its live nodes.  A class that fails here is wrong, not the engine."""
import numpy as np
import pytest

import derive_cases as DC
from helpers import oracle_arrays


class Run:
    """one case through the oracle: the graph after the procedure (before correct_reads), the verdict, the corrected
    reads and their graph"""

    def __init__(self, name):
        from amira_oracle import GeneMerGraph
        self.name = name
        self.reads, self.k, self.procedure, self.edge_died_alone, self.derivable = DC.case(name)
        (self.vocab, self.toks, self.offs, self.read_ids, _, _, _, pos, fq) = DC.inputs(self.reads)
        g = GeneMerGraph(self.reads, self.k, {r: list(v) for r, v in pos.items()})
        self.n_built = (len(g.get_nodes()), len(g.get_edges()))
        self.first_dirs_built = [n.get_geneMer().get_geneMerDirection() for n in g.get_nodes().values()]
        self.self_loops_built = [h for h, e in g.get_edges().items() if e.get_sourceNode() == e.get_targetNode()]
        DC.run_procedure(g, self.procedure)
        self.g = g
        self.read_nodes = {r: list(v) for r, v in g.get_readNodes().items()}
        self.predicted = DC.predicted_derivable(g, self.edge_died_alone)
        self.before = oracle_arrays(g, self.vocab, self.read_ids, self.offs, self.k)
        self.r2, self.p2 = g.correct_reads(fq)
        self.g2 = GeneMerGraph(self.r2, self.k, self.p2)

    def cut_reads(self):
        """{read: (dead windows in front, dead windows behind)} of the reads that stay and lost some"""
        out = {}
        for r, nodes in self.read_nodes.items():
            live = [i for i, h in enumerate(nodes) if h is not None]
            if live and len(live) < len(nodes):
                out[r] = (live[0], len(nodes) - 1 - live[-1])
        return out


_RUNS = {}


def run_of(name):
    if name not in _RUNS:
        _RUNS[name] = Run(name)
    return _RUNS[name]


CLASSES = ("identity", "circular", "both_ends_cut", "front_reads_dropped", "long_reads", "short_reads", "self_loop_and_flip",
           "component_and_listed", "gap_rethreaded", "dead_end_kept", "edge_threshold", "edge_removed",
           "everything_dies")


def test_every_class_is_present():
    for c in CLASSES:
        assert any(n == c or n.startswith(c + "_") for n in DC.CASES), c
    for n in DC.KEPT_READS:
        assert f"front_reads_dropped_{n}" in DC.CASES
    for name in DC.CASES:
        reads, k, procedure, _, _ = DC.case(name)
        assert 0 < len(reads) <= 300 and max(len(v) for v in reads.values()) <= 230 and k >= 1, name


@pytest.mark.parametrize("name", sorted(DC.CASES))
def test_predicate_says_what_the_class_was_built_for(name):
    r = run_of(name)
    assert r.predicted == r.derivable, name


@pytest.mark.parametrize("name", sorted(n for n, c in DC.CASES.items() if c[3]))
def test_corrected_reads_make_the_live_part_of_the_graph(name):
    """GeneMerGraph(corrected reads) == the graph before the correction restricted to its live nodes: tokens,
    coverages, first directions, edge endpoints, directions and coverages, list orders, per-read node lists"""
    r = run_of(name)
    ids2 = list(r.r2)
    offs2 = np.concatenate([[0], np.cumsum([len(r.r2[x]) for x in ids2])]).astype(np.int64)
    after = oracle_arrays(r.g2, r.vocab, ids2, offs2, r.k)
    for key in ("tokens", "coverage", "first_dir", "src", "tgt", "sdir", "tdir", "ecov"):
        assert np.array_equal(r.before[key], after[key]), (name, key)
    assert r.before["adj"] == after["adj"], name
    # per read: the live windows of the old read, in order, are the windows of the new one; reads without one are gone
    ridx = {x: i for i, x in enumerate(r.read_ids)}
    kept = []
    for rid in r.read_ids:
        a, b = int(r.offs[ridx[rid]]), int(r.offs[ridx[rid] + 1])
        n_win = max(b - a - r.k + 1, 0)
        old = [int(x) for x in r.before["tok_node"][a:a + n_win] if x >= 0]
        if not old:
            assert rid not in r.r2, (name, rid)
            continue
        kept.append(rid)
        j = ids2.index(rid)
        a2 = int(offs2[j])
        new = after["tok_node"][a2:a2 + len(r.r2[rid]) - r.k + 1]
        assert old == new.tolist(), (name, rid)
        old_d = [int(d) for x, d in zip(r.before["tok_node"][a:a + n_win], r.before["tok_dir"][a:a + n_win]) if x >= 0]
        assert old_d == after["tok_dir"][a2:a2 + len(new)].tolist(), (name, rid)
    assert kept == ids2, name
    want_reads = [[kept.index(r.read_ids[i]) for i in row] for row in r.before["node_reads"]]
    assert want_reads == after["node_reads"], name


# ------------------------------------------------------------------ the defining property of every class
def test_identity():
    r = run_of("identity")
    assert (len(r.g.get_nodes()), len(r.g.get_edges())) == r.n_built and not r.cut_reads()
    assert r.r2 == r.reads and not r.g.get_reads_to_correct()


def test_circular():
    r = run_of("circular")
    assert r.r2 == r.reads and not r.cut_reads()
    nodes, pairs = first_occurrences(r)
    for first in (nodes, pairs):
        assert all(i + (r.k + 2) <= len(r.reads[rid]) for rid, i in first.values())   # inside a window of k + 2 genes
    assert len(nodes) < len(next(iter(r.read_nodes.values())))                       # the read meets a node twice


def first_occurrences(r):
    """(read, window) of the first occurrence of every live node and of every live pair of adjacent nodes"""
    nodes, pairs = {}, {}
    for rid, row in r.read_nodes.items():
        for i, h in enumerate(row):
            if h is None:
                continue
            nodes.setdefault(h, (rid, i))
            if i + 1 < len(row) and row[i + 1] is not None:
                pairs.setdefault(frozenset((h, row[i + 1])), (rid, i))
    return nodes, pairs


@pytest.mark.parametrize("name", ["both_ends_cut", "both_ends_cut_k5", "both_ends_cut_deep"])
def test_both_ends_cut(name):
    r = run_of(name)
    cuts = r.cut_reads()
    assert any(f > 0 and b == 0 for f, b in cuts.values()), "a read cut at the front only"
    assert any(f == 0 and b > 0 for f, b in cuts.values()), "a read cut at the back only"
    assert any(f > 0 and b > 0 for f, b in cuts.values()), "a read cut at both ends"
    assert len(r.r2) == len(r.reads)                      # nobody vanishes here
    nodes, pairs = first_occurrences(r)
    for what, first in (("node", nodes), ("edge class", pairs)):
        assert any(rid in cuts and cuts[rid][0] > 0 and i - cuts[rid][0] > 0 for rid, i in first.values()), \
            f"a {what} first seen at a nonzero offset of a read cut at its front"


def test_both_ends_cut_deep_second_stage():
    """the deep variant after its first correction: a clip at DEEP_CLIP cuts reads again and is derivable again (a
    second derived rebuild in a row); filter(2, 1) instead leaves a read with dead windows between live ones"""
    from amira_oracle import GeneMerGraph
    r = run_of("both_ends_cut_deep")
    for step, derivable in ((("clip", DC.DEEP_CLIP), True), (("filter", 2, 1), False)):
        g = GeneMerGraph(r.r2, r.k, {x: list(v) for x, v in r.p2.items()})
        n0 = len(g.get_nodes())
        DC.run_procedure(g, [step])
        assert len(g.get_nodes()) < n0
        rows = g.get_readNodes()
        assert sum(1 for row in rows.values() if row[0] is None or row[-1] is None) >= 3
        assert DC.predicted_derivable(g, False) == derivable, step


@pytest.mark.parametrize("n_keep", DC.KEPT_READS)
def test_front_reads_dropped(n_keep):
    r = run_of(f"front_reads_dropped_{n_keep}")
    assert len(r.r2) == n_keep
    assert list(r.reads)[:3] == [x for x in list(r.reads)[:3] if x not in r.r2], "reads 0 .. 2 vanish"
    first = next(iter(r.r2))
    assert first != next(iter(r.reads)) and first == list(r.reads)[3]
    cuts = r.cut_reads()
    assert cuts[first][0] > 0                              # the first read that stays is cut at its front ...
    nodes, _ = first_occurrences(r)
    assert any(rid == first and i - cuts[first][0] > 0 for rid, i in nodes.values())   # ... and shows a node first
    assert max(len(v) for v in r.reads.values()) <= r.k + 2


def test_long_reads():
    r = run_of("long_reads")
    ids2 = list(r.r2)
    cuts = r.cut_reads()
    found = {}
    for j, rid in enumerate(ids2):
        w = len(r.r2[rid]) - r.k + 1
        if w in DC.LONG_WINDOWS and rid in cuts and cuts[rid][0] > 0 and cuts[rid][1] > 0:
            group = ids2[j - j % 4: j - j % 4 + 4]
            assert any(len(r.r2[x]) - r.k + 1 < 16 for x in group), (rid, "a short read in its group of four")
            found[w] = j % 4
    assert sorted(found) == sorted(DC.LONG_WINDOWS)
    assert len(set(found.values())) > 1                    # not always the same place of the four


def test_short_reads():
    r = run_of("short_reads")
    ids = list(r.reads)
    short = [i for i, x in enumerate(ids) if len(r.reads[x]) < r.k]
    exact = [i for i, x in enumerate(ids) if len(r.reads[x]) == r.k]
    assert len(short) >= 3 and len(exact) >= 3
    assert set(ids[i] for i in short) == set(r.g.get_short_read_annotations())
    assert all(ids[i] not in r.r2 for i in short)
    assert any(ids[i] in r.r2 for i in exact) and any(ids[i] not in r.r2 for i in exact)
    order = sorted(short + exact)
    assert any(a in short and b in exact for a, b in zip(order, order[1:]))
    assert any(a in exact and b in short for a, b in zip(order, order[1:]))


def test_self_loop_and_flip():
    r = run_of("self_loop_and_flip")
    loops = [h for h, e in r.g.get_edges().items() if e.get_sourceNode() == e.get_targetNode()]
    assert len(loops) == 1 and loops == r.self_loops_built          # one directed edge, and it lives
    assert -1 in [n.get_geneMer().get_geneMerDirection() for n in r.g.get_nodes().values()]
    assert 1 in [n.get_geneMer().get_geneMerDirection() for n in r.g.get_nodes().values()]
    assert {1, -1} <= set(r.before["sdir"].tolist()) and {1, -1} <= set(r.before["tdir"].tolist())
    # the reverse-strand read walks the genome's nodes the other way round than the clean reads do
    rev, clean = r.read_nodes["rev0"], r.read_nodes["c000"]
    shared = [h for h in rev if h is not None and h in clean]
    assert len(shared) > 10 and [clean.index(h) for h in shared] == sorted((clean.index(h) for h in shared), reverse=True)
    assert r.cut_reads()["loop0"] == (1, 0) and r.cut_reads()["loop2"] == (0, 1)


def test_component_and_listed():
    r = run_of("component_and_listed")
    assert [s[0] for s in r.procedure] == ["components", "nodes"]
    assert "e000" not in r.r2 and "e001" not in r.r2 and next(iter(r.reads)) == "e001"
    cuts = r.cut_reads()
    assert cuts and all(x.startswith("n") for x in cuts)
    assert len(r.g.get_nodes()) < r.n_built[0]


def gaps(r):
    return {rid for rid, row in r.read_nodes.items()
            if any(row[i] is None and any(row[:i]) and any(row[i + 1:]) for i in range(len(row)))}


def test_gap_rethreaded():
    r = run_of("gap_rethreaded")
    assert gaps(r) == {"n000"}
    assert r.r2["n000"] == r.reads["c000"][5:30] and r.r2["n000"] != r.reads["n000"]


def test_dead_end_kept():
    r = run_of("dead_end_kept")
    assert gaps(r) == {"n000"}
    assert r.r2["n000"] == r.reads["n000"]                 # genes kept around the dead windows


@pytest.mark.parametrize("name", ["edge_threshold", "edge_removed"])
def test_an_edge_dies_between_two_nodes_that_stay(name):
    r = run_of(name)
    assert r.edge_died_alone
    assert len(r.g.get_nodes()) == r.n_built[0] and len(r.g.get_edges()) < r.n_built[1]
    assert not gaps(r) and not r.cut_reads() and r.r2 == r.reads
    # the graph of the (unchanged) reads has the edge again: the live part of the graph at hand is NOT that graph
    assert len(r.g2.get_edges()) == r.n_built[1]


def test_everything_dies():
    r = run_of("everything_dies")
    assert not r.g.get_nodes() and not r.r2
    assert "everything_dies" in DC.NEVER_DERIVED
