"""Constructed read sets on the boundary of the derived rebuild (amg_derive.hip) and the verdict the engine must reach
on each, for tests/test_derive_cases_cpu.py (the cases against the oracle alone) and tests/test_gpu_derive.py.

A case class is a function that returns (reads, k, procedure).  The procedure is the list of removals applied to the
engine and to the oracle between the build and the correction:

  ("filter", n, e)     filter_graph(n, e)
  ("clip", L)          remove_short_linear_paths(L)
  ("components", m)    remove_low_coverage_components(m)
  ("nodes", pick)      remove_node of every node hash pick(g) names on the oracle graph as it is then
  ("edges", pick)      remove_edge of every (directed) edge hash pick(g) names

CASES maps a name to (function, arguments, edge_died_alone, derivable): whether the procedure removes an edge whose two
nodes stay is a property of the procedure that the case states; `derivable` is what the class was built to be, which
the CPU test holds against predicted_derivable.

The read sets come from the `backbone` / `noisy` generators of tests/test_gpu_correct_limits.py: a genome of distinct
genes, noisy reads first (so the genome's gene-mers are first seen in THEM wherever they reach), then clean reads.  A
substituted gene one in from a read's end makes two gene-mers nobody else has at that end: a tip of two nodes of
coverage 1, which a tip clip or a coverage filter removes, and the read is cut there."""
import numpy as np

from test_gpu_correct_limits import backbone, noisy, positions_and_lengths  # noqa: F401  (generators: imported, not copied)


# ------------------------------------------------------------------ the rule
def predicted_derivable(g, edge_died_alone):
    """amg_derive.hip's header on oracle data, just before the oracle's correct_reads: the corrected reads make the
    graph at hand restricted to its live nodes when every read is kept whole, cut to one run of live windows or gone
    (no None between two nodes: nothing is re-threaded and no read keeps its genes around a dead window) and no edge
    was removed with both its nodes alive.  Reads nothing from the engine."""
    for nodes in g.get_readNodes().values():
        live = [i for i, h in enumerate(nodes) if h is not None]
        if live and live[-1] - live[0] + 1 != len(live):
            return False
    return not edge_died_alone


# ------------------------------------------------------------------ running a procedure
def build_orders(g):
    """engine ids of the oracle graph as built: node / edge id = position in first-seen order"""
    return {h: i for i, h in enumerate(g.get_nodes())}, {h: i for i, h in enumerate(g.get_edges())}


def apply_step(g, step, order, eorder, eng=None):
    """one removal on the oracle graph and, when given, on the engine (ids of the build: `order`, `eorder`); a clip
    returns (engine's removed ids, oracle's), both sorted"""
    what = step[0]
    if what == "filter":
        g.filter_graph(step[1], step[2])
        if eng is not None:
            eng.filter(step[1], step[2])
    elif what == "clip":
        want = sorted(order[h] for h in g.remove_short_linear_paths(step[1]))
        got = sorted(eng.remove_short_linear_paths(step[1]).tolist()) if eng is not None else want
        return got, want
    elif what == "components":
        g.remove_low_coverage_components(step[1])
        if eng is not None:
            eng.remove_low_coverage_components(step[1])
    elif what == "nodes":
        hashes = list(step[1](g))
        for h in hashes:
            g.remove_node(g.get_node_by_hash(h))
        if eng is not None:
            eng.remove_nodes([order[h] for h in hashes])
    elif what == "edges":
        hashes = list(step[1](g))
        for h in hashes:
            g.remove_edge(h)
        if eng is not None:
            eng.remove_edges([eorder[h] for h in hashes])
    else:
        raise ValueError(what)
    return None


def run_procedure(g, procedure, eng=None):
    order, eorder = build_orders(g)
    for step in procedure:
        r = apply_step(g, step, order, eorder, eng)
        if r is not None:
            assert r[0] == r[1], ("removed ids", step)


def leading_dead(nodes):
    """dead windows before the first live one (0 for a read whose windows are all dead)"""
    for i, h in enumerate(nodes):
        if h is not None:
            return i
    return 0


# ------------------------------------------------------------------ the classes
def end_cut(a, b, front=True, back=True):
    """a noisy read over genes a .. b-1 with a substituted gene one in from the chosen ends"""
    return dict(a=a, b=b, subs=((a + 1,) if front else ()) + ((b - 2,) if back else ()))


def identity():
    """nothing dies: a filter that removes nothing, a correction that corrects nothing"""
    reads = backbone(40, [dict(a=3, b=20), dict(a=15, b=40), dict(a=0, b=9)], n_clean=3)
    return reads, 3, [("filter", 1, 1)]


def circular():
    """nothing dies, and every read runs once round a circular genome and k + 1 genes on: its last two windows repeat
    its first two, so no gene-mer and no edge class is first seen in the last two windows of a read.  A derive at
    k + 2 — which the engine must not try — would find every first occurrence inside a window of that size, so none of
    its own checks would stop it"""
    k = 3
    genome = backbone(30, [], n_clean=1)["c000"]
    reads = {f"c{j:03d}": genome + genome[:k + 1] for j in range(3)}
    return reads, k, [("filter", 1, 1)]


def both_ends_cut(k=3, deep=False):
    """tips at the front, at the back and at both ends of noisy reads that are the FIRST to show the genome's
    gene-mers; a tip clip removes the tips.  deep (k = 3): also tips of four nodes, which the clip at k leaves and a
    clip at DEEP_CLIP takes (a second derivable correction after the first), and a substituted gene in the middle of
    a read (a bubble of coverage 1: no tip, but a filter(2, 1) later has the read re-threaded)"""
    spec = [end_cut(10, 34, back=False), end_cut(28, 52, front=False), end_cut(46, 66),
            dict(a=5, b=22), end_cut(20, 20 + k + 3, back=False), end_cut(40, 60)]
    extra = ()
    if deep:
        assert k == 3
        spec += [dict(a=12, b=40, subs=(13, 15)), dict(a=30, b=58, subs=(53, 55)), dict(a=8, b=36, subs=(22,)),
                 dict(a=36, b=64, subs=(37, 39, 59, 61))]
        extra = [[f"+y{i}" for i in range(10)]] * 2       # a component of its own, coverage 2, no tip
    reads = backbone(70, spec, n_clean=4, extra=extra)
    return reads, k, [("clip", k)]


DEEP_CLIP = 6


def front_reads_dropped(n_keep, k=3):
    """three reads of genes nobody else has come first and vanish under filter(2, 1); the first read that stays is cut at
    its front and is the first to show two of the genome's gene-mers; n_keep reads stay, all of k + 1 or k + 2 genes"""
    gone = [dict(a=0, b=k + 1, subs=tuple(range(k + 1))) for _ in range(3)]
    reads = backbone(k + 2, gone + [dict(a=0, b=k + 2, subs=(0,))], n_clean=n_keep - 1)
    return reads, k, [("filter", 2, 1)]


KEPT_READS = (63, 64, 65, 255, 256, 257)          # k_dv_windows: 64 reads to a wave, 256 to a workgroup
LONG_WINDOWS = (64, 65, 129, 200)


def long_reads():
    """reads that keep 64, 65, 129 and 200 windows between two clipped tips, each among short ones in its group of four
    kept reads"""
    k = 3
    spec = []
    for j, w in enumerate(LONG_WINDOWS):
        short = [end_cut(30 + 7 * j, 42 + 7 * j, back=False), dict(a=60 + j, b=66 + j), end_cut(80 + 5 * j, 90 + 5 * j)]
        long_ = end_cut(8 + j, 8 + j + w + 4 + k - 1)
        spec += short[:j % 4] + [long_] + short[j % 4:]
    reads = backbone(230, spec, n_clean=4)
    return reads, k, [("clip", k)]


def short_reads():
    """reads of fewer than k genes (no window: they never reach correct_reads) and of exactly k (one window: kept when
    it is the genome's, gone when nobody else has it), interleaved with longer ones"""
    k = 3
    reads = backbone(30, [dict(a=4, b=6), dict(a=4, b=7), dict(a=9, b=10), dict(a=10, b=13, subs=(11,)),
                          dict(a=2, b=12), dict(a=14, b=16), dict(a=20, b=23), end_cut(12, 24, back=False),
                          dict(a=25, b=27), dict(a=24, b=27, subs=(24,))], n_clean=3)
    return reads, k, [("filter", 2, 1)]


def self_loop_and_flip():
    """a gene k + 1 times in a row (two windows of one gene-mer: a self-loop) in three reads, the first of them behind
    a gene nobody else has; and a read through the genome on the reverse strand, first of all reads"""
    k = 3
    body = backbone(40, [end_cut(6, 24), end_cut(18, 38, front=False)], n_clean=3)
    genome = body["c000"]
    rev = [("-" if g[0] == "+" else "+") + g[1:] for g in reversed(genome[4:30])]
    reads = {"rev0": rev, "loop0": ["+zz"] + ["+rep"] * (k + 1), "loop1": ["+rep"] * (k + 1)}
    reads.update(body)
    reads["loop2"] = ["+rep"] * (k + 1) + ["+yy"]
    return reads, k, [("filter", 2, 1)]


def _coverage_one(g):
    return [h for h, n in g.get_nodes().items() if n.get_node_coverage() == 1]


def component_and_listed():
    """two reads of their own genes are a component of coverage 2 at most, removed as a component; the tips of the
    noisy reads are removed as listed nodes; no filter, no clip"""
    k = 3
    lone = [f"+y{i}" for i in range(9)]
    reads = backbone(50, [end_cut(5, 25), end_cut(20, 45, front=False), end_cut(30, 48, back=False)], n_clean=3,
                     extra=[lone, lone[2:8]])
    reads = {"e001": reads.pop("e001"), **reads}       # one of the component's reads first: read 0 vanishes
    return reads, k, [("components", 3), ("nodes", _coverage_one)]


def gap_rethreaded():
    """a substituted gene in the middle of a read: dead windows between live ones, and a path around them"""
    reads = backbone(40, [dict(a=5, b=30, subs=(17,)), dict(a=10, b=38)], n_clean=3)
    return reads, 3, [("filter", 2, 1)]


def dead_end_kept():
    """a read that lacks four genes: no path within 2k nodes around its dead windows, so it keeps its genes"""
    reads = backbone(60, [dict(a=0, b=44, cuts=[(20, 4)]), dict(a=30, b=55)], n_clean=5)
    return reads, 3, [("filter", 3, 1)]


def edge_threshold():
    """filter(1, 2): no node dies, the edges only one read walks die between two nodes that stay"""
    reads = backbone(30, [dict(a=3, b=12), dict(a=20, b=30)], n_clean=2,
                     extra=[["+g5", "+g6", "+g7", "+g20", "+g21", "+g22"]])
    return reads, 3, [("filter", 1, 2)]


def _first_edge(g):
    return [next(iter(g.get_edges()))]


def edge_removed():
    """remove_edge of one live directed edge"""
    reads = backbone(30, [dict(a=3, b=12), dict(a=20, b=30)], n_clean=2)
    return reads, 3, [("edges", _first_edge)]


def everything_dies():
    """a node threshold nothing reaches: no read is left"""
    reads = backbone(20, [dict(a=3, b=12)], n_clean=2)
    return reads, 3, [("filter", 10 ** 6, 1)]


# name -> (function, arguments, edge_died_alone, derivable)
CASES = {"identity": (identity, (), False, True),
         "circular": (circular, (), False, True),
         "both_ends_cut": (both_ends_cut, (), False, True),
         "both_ends_cut_k5": (both_ends_cut, (5,), False, True),
         "both_ends_cut_deep": (both_ends_cut, (3, True), False, True),
         "long_reads": (long_reads, (), False, True),
         "short_reads": (short_reads, (), False, True),
         "self_loop_and_flip": (self_loop_and_flip, (), False, True),
         "component_and_listed": (component_and_listed, (), False, True),
         "gap_rethreaded": (gap_rethreaded, (), False, False),
         "dead_end_kept": (dead_end_kept, (), False, False),
         "edge_threshold": (edge_threshold, (), True, False),
         "edge_removed": (edge_removed, (), True, False),
         "everything_dies": (everything_dies, (), False, True)}
for _n in KEPT_READS:
    CASES[f"front_reads_dropped_{_n}"] = (front_reads_dropped, (_n,), False, True)

# the engine's verdict is stated outright, not through the predicate, where the predicate is not what decides:
# an edge that died on its own (the flag amg_filter / amg_remove_edges raise), and no read left (derive_from_previous
# declines by its first line although the rule holds trivially)
NEVER_DERIVED = ("edge_threshold", "edge_removed", "everything_dies")


def case(name):
    fn, args, edge_died_alone, derivable = CASES[name]
    reads, k, procedure = fn(*args)
    return reads, k, procedure, edge_died_alone, derivable


def inputs(reads):
    """what the engine takes: vocabulary, tokens, offsets, read ids, flat positions, read lengths, and the oracle's
    position dict and fastq stand-in"""
    from amira_amd.tokens import tokenize
    from helpers import flat_positions
    pos, fq = positions_and_lengths(reads)
    vocab, toks, offs, read_ids = tokenize(reads)
    gs, ge = flat_positions(read_ids, reads, pos)
    rl = np.asarray([len(fq[r]["sequence"]) for r in read_ids], dtype=np.int64)
    return vocab, toks, offs, read_ids, gs, ge, rl, pos, fq
