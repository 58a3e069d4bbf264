"""The live adjacency of a graph of which a filter has left little (ensure_live_adj, amg_live_rows.hip).  What its rows
must be whichever way they are made: a live node without a live edge reads as empty, and nothing an older and larger
graph left in the row buffer — which outlives graphs — is ever acted on (today the build zeroes every row; a build that
writes the rows of live nodes only has to pass here unchanged).  Every walker of the rows runs on such graphs — the
re-threading search of correct_reads, tip clipping on the lists, k_lr_patch after more nodes died — against the
sequential C oracle (token_oracle.Sweep) after every stage.

Graphs as read sets at gene-mer size 1 (tests/graph_shapes.py: a prefix of D one-gene reads fixes the node ids, a read
of two genes is an edge), every gene on the + strand, plus reads of three genes (a, x, b) whose middle node x has
coverage 2 and dies in filter(3, 1): a None run between two live windows, which the correction re-threads along the
live rows of a."""
import numpy as np
import pytest

import graph_shapes as G
import token_oracle
from helpers import compare_corrected, compare_engine_to_sweep

pytestmark = pytest.mark.gpu


def sparse_case(D, seed, ends):
    """(tokens, read_offsets, two_v), parts.  Half the nodes are a spine (a chain in shuffled ids, every link three times:
    alive), with a tip of two nodes on its sixth node (three times: alive, clipped at min_length 3); `lone` has three
    one-gene reads and three links to nodes that die: alive without a live edge; every other node x is the middle of one
    read (spine[a], x, spine[a + 2]) and dies.  ends: "alive" — nodes 0 and D - 1 are spine nodes; "dead" — they are
    among the x; "lone" — node 0 is the lone node and D - 1 the tip's end."""
    rng = np.random.default_rng(seed)
    ids = [int(i) for i in rng.permutation(np.arange(1, D - 1))]
    n_spine = D // 2
    if ends == "alive":
        spine, rest = [0] + ids[:n_spine - 2] + [D - 1], ids[n_spine - 2:]
        lone, tip, dead = rest[0], rest[1:3], rest[3:]
    elif ends == "dead":
        spine, rest = ids[:n_spine], ids[n_spine:]
        lone, tip, dead = rest[0], rest[1:3], rest[3:] + [0, D - 1]
    else:
        spine, rest = ids[:n_spine], ids[n_spine:]
        lone, tip, dead = 0, [rest[0], D - 1], rest[1:]
    spine = [int(i) for i in rng.permutation(spine)]
    reads = []
    for a, b in zip(spine[:-1], spine[1:]):
        reads += [[a, b]] * 3
    reads += [[spine[5], tip[0]]] * 3 + [[tip[0], tip[1]]] * 3
    reads += [[lone]] * 3
    for j, x in enumerate(dead):                     # x: the prefix read and one more, coverage 2
        a = j % (n_spine - 2)
        if j < 3:
            reads.append([lone, x])                  # the lone node's links
        elif j == 3:
            reads.append([lone, x, spine[3]])        # a question that starts at the node without edges
        elif j % 2:
            reads.append([spine[a], x, spine[a + 2]])
        else:
            reads.append([spine[a + 2], x, spine[a]])
    order = rng.permutation(len(reads))
    reads = [reads[i] for i in order]
    V = D
    toks = np.concatenate([V + np.arange(V), V + np.concatenate([np.asarray(r) for r in reads])]).astype(np.int32)
    lens = np.concatenate([np.ones(V, np.int64), np.asarray([len(r) for r in reads], np.int64)])
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return (toks, offs, 2 * V), {"spine": spine, "tip": tip, "lone": lone, "dead": dead}


@pytest.fixture(scope="module")
def eng():
    from amira_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def begin(eng, tokens):
    eng.set_reads(*tokens)
    orc = token_oracle.Sweep(*tokens)
    eng.build(1)
    orc.build(1)
    compare_engine_to_sweep(eng, orc, "build")
    return orc


def filter_both(eng, orc, m=3):
    eng.filter(m, 1)
    orc.filter(m, 1)
    compare_engine_to_sweep(eng, orc, "filter")


def clip_both(eng, orc, min_length):
    got, want = eng.remove_short_linear_paths(min_length), orc.remove_short_linear_paths(min_length)
    assert sorted(got.tolist()) == sorted(want.tolist())
    compare_engine_to_sweep(eng, orc, "clip")
    return len(want)


def check_parts(orc, parts, D):
    """the graph after the filter is what the case says: the spine, the tip and the lone node alive, the lone node
    without a live edge, everything else dead"""
    n, e = orc.nodes(), orc.edges()
    alive = n["alive"] != 0
    want = np.zeros(D, bool)
    want[parts["spine"] + parts["tip"] + [parts["lone"]]] = True
    assert np.array_equal(alive, want)
    live_e = e["alive"] != 0
    assert live_e.any() and not (live_e & ((e["src"] == parts["lone"]) | (e["tgt"] == parts["lone"]))).any()


@pytest.mark.parametrize("ends", ["alive", "dead", "lone"])
@pytest.mark.parametrize("D", [41, 1030])
def test_rows_after_a_filter(eng, D, ends):
    """filter -> correct_reads: a live node with no live edge (asked as the start of a path), node 0 and the last node
    alive, dead, or the node without edges; D = 1 030: several workgroups of the row kernels, D mod 4 = 2 — the scalar
    tail of the four-nodes-a-thread kernels"""
    tokens, parts = sparse_case(D, 5 + D, ends)
    orc = begin(eng, tokens)
    filter_both(eng, orc)
    check_parts(orc, parts, D)
    out = compare_corrected(eng, orc, False, "correct")
    assert out["changed"].any()
    # tip clipping on the lists the correction has made
    assert clip_both(eng, orc, 3) >= 2
    compare_corrected(eng, orc, False, "correct after the clip")


@pytest.mark.parametrize("first_path", [3, 1])
def test_paths_of_three_nodes_among_dead_ones(eng, monkeypatch, first_path):
    """graph_shapes.triples at 257 nodes, three paths in ten given three times: filter(4, 1) leaves those paths (ends 4,
    middle 7) and kills the others and the two nodes no read joins (255, 256: the last node is dead); node 0 is alive
    or dead with its path.  Lists made by the clip itself (AMG_CLIP_LISTS=1), which removes every live path's two ends"""
    rng = np.random.default_rng(77)
    times = np.where(rng.random(257 // 3) < 0.3, 3, 1)
    times[0] = first_path
    shape = G.triples(257, 0, times)
    orc = begin(eng, G.as_tokens(shape.D, shape.pairs, 3, np.ones((len(shape.pairs), 2), np.int64)))
    filter_both(eng, orc, 4)
    alive = orc.nodes()["alive"] != 0
    assert alive[0] == (first_path == 3) and not alive[256] and 0 < alive.sum() < 257
    compare_corrected(eng, orc, False, "correct")
    monkeypatch.setenv("AMG_CLIP_LISTS", "1")
    clip_both(eng, orc, 2)
    compare_corrected(eng, orc, False, "correct after the clip")


def test_all_nodes_dead(eng, monkeypatch):
    """filter(50, 1) leaves nothing: correct_reads drops every read; lists of no live node and no live edge are made
    (AMG_CLIP_LISTS=1: the clip walks lists, not its row summary) and walked"""
    tokens, _ = sparse_case(41, 46, "alive")
    orc = begin(eng, tokens)
    filter_both(eng, orc, 50)
    assert orc.counts()["n_live_nodes"] == 0
    assert compare_corrected(eng, orc, False, "correct")["read_offsets"].tolist() == [0]
    monkeypatch.setenv("AMG_CLIP_LISTS", "1")
    assert clip_both(eng, orc, 3) == 0


@pytest.mark.parametrize("ends", ["alive", "dead"])
def test_rows_patched_after_more_nodes_died(eng, ends):
    """filter -> correct_reads (lists made) -> tip clipping (nodes die: the lists are behind) -> correct_reads: k_lr_patch
    brings the rows up to date in place"""
    D = 1030
    tokens, parts = sparse_case(D, 5 + D, ends)
    orc = begin(eng, tokens)
    filter_both(eng, orc)
    compare_corrected(eng, orc, False, "correct")
    assert clip_both(eng, orc, 3) >= 2
    compare_corrected(eng, orc, False, "correct on patched rows")
    eng.remove_low_coverage_components(8)
    orc.remove_low_coverage_components(8)
    compare_engine_to_sweep(eng, orc, "component filter")
    compare_corrected(eng, orc, False, "correct on rows patched twice")


@pytest.mark.parametrize("lists_first", [True, False])
def test_stale_rows_of_a_larger_graph(eng, monkeypatch, lists_first):
    """a graph of 41 nodes after one of 820 on the same engine: the row buffer still holds the larger graph's rows,
    offsets and all, wherever the smaller graph's build does not write.  Tip clipping on the lists (made by a
    correction first, or by the clip itself with AMG_CLIP_LISTS=1) and the correction after it must not see them"""
    big, _ = sparse_case(820, 825, "alive")
    orc = begin(eng, big)
    filter_both(eng, orc)
    compare_corrected(eng, orc, False, "large graph")
    assert clip_both(eng, orc, 3) >= 2
    compare_corrected(eng, orc, False, "large graph, patched")
    small, parts = sparse_case(41, 46, "dead")
    orc = begin(eng, small)
    filter_both(eng, orc)
    check_parts(orc, parts, 41)
    if lists_first:
        compare_corrected(eng, orc, False, "small graph")
    else:
        monkeypatch.setenv("AMG_CLIP_LISTS", "1")
    assert clip_both(eng, orc, 3) >= 2
    compare_corrected(eng, orc, False, "small graph after the clip")
