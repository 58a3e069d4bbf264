"""Tip clipping on the one-pass row summary (k_row_tickets, amg_live_rows.hip; RView, amg_rows.h) against the CPU oracle, and against
the walk over the live lists (AMG_CLIP_LISTS=1), which must agree with it to the last id.

A case is a read set, a gene-mer size and a list of steps applied to the engine and to the oracle after the build:

  ("clip", L[, genes])   remove_short_linear_paths(L), nodes that hold one of `genes` protected
  ("filter", n, e)       filter_graph(n, e)
  ("edges", pick)        remove_edge of every directed edge hash pick(g) names
  ("nodes", pick)        remove_node of every node hash pick(g) names
  ("correct"[, True])    correct_reads; True: the oracle corrects a second graph brought to the same state, so that
                         the first one can go on (the reference's correct_reads rewrites the positions it was given)
  ("rebuild",)           adopt the corrected reads and build: the derived rebuild where the correction allows it

The oracle's side of a case (`expected`) is computed once and shared by the two engine runs.  After every step the
engine equals the oracle (removed ids, live arrays, corrected reads); what the two runs left (removed ids, live
arrays, corrected arrays) is compared array by array."""
import functools

import numpy as np
import pytest

import procedures as P
from helpers import check_corrected, compare_engine_to_oracle, flat_positions, live_arrays, oracle_arrays

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from amira_amd import Engine
    e = Engine(0)
    yield e
    e.close()


# ------------------------------------------------------------------ the oracle's side
def _inputs(reads):
    from amira_amd import synth
    return synth.positions_for(reads), P.FakeFastq(synth.fake_fastq_lengths(reads))


def _graph(reads, pos, k):
    from amira_oracle import GeneMerGraph
    return GeneMerGraph(reads, k, {r: [list(p) for p in v] for r, v in pos.items()})


def _orders(g):
    return {h: i for i, h in enumerate(g.get_nodes())}, {h: i for i, h in enumerate(g.get_edges())}


def _remove(g, step, order=None, eorder=None):
    """a "filter" / "edges" / "nodes" step on an oracle graph; with the orders taken at its build: the engine's ids of
    what was picked (the oracle deletes what it removes, so positions in its dicts shift)"""
    if step[0] == "filter":
        g.filter_graph(step[1], step[2])
        return None
    hashes = list(step[1](g))
    for h in hashes:
        if step[0] == "edges":
            g.remove_edge(h)
        else:
            g.remove_node(g.get_node_by_hash(h))
    ids = eorder if step[0] == "edges" else order
    return [ids[h] for h in hashes] if ids is not None else None


def expected(reads, k, steps, check=None):
    """the oracle's record of every step, in the engine's conventions.  Node / edge ids are those of the build the
    step works on: the oracle deletes what it removes, so positions in its dicts are translated through the orders
    taken right after each build."""
    from amira_amd import tokenize
    pos, fq = _inputs(reads)
    vocab, toks, offs, read_ids = tokenize(reads)
    g = _graph(reads, pos, k)
    cur = {"reads": reads, "pos": pos, "ids": read_ids, "offs": offs, "done": []}
    order, eorder = _orders(g)
    out = [("build", oracle_arrays(g, vocab, read_ids, offs, k))]
    corrected = None
    for step in steps:
        what = step[0]
        if what == "clip":
            genes = list(step[2]) if len(step) > 2 else []
            protect = None
            if genes:
                protect = np.zeros(len(order), np.uint8)
                protect[[order[h] for h in g.get_AMR_nodes(genes)]] = 1
            before = dict(g.get_nodes())
            removed = g.remove_short_linear_paths(step[1], genes) if genes else g.remove_short_linear_paths(step[1])
            if check is not None:
                check(before, g, removed)
            out.append(("clip", step[1], protect, sorted(order[h] for h in removed),
                        oracle_arrays(g, vocab, cur["ids"], cur["offs"], k)))
            cur["done"].append(step)
        elif what in ("filter", "edges", "nodes"):
            ids = _remove(g, step, order, eorder)
            out.append((what, step[1:], ids, oracle_arrays(g, vocab, cur["ids"], cur["offs"], k)))
            cur["done"].append(step)
        elif what == "correct":
            target = g
            if len(step) > 1 and step[1]:
                target = _graph(cur["reads"], cur["pos"], k)
                for s in cur["done"]:
                    if s[0] == "clip":
                        target.remove_short_linear_paths(*s[1:])
                    else:
                        _remove(target, s)
            corrected = target.correct_reads(fq)
            out.append(("correct", corrected))
        elif what == "rebuild":
            r2, p2 = corrected
            ids2 = list(r2.keys())
            offs2 = np.concatenate([[0], np.cumsum([len(r2[r]) for r in ids2])]).astype(np.int64)
            g = _graph(r2, p2, k)
            cur = {"reads": r2, "pos": p2, "ids": ids2, "offs": offs2, "done": []}
            order, eorder = _orders(g)
            out.append(("rebuild", oracle_arrays(g, vocab, ids2, offs2, k)))
        else:
            raise ValueError(what)
    return {"k": k, "reads": reads, "vocab": vocab, "tokens": toks, "offsets": offs, "ids": read_ids, "pos": pos, "fq": fq,
            "records": out}


# ------------------------------------------------------------------ the engine's side
def engine_run(eng, exp, routes=()):
    """the steps of `exp` on the engine, compared with the oracle's record after each; returns what the run left for
    the comparison between two runs.  routes: per "correct" step, True where the correction must have re-threaded"""
    vocab, read_ids, fq, k = exp["vocab"], exp["ids"], exp["fq"], exp["k"]
    eng.set_reads(exp["tokens"], exp["offsets"], vocab.two_v)
    gs, ge = flat_positions(read_ids, exp["reads"], exp["pos"])
    eng.set_positions(gs, ge, np.asarray([len(fq[r]["sequence"]) for r in read_ids], dtype=np.int64))
    left, ids, n_correct = [], read_ids, 0
    for rec in exp["records"]:
        what = rec[0]
        if what == "build":
            eng.build(k)
            compare_engine_to_oracle(eng, rec[1])
        elif what == "clip":
            removed = eng.remove_short_linear_paths(rec[1], protect=rec[2])
            assert removed.tolist() == rec[3], (rec[1], removed.tolist(), rec[3])
            compare_engine_to_oracle(eng, rec[4], live_only=True)
            left += [removed, live_arrays(eng)]
        elif what == "filter":
            eng.filter(*rec[1])
            compare_engine_to_oracle(eng, rec[3], live_only=True)
        elif what in ("edges", "nodes"):
            (eng.remove_edges if what == "edges" else eng.remove_nodes)(rec[2])
            compare_engine_to_oracle(eng, rec[3], live_only=True)
        elif what == "correct":
            ids_next, out = check_corrected(eng, vocab, ids, *rec[1])
            if n_correct < len(routes) and routes[n_correct]:
                assert eng.correct_routes()["gapped"] > 0      # re-threaded: the live lists were made (or patched)
            n_correct += 1
            left.append(out)
        elif what == "rebuild":
            eng.adopt_corrected()
            eng.build(k)
            ids = ids_next
            compare_engine_to_oracle(eng, rec[1])
            left.append(live_arrays(eng))
    return left


def same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if isinstance(x, dict):
            assert x.keys() == y.keys()
            for key in x:
                assert np.array_equal(x[key], y[key]), key
        else:
            assert np.array_equal(x, y)


def both_ways(eng, monkeypatch, exp, routes=()):
    """the case by the default (the row summary where no lists exist) and with AMG_CLIP_LISTS=1 (always the lists)"""
    monkeypatch.setenv("AMG_CORR_ROUTES", "1")
    monkeypatch.delenv("AMG_CLIP_LISTS", raising=False)
    a = engine_run(eng, exp, routes)
    monkeypatch.setenv("AMG_CLIP_LISTS", "1")
    b = engine_run(eng, exp, routes)
    same(a, b)
    return a


# ------------------------------------------------------------------ synthetic read sets (tests/test_gpu_sweep.py's first two)
SETS = {"k5": (7, 400, 30, 300, 5, 0.03), "k3": (11, 400, 24, 200, 3, 0.03)}


@functools.lru_cache(maxsize=None)
def synth_reads(name):
    seed, N, L, V, k, err = SETS[name]
    return P.synth_inputs(seed, N, L, V, err)[0], k


def n_removed(left):
    return len(left[0])


@pytest.mark.parametrize("name,L", [(n, L) for n in SETS for L in (1, 2, SETS[n][4], 2 * SETS[n][4], 64)])
def test_pristine_graph(eng, monkeypatch, name, L):
    """a graph just built (no labels: the closed test reads the rows), clipped at several lengths, then corrected and
    rebuilt from the clipped graph.  Something must go at some length: the oracle removes nodes from L = 2 on in both
    read sets (26 / 20 at L = 2, 379 / 153 at L = 64), nothing at L = 1 (no path is shorter than one node)"""
    reads, k = synth_reads(name)
    exp = expected(reads, k, [("clip", L), ("correct",), ("rebuild",)])
    left = both_ways(eng, monkeypatch, exp)
    assert (n_removed(left) > 0) == (L >= 2)


def every_seventh_edge_with_twin(g):
    """every seventh directed edge in id order and the edge back (the reference's tip clipping asserts that adjacency
    is mutual, construct_graph.py:364-386: with one direction alone removed the oracle raises instead of clipping)"""
    edges = g.get_edges()
    picked = []
    for h in list(edges)[::7]:
        e = edges[h]
        picked.append(h)
        picked += [x for x, t in edges.items()
                   if t.get_sourceNode() == e.get_targetNode() and t.get_targetNode() == e.get_sourceNode()
                   and t.get_sourceNodeDirection() == -e.get_targetNodeDirection()
                   and t.get_targetNodeDirection() == -e.get_sourceNodeDirection()]
    return list(dict.fromkeys(picked))


def test_dead_edges_between_live_nodes(eng, monkeypatch):
    """edges removed on their own: both their nodes live on, so the pass over the edges must skip them by their own
    alive byte; the clip is the one by component labels (the graph is no longer as built)"""
    reads, k = synth_reads("k5")
    exp = expected(reads, k, [("edges", every_seventh_edge_with_twin), ("clip", k), ("correct",), ("rebuild",)])
    left = both_ways(eng, monkeypatch, exp)
    assert n_removed(left) > 0


def test_every_seventh_directed_edge_alone(eng, monkeypatch):
    """every seventh DIRECTED edge removed and its twin left: the reference cannot clip such a graph (see
    every_seventh_edge_with_twin), the engine can — no oracle here, the two views must agree with each other"""
    from amira_amd import tokenize
    reads, k = synth_reads("k5")
    vocab, toks, offs, read_ids = tokenize(reads)
    left = []
    for lists in (False, True):
        if lists:
            monkeypatch.setenv("AMG_CLIP_LISTS", "1")
        else:
            monkeypatch.delenv("AMG_CLIP_LISTS", raising=False)
        eng.set_reads(toks, offs, vocab.two_v)
        eng.build(k)
        eng.remove_edges(np.arange(0, eng.counts()["n_edges"], 7))
        removed = eng.remove_short_linear_paths(k)
        left.append([removed, live_arrays(eng)])
    same(*left)


def test_after_a_coverage_filter(eng, monkeypatch):
    """filter(2, 1), then the clip: by component labels, on rows that lost edges with their nodes"""
    reads, k = synth_reads("k5")
    exp = expected(reads, k, [("filter", 2, 1), ("clip", k), ("correct",), ("rebuild",)])
    left = both_ways(eng, monkeypatch, exp)
    assert n_removed(left) > 0       # (the oracle removes 3 nodes)


@pytest.mark.parametrize("min_cov", [3, 2])
def test_lists_already_present(eng, monkeypatch, min_cov):
    """filter(min_cov, 1) and a correction that re-threads reads: the live lists exist when the clip comes, so it walks
    them (with or without the switch) and leaves them to be patched.  Had the row summary been written over them, the
    correction after the clip — which re-threads again, through the patched lists — would not match the oracle.
    (After filter(3, 1) this read set has no tip left and the clip removes nothing; after filter(2, 1) it removes 3.)"""
    reads, k = synth_reads("k5")
    exp = expected(reads, k, [("filter", min_cov, 1), ("correct", True), ("clip", k), ("correct",)])
    left = both_ways(eng, monkeypatch, exp, routes=(True, True))
    assert (len(left[1]) > 0) == (min_cov == 2)


def every_ninth_live_node(g):
    return list(g.get_nodes())[::9]


def test_lists_needed_after_a_light_clip(eng, monkeypatch):
    """clip of a fresh graph (row summary in the lists' row buffer), then listed nodes die and the correction
    re-threads reads: the lists must be made from the edges, not patched from rows that never were lists"""
    reads, k = synth_reads("k5")
    exp = expected(reads, k, [("clip", k), ("nodes", every_ninth_live_node), ("correct",)])
    left = both_ways(eng, monkeypatch, exp, routes=(True,))
    assert n_removed(left) > 0


# ------------------------------------------------------------------ hand-made read sets (k = 3)
def genes(text, strand="+"):
    return [strand + x for x in text.split()]


def labels(g_nodes):
    """node hash -> the genes of its canonical gene-mer, strands dropped"""
    return {h: tuple(x.get_name() for x in n.get_canonical_geneMer()) for h, n in g_nodes.items()}


def holding(g_nodes, gene):
    return {h for h, names in labels(g_nodes).items() if gene in names}


BACKBONE = " ".join(f"b{i}" for i in range(16))


def hub_reads():
    """one read that passes a b c 72 times, each time with another gene behind it: (a, b, c) has 73 neighbours on one
    side and 71 on the other (rows far beyond the two slots of the summary, beyond a wave's 64 lanes for the lists);
    a short read hangs a tip of two nodes off it (the long read's last node is a tip of one node: it goes too)"""
    return {"long": genes(" ".join(f"a b c x{i}" for i in range(72))), "tip": genes("a b c t1 t2")}, 3


def check_hub(before, g, removed):
    hub = next(n for n in before.values() if tuple(x.get_name() for x in n.get_canonical_geneMer()) in (("a", "b", "c"), ("c", "b", "a")))
    assert hub.__hash__() in g.get_nodes()
    assert min(len(hub.get_forward_edge_hashes()), len(hub.get_backward_edge_hashes())) >= 70    # (after the clip)
    tip = holding(before, "t1")
    assert len(tip) == 2 and tip <= set(removed)


def test_tip_on_a_hub(eng, monkeypatch):
    reads, k = hub_reads()
    both_ways(eng, monkeypatch, expected(reads, k, [("clip", 3), ("correct",), ("rebuild",)], check_hub))


def two_backward_reads():
    """X = (x1, x2, x3) is reached from (v, x1, x2) and from (w, x1, x2) on its backward side and goes on to
    (x2, x3, u1), (x3, u1, u2) on its forward side.  (w, x1, x2) exists before X does (reads that stop at x2), the
    edge to (v, x1, x2) is made first: of X's two backward edges the one with the smaller id leads to the node with
    the larger id.  With X's forward edge removed alone, X is a path node of degree two whose edges are both
    backward, and the walk that comes in from the tip (x3, u1, u2) goes on along the FIRST of them: down the v chain,
    which makes the path too long to clip.  The other edge would end it at four nodes — a tip to remove."""
    reads = {}
    for c in range(10):
        reads[f"w0_{c}"] = genes("w x1 x2", "-")
    reads["v"] = genes("v4 v3 v2 v x1 x2 x3 u1 u2", "-")
    for c in range(10):
        reads[f"w1_{c}"] = genes("w x1 x2 x3", "-")
    return reads, 3


def forward_edge_of_x(g):
    x = next(n for n in g.get_nodes().values() if {y.get_name() for y in n.get_canonical_geneMer()} == {"x1", "x2", "x3"})
    assert len(x.get_forward_edge_hashes()) == 1 and len(x.get_backward_edge_hashes()) == 2
    return list(x.get_forward_edge_hashes())


def check_two_backward(before, g, removed):
    order, eorder = _orders(g)     # (nothing has been deleted from the node dict; edge positions keep their order)
    x = next(n for n in g.get_nodes().values() if {y.get_name() for y in n.get_canonical_geneMer()} == {"x1", "x2", "x3"})
    assert x.get_forward_edge_hashes() == []
    e0, e1 = x.get_backward_edge_hashes()
    assert eorder[e0] < eorder[e1]
    t0, t1 = (g.get_edge_by_hash(e).get_targetNode().__hash__() for e in (e0, e1))
    assert order[t0] > order[t1]
    assert removed == []


def test_first_of_two_backward_edges(eng, monkeypatch):
    reads, k = two_backward_reads()
    exp = expected(reads, k, [("edges", forward_edge_of_x), ("clip", 5), ("correct",)], check_two_backward)
    both_ways(eng, monkeypatch, exp)


def tip_length_reads():
    """two tips off a backbone of coverage 3: p of two nodes, q of three"""
    reads = {f"bb{c}": genes(BACKBONE) for c in range(3)}
    reads["p"] = genes("b4 b5 b6 p1 p2")
    reads["q"] = genes("b9 b10 b11 q1 q2 q3")
    return reads, 3


def check_tip_lengths(before, g, removed):
    p, q = holding(before, "p1"), holding(before, "q1")
    assert len(p) == 2 and len(q) == 3
    assert p <= set(removed) and not (q & set(removed))


def test_tip_of_min_length_and_one_less(eng, monkeypatch):
    """min_length 3: the tip of two nodes goes, the tip of three stays"""
    reads, k = tip_length_reads()
    both_ways(eng, monkeypatch, expected(reads, k, [("clip", 3), ("correct",), ("rebuild",)], check_tip_lengths))


def check_whole_component(before, g, removed):
    m = holding(before, "m2")
    assert len(m) == 2 and not (m & set(removed))
    assert holding(before, "p1") <= set(removed)


def test_path_that_is_its_component(eng, monkeypatch):
    """a read of four genes nobody else has: two nodes, a path shorter than min_length that is its whole component"""
    reads, k = tip_length_reads()
    reads["m"] = genes("m1 m2 m3 m4")
    both_ways(eng, monkeypatch, expected(reads, k, [("clip", 5), ("correct",), ("rebuild",)], check_whole_component))


def high_coverage_reads():
    """a backbone of coverage 1 with two tips of two nodes: h of coverage 6 (above 1.5 x the mean of 49 / 32),
    l of coverage 1"""
    reads = {"bb": genes(" ".join(f"b{i}" for i in range(30)))}
    for c in range(6):
        reads[f"h{c}"] = genes("b10 b11 b12 h1 h2")
    reads["l"] = genes("b20 b21 b22 l1 l2")
    return reads, 3


def check_high_coverage(before, g, removed):
    h, low = holding(before, "h1"), holding(before, "l1")
    assert len(h) == 2 and all(before[x].get_node_coverage() == 6 for x in h)
    assert not (h & set(removed)) and low <= set(removed)


def test_tip_of_high_coverage(eng, monkeypatch):
    reads, k = high_coverage_reads()
    both_ways(eng, monkeypatch, expected(reads, k, [("clip", 3), ("correct",), ("rebuild",)], check_high_coverage))


def check_protected(before, g, removed):
    p = holding(before, "p1")
    kept = holding(before, "p2")
    assert len(kept) == 1 and kept < p
    assert not (kept & set(removed)) and (p - kept) <= set(removed)


def test_protected_node_of_a_tip(eng, monkeypatch):
    """the end node of the tip p holds the protected gene p2: it stays, the tip's other node goes"""
    reads, k = tip_length_reads()
    both_ways(eng, monkeypatch, expected(reads, k, [("clip", 3, ("p2",)), ("correct",), ("rebuild",)], check_protected))
