"""tests/path_sketch.py against the reference alone: `expected` gives what the oracle's GeneMerGraph gives on a graph with
bubbles, and every case class has the property it was built for.  A class that fails here is wrong, not the engine."""
import numpy as np
import pytest

import path_sketch as PS
import procedures as P


def test_expected_is_what_the_oracle_graph_computes():
    """get_minhashes_for_paths + get_minimizers_from_minhashes (construct_graph.py:2148-2194, :1747-1751) at their fixed
    ksize 11 and scaled 10, on the kind of graph tests/test_gpu_bubbles.py::_graph makes"""
    from amira_amd import synth
    from amira_amd.tokens import tokenize
    from amira_oracle import GeneMerGraph
    k = 3
    ids, sts = synth.loop_reads(71, 40, 16, 40, 0.04, 0)
    calls = synth.to_read_dict(ids, sts, synth.gene_names(40, 0))
    pos = {r: [(80 * i, 80 * i + 59) for i in range(len(g))] for r, g in calls.items()}
    fq = P.synth_fastq(calls, pos, flank=40)
    g = GeneMerGraph(calls, k, pos)
    _, toks, offs, read_ids = tokenize(calls)
    order = {h: i for i, h in enumerate(g.get_nodes())}
    tok_node = np.full(len(toks), -1, np.int32)
    for r, rid in enumerate(read_ids):
        for i, h in enumerate(g.get_readNodes()[rid]):
            tok_node[int(offs[r]) + i] = order[h]
    gs = np.array([p[0] for rid in read_ids for p in pos[rid]], np.int64)
    ge = np.array([p[1] for rid in read_ids for p in pos[rid]], np.int64)
    paths = []
    for junctions in g.identify_potential_bubble_starts().values():
        unique = g.get_all_paths_between_junctions_in_component(junctions, 4 * k, 1)
        paths += sorted(g.filter_paths_between_bubble_starts(unique), key=lambda e: len(e[0]))
    assert len(paths) >= 4
    sketches = g.get_minhashes_for_paths(paths, fq, 1)
    want = [g.get_minimizers_from_minhashes([n[0] for n in p[0]], sketches) for p in paths]
    pairs = [(a, b) for a in range(len(paths)) for b in range(len(paths))]
    sizes, common = PS.expected(toks, offs, gs, ge, k, tok_node, [fq[rid]["sequence"] for rid in read_ids], None, 11, 10,
                                [[order[n[0]] for n in p[0]] for p in paths], pairs)
    assert sizes.dtype == np.int64 and common.dtype == np.int64
    assert sizes.tolist() == [len(s) for s in want] and min(sizes) > 0
    assert common.tolist() == [len(want[a] & want[b]) for a, b in pairs]
    assert len(set(common.tolist())) > 10   # (overlaps of many sizes, not all or nothing)


ALL = list(PS.CLASSES) + PS.SEAM_CASES


def _one_segment(c, p):
    (n,) = set(c.paths[p])
    texts = [t for m, t in PS.segments(c.off, c.gs, c.ge, c.k, c.tok_node, c.sequences, c.row_to_seq) if m == n]
    assert len(texts) == 1, (c.name, p)
    return texts[0]


@pytest.mark.parametrize("name", ALL, ids=PS.case_id)
def test_every_claim_of_a_case_holds_by_the_reference(name):
    c = PS.case(name)
    sizes, common = c.expected()
    assert len(c.claims) > 0 and sizes.sum() > 0 and common.sum() > 0, c.name
    for claim in c.claims:
        what = claim[0]
        if what == "common_is_size":
            assert common[claim[1]] == sizes[claim[2]] > 0, (c.name, claim)
        elif what == "size":
            assert sizes[claim[1]] == claim[2], (c.name, claim)
        elif what == "smaller":
            assert sizes[claim[1]] < sizes[claim[2]], (c.name, claim)
        elif what == "text":
            assert _one_segment(c, claim[1]) == claim[2], (c.name, claim[:2])
        elif what == "seam":
            S, s = _one_segment(c, claim[1]), claim[2]
            for o in range(s - c.ksize + 1, s + 1):
                assert o >= 0 and len(S[o:o + c.ksize]) == c.ksize and PS.sketch(S[o:o + c.ksize], c.ksize, 1), (c.name, claim, o)
        else:
            raise AssertionError(claim)


@pytest.mark.parametrize("name", PS.SEAM_CASES, ids=PS.case_id)
def test_seam_cases_cover_what_they_list(name):
    k, ksize, scaled, lengths = name
    c = PS.case(name)
    texts = [cl[2] for cl in c.claims if cl[0] == "text"]
    assert [len(t) for t in texts] == list(lengths or PS.seam_lengths(ksize))
    assert len(set(t for t in texts if len(t) > 3)) == len([t for t in texts if len(t) > 3])   # bases of their own
    seams = [cl[2] for cl in c.claims if cl[0] == "seam"]
    for s in PS.SEAMS:   # a seam counts where a k-mer starts on it: the segment reaches a chunk of its own behind it
        assert seams.count(s) == sum(1 for t in texts if len(t) >= s + ksize)
    if lengths is None:
        assert seams.count(1024) >= 5 and seams.count(2048) >= 1 and max(len(t) for t in texts) > 3072 and len(texts) >= 10
    # every seam inside a segment has its witness, and the witness is the stretch around the seam
    n_witnesses = sum(1 for cl in c.claims if cl[0] == "common_is_size")
    assert n_witnesses == sum(1 for t in texts for s in PS.SEAMS
                              if len(t) > s and len(t[max(s - ksize - 2, 0):s + ksize + 2]) >= ksize)
    assert n_witnesses >= len(seams) > 0


def test_membership_lists_one_node_by_every_count():
    c = PS.case("membership")
    listings = np.bincount([n for p in c.paths for n in p])
    assert set(PS.LISTED_BY) <= set(listings.tolist())
    empty = [i for i, p in enumerate(c.paths) if not p]
    assert empty[0] == 0 and empty[-1] == len(c.paths) - 1 and len(empty) == 3
    assert any(a == b and c.paths[a] for a, b in c.pairs) and any(a == b and not c.paths[a] for a, b in c.pairs)
    assert any(c.paths[a] and not c.paths[b] for a, b in c.pairs) and any(not c.paths[a] and c.paths[b] for a, b in c.pairs)
    assert any(len(p) == 2 and p[0] == p[1] for p in c.paths)


def test_filtered_case_names_nodes_without_a_live_window():
    c = PS.case("membership_filtered")
    live = set(c.tok_node[c.tok_node >= 0].tolist())
    assert (c.tok_node == -2).sum() == 2
    assert any(p and not set(p) & live for p in c.paths), "a path of dead nodes only"
    assert any(set(p) & live and set(p) - live for p in c.paths), "a path of a live and a dead node"


def test_sharing_case_has_what_it_lists():
    c = PS.case("sharing")
    per_read = [c.tok_node[int(a):int(b)] for a, b in zip(c.off[:-1], c.off[1:])]
    assert any(len(r[r >= 0]) > len(set(r[r >= 0].tolist())) for r in per_read), "a node twice on one read"
    # the reverse-strand read sits on the nodes of the forward one, and its segments are their reverse complements
    w = c.reverse_first_window
    fw = [x for x in np.flatnonzero(c.tok_node == c.tok_node[w]).tolist() if x != w]
    assert len(fw) == 1 and c.tokens[w] < c.two_v // 2 <= c.tokens[fw[0]]
    fwd, rev = [t for _, t in PS.segments(c.off, c.gs, c.ge, c.k, c.tok_node, c.sequences, c.row_to_seq, {int(c.tok_node[w])})]
    assert len(fwd) == 280 and rev == PS.revcomp(fwd)
    reads_of_node = np.bincount(c.tok_node[c.tok_node >= 0])
    assert reads_of_node.max() == 40
    node = int(reads_of_node.argmax())
    starts = c.gs[c.tok_node == node]
    assert len(set((starts % 64).tolist())) == 40
    # sequences in another order than the reads, more of them than reads, and reads without one on no path
    rows = c.row_to_seq
    assert len(c.sequences) > (rows >= 0).sum() and (rows[rows >= 0] != np.flatnonzero(rows >= 0)).any()
    assert len(set(rows[rows >= 0].tolist())) == (rows >= 0).sum()
    listed = {n for p in c.paths for n in p}
    for r in np.flatnonzero(rows < 0).tolist():
        assert not listed & set(c.tok_node[int(c.off[r]):int(c.off[r + 1])].tolist())


def test_runs_case_has_both_kinds_of_waves():
    c = PS.case("runs")
    pairs = PS.sorted_pairs(c, c.tok_node)
    assert len(pairs) == PS.pair_count(c, c.tok_node)
    inside, spanning = PS.wave_kinds([p for p, _ in pairs])
    assert inside >= 100 and spanning >= 100, (inside, spanning)
    # two neighbours in path order with the same single hash: the last pair of one, the first of the next
    twins = [(a, b) for (a, x), (b, y) in zip(pairs, pairs[1:]) if a != b and x == y]
    assert len(twins) >= 2 and all(b == a + 1 for a, b in twins)
    sizes, _ = c.expected()
    assert len(c.small) == 400 and sorted(set(sizes[c.small].tolist())) == [1, 2, 3, 4, 5]
    assert all(2900 < sizes[p] <= 3000 for p in c.big)
    for p, q in zip(c.big, c.big[1:]):
        assert any(p < s < q for s in c.small)   # small paths between the big ones


def test_pair_count_counts_every_occurrence():
    c = PS.Case("count", 3, 4, 1, 5)
    x = c.whole("ACGTACGTAC")       # 7 windows, fewer distinct hashes
    c.path([x])
    c.path([x, x])
    c.path([c.whole("ACG")])
    c.finish()
    assert PS.kept_windows("ACGTACGTAC", 4, 1) == 7 > len(PS.sketch("ACGTACGTAC", 4, 1))
    assert PS.pair_count(c, c.tok_node) == 7 * 3
