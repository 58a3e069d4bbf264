"""amg_path_sketch_overlaps (amira_amd/csrc/amg_sketch.hip) on the constructed cases of tests/path_sketch.py: sketch
sizes and overlaps exactly as the reference's slices, sourmash's hashes and Python's sets give them
(tests/test_path_sketch_cpu.py holds the cases and `expected` against the oracle alone) — segments that cross the seams
of k_bs_hash's chunks at every k-mer width, the clipping of a Python slice, what a base may be, nodes listed by many
paths, empty paths, windows that share bases, waves of k_bs_unique inside one path and across many — and what a refused
call leaves behind: nothing."""
import numpy as np
import pytest

import path_sketch as PS

pytestmark = pytest.mark.gpu

E_ARG, E_STATE, E_NOMEM = -2, -3, -6     # include/amg.h
BASE = PS.SEAM_CASES[8]                   # the class-(a) call the others are followed by: k 3, ksize 11, scaled 1


@pytest.fixture(scope="module")
def eng():
    from amira_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def load(eng, c, gs=None, ge=None, positions=True):
    """the case's reads (and positions) on the engine, its graph built; returns the engine's node id per window"""
    eng.set_reads(c.tokens, c.off, c.two_v)
    if positions:
        eng.set_positions(c.gs if gs is None else gs, c.ge if ge is None else ge)
    eng.build(c.k)
    if c.filter is not None:
        eng.filter(c.filter, 1)
    return eng.read_node_ids()


def call(eng, c, paths=None, pairs=None, sequences=None, row_to_seq="case", ksize=None, scaled=None):
    from amira_amd.engine import Sequences
    path_off, path_node = c.path_arrays(paths)
    pairs = c.pairs if pairs is None else pairs
    s = Sequences(c.sequences if sequences is None else sequences, 0)
    try:
        return eng.path_sketch_overlaps(s, c.row_to_seq if isinstance(row_to_seq, str) else row_to_seq,
                                        c.ksize if ksize is None else ksize, c.scaled if scaled is None else scaled,
                                        path_off, path_node, [a for a, _ in pairs], [b for _, b in pairs])
    finally:
        s.close()


def same(c, got, want, what=""):
    for name, g, w in zip(("sizes", "common"), got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == np.int64 and w.dtype == np.int64 and g.shape == w.shape, (c.name, what, name)
        bad = np.flatnonzero(g != w)
        assert len(bad) == 0, "%s %s: %s differ at %s: got %s, expected %s" % (c.name, what, name, bad[:8].tolist(),
                                                                             g[bad[:8]].tolist(), w[bad[:8]].tolist())


def check(eng, c, what=""):
    """load, call, compare with the reference (on the engine's own node ids, which are the ones the case was built on)"""
    tok_node = load(eng, c)
    windows = c.tok_node != -1
    assert np.array_equal(tok_node[windows], c.tok_node[windows]) and (tok_node[~windows] < 0).all(), c.name
    want = c.expected(tok_node)
    got = call(eng, c)
    same(c, got, want, what)
    return want


# ------------------------------------------------------------------ every class, exactly
@pytest.mark.parametrize("name", PS.SEAM_CASES, ids=PS.case_id)
def test_segments_across_the_seams_of_the_chunks(eng, name):
    c = PS.case(name)
    sizes, common = check(eng, c)
    assert sizes.sum() > 0 and common.sum() > 0, c.name
    if c.scaled == 1:   # every hash of a witness is in the segment it was cut from
        for _, q, p in (cl for cl in c.claims if cl[0] == "common_is_size"):
            assert common[q] == sizes[p] > 0


@pytest.mark.parametrize("name", sorted(PS.CLASSES))
def test_class_equals_the_reference(eng, name):
    c = PS.case(name)
    sizes, common = check(eng, c)
    assert sizes.sum() > 0 and common.sum() > 0, c.name


def test_no_pairs_no_paths_and_nothing_to_hash(eng):
    c = PS.case("membership")
    tok_node = load(eng, c)
    sizes, _ = c.expected(tok_node)
    none = np.zeros(0, np.int64)
    same(c, call(eng, c, pairs=[]), (sizes, none), "n_pairs == 0")
    same(c, call(eng, c, paths=[], pairs=[]), (none, none), "n_paths == 0")
    same(c, call(eng, c, paths=[[], []], pairs=[(0, 1), (1, 1)]), (np.zeros(2, np.int64), np.zeros(2, np.int64)), "empty paths only")
    same(c, call(eng, c), c.expected(tok_node), "afterwards")
    # no segment reaches ksize: no (path, hash) pair at all
    c = PS.case("slices")
    tok_node = load(eng, c)
    short = [i for i, s in enumerate(c.expected(tok_node)[0].tolist()) if s == 0]
    assert len(short) >= 8
    same(c, call(eng, c, paths=[c.paths[i] for i in short], pairs=[(0, 1)]), (np.zeros(len(short), np.int64), np.zeros(1, np.int64)),
         "nothing to hash")


def test_positions_and_rows_of_unlisted_reads_are_not_looked_at(eng):
    """the reference slices the reads of the paths' nodes and no others"""
    c = PS.case(BASE)
    tok_node = load(eng, c)
    want = c.expected(tok_node)
    w = int(np.flatnonzero(tok_node == c.paths[1][0])[0])
    gs = c.gs.copy()
    gs[w] = -7
    rows = np.arange(len(c.off) - 1, dtype=np.int32)
    rows[int(np.searchsorted(c.off, w, side="right")) - 1] = -1
    keep = [p for p in range(len(c.paths)) if p != 1]
    load(eng, c, gs=gs)
    got = call(eng, c, paths=[c.paths[p] for p in keep], pairs=[], row_to_seq=rows)
    same(c, got, (want[0][keep], np.zeros(0, np.int64)))


# ------------------------------------------------------------------ refusals, and what they leave behind
def _first_window(c, tok_node, p=0):
    w = int(np.flatnonzero(tok_node == c.paths[p][0])[0])
    return w, int(np.searchsorted(c.off, w, side="right")) - 1


def _negative_start(eng, c, tok_node):
    gs = c.gs.copy()
    gs[_first_window(c, tok_node)[0]] = -1
    load(eng, c, gs=gs)
    call(eng, c)


def _negative_end(eng, c, tok_node):
    ge = c.ge.copy()
    ge[_first_window(c, tok_node)[0] + c.k - 1] = -5
    load(eng, c, ge=ge)
    call(eng, c)


def _row(value):
    def run(eng, c, tok_node):
        rows = np.arange(len(c.off) - 1, dtype=np.int32)
        rows[_first_window(c, tok_node, 1)[1]] = value(c)
        call(eng, c, row_to_seq=rows)
    return run


def _no_positions(eng, c, tok_node):
    load(eng, c, positions=False)
    call(eng, c)


REFUSALS = {
    "a gene start below zero on a listed node": (E_ARG, _negative_start),
    "a gene end below zero on a listed node": (E_ARG, _negative_end),
    "row_to_seq of -1 on a listed node": (E_ARG, _row(lambda c: -1)),
    "row_to_seq at the number of sequences": (E_ARG, _row(lambda c: len(c.sequences))),
    "row_to_seq beyond the number of sequences": (E_ARG, _row(lambda c: len(c.sequences) + 1000)),
    "fewer sequences than reads": (E_ARG, lambda eng, c, t: call(eng, c, sequences=c.sequences[:-1])),
    "a path node equal to the node count": (E_ARG, lambda eng, c, t: call(eng, c, paths=c.paths + [[c.n_nodes]])),
    "a path node below zero": (E_ARG, lambda eng, c, t: call(eng, c, paths=c.paths + [[-1]])),
    "a pair naming a missing path": (E_ARG, lambda eng, c, t: call(eng, c, pairs=c.pairs + [(0, len(c.paths))])),
    "a pair naming path -1": (E_ARG, lambda eng, c, t: call(eng, c, pairs=[(-1, 0)] + c.pairs)),
    "ksize 0": (E_ARG, lambda eng, c, t: call(eng, c, ksize=0)),
    "ksize 33": (E_ARG, lambda eng, c, t: call(eng, c, ksize=33)),
    "scaled 0": (E_ARG, lambda eng, c, t: call(eng, c, scaled=0)),
    "no positions set": (E_STATE, _no_positions),
}


@pytest.mark.parametrize("what", list(REFUSALS))
def test_a_refused_call_leaves_nothing_behind(eng, what):
    from amira_amd._ffi import AmgError
    code, run = REFUSALS[what]
    c = PS.case(BASE)
    want = check(eng, c, "before")
    assert want[0].sum() > 0 and want[1].sum() > 0
    with pytest.raises(AmgError) as err:
        run(eng, c, c.tok_node)
    assert err.value.code == code, (what, str(err.value))
    # the same engine, whatever the refused call did to it: the class-(a) call again
    load(eng, c)
    same(c, call(eng, c), want, "after " + what)


def test_pair_limit_on_its_boundary(eng, monkeypatch):
    """AMG_TEST_SKETCH_PAIRS = n: a call of M (path, hash) pairs is refused when M >= n"""
    from amira_amd._ffi import AmgError
    c = PS.case(PS.SEAM_CASES[9])    # (scaled 2: the count is of the hashes that pass the cut)
    tok_node = load(eng, c)
    want = c.expected(tok_node)
    M = PS.pair_count(c, tok_node)
    assert 1000 < M < sum(len(s) for s in c.sequences) * 0.6
    for limit, refused in ((M - 1, True), (M, True), (M + 1, False), (M - 1, True), (M + 1, False)):
        monkeypatch.setenv("AMG_TEST_SKETCH_PAIRS", str(limit))
        if refused:
            with pytest.raises(AmgError) as err:
                call(eng, c)
            assert err.value.code == E_NOMEM, (limit, M)
        else:
            same(c, call(eng, c), want, "limit %d of %d" % (limit, M))
    monkeypatch.delenv("AMG_TEST_SKETCH_PAIRS")
    same(c, call(eng, c), want, "without a limit")


# ------------------------------------------------------------------ one engine, many calls
def test_calls_of_all_sizes_on_one_engine_equal_those_of_fresh_engines(eng):
    """the call keeps its buffers: a large call, a tiny one, the large one again, then another graph (another k)"""
    from amira_amd import Engine
    tiny = PS.Case("tiny", 3, 11, 1, 71)
    x = tiny.whole(PS.bases(tiny.rng, 30))
    tiny.path([x])
    tiny.pair(0, 0)
    tiny.finish()
    order = [PS.case("runs"), tiny, PS.case("runs"), PS.case(PS.SEAM_CASES[12]), PS.case(BASE)]
    assert order[3].k == 5 and order[4].k == 3
    reused = []
    for c in order:
        load(eng, c)
        reused.append(call(eng, c))
    for c, got in zip(order, reused):
        fresh = Engine(0)
        try:
            tok_node = load(fresh, c)
            alone = call(fresh, c)
        finally:
            fresh.close()
        same(c, got, alone, "on the reused engine against a fresh one")
        same(c, got, c.expected(tok_node), "on the reused engine")
        assert alone[0].sum() > 0 and alone[1].sum() > 0
