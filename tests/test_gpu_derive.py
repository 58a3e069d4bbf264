"""The derived rebuild (amg_derive.hip: the graph of a correction that re-threaded nothing is the graph at hand squeezed
to its live part) on its boundary and as a graph to work on.

  a  every case class of tests/derive_cases.py: the engine derives exactly when predicted_derivable (computed from the
     oracle graph alone) says so, and the graph equals the oracle's either way, with and without AMG_NO_DERIVE=1
  b  a second cleaning iteration chained onto the sweep of test_gpu_sweep.py without a new set_reads, compared with the
     oracle after every step; the verdict of every rebuild against the predicate
  c  the derived graph under every consumer: component filter, listed removals and re-threading, tip clipping,
     match_patterns, finalize
  d  build_filtered on a derive-ready context
  e  leaving the derived state: another k, fresh reads, a plain build after the flag was used
  f  borrowed device inputs and int32 positions through a derived rebuild

All comparisons are exact.  Oracle results that several tests need are computed once (SOURCES) and not changed."""
import random

import numpy as np
import pytest

import derive_cases as DC
import procedures as P
from helpers import check_corrected, compare_engine_to_oracle, live_arrays, oracle_arrays
from test_gpu_sweep import sweep_begin, sweep_iteration

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from amira_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def graph_state(eng):
    """everything the read-backs show of the graph at hand"""
    n, e = eng.nodes(), eng.edges()
    tn, td = eng.read_nodes()
    off, adj = eng.node_adj()
    roff, ridx = eng.node_reads()
    out = {"n_" + key: v for key, v in n.items()}
    out.update({"e_" + key: v for key, v in e.items()})
    out.update(tok_node=tn, tok_dir=np.where(tn >= 0, td, 0), adj_off=off, adj=adj, nr_off=roff, nr=ridx)
    return out


def same_state(a, b, what):
    assert a.keys() == b.keys()
    for key in a:
        assert np.array_equal(a[key], b[key]), (what, key)


def check_graph(eng, want):
    """compare_engine_to_oracle (nodes, edges, components, adjacency, per-window ids, node reads) and the first-seen
    token of every node: the first window of the read set that is the node"""
    compare_engine_to_oracle(eng, want)
    ids, first = np.unique(want["tok_node"], return_index=True)
    first = first[ids >= 0]
    assert np.array_equal(eng.nodes()["first_token"], first)
    c = eng.counts()
    assert c["n_live_nodes"] == c["n_nodes"] and c["n_live_edges"] == c["n_edges"] and c["n_reads_to_correct"] == 0


def load(eng, reads, pos32=False):
    vocab, toks, offs, read_ids, gs, ge, rl, pos, fq = DC.inputs(reads)
    eng.set_reads(toks, offs, vocab.two_v)
    if pos32:
        eng.set_positions(gs.astype(np.int32), ge.astype(np.int32), rl)
    else:
        eng.set_positions(gs, ge, rl)
    return vocab, offs, read_ids, {r: list(v) for r, v in pos.items()}, fq


# ------------------------------------------------------------------ a. verdict and graph, per case class
def run_case(eng, name, first_build=None):
    """build, the case's procedure, correct, adopt, rebuild: everything compared with the oracle; returns (predicted,
    derived, the state of the rebuilt graph).  first_build: (min_node_cov, min_edge_cov) — the procedure is that
    filter, and the engine applies it on the way (build_filtered)"""
    from amira_oracle import GeneMerGraph
    reads, k, procedure, edge_died_alone, _ = DC.case(name)
    vocab, offs, read_ids, pos, fq = load(eng, reads)
    g = GeneMerGraph(reads, k, pos)
    if first_build is None:
        eng.build(k)
        compare_engine_to_oracle(eng, oracle_arrays(g, vocab, read_ids, offs, k))
        DC.run_procedure(g, procedure, eng)
    else:
        assert procedure == [("filter",) + tuple(first_build)]
        eng.build_filtered(k, *first_build)
        DC.run_procedure(g, procedure)
    compare_engine_to_oracle(eng, oracle_arrays(g, vocab, read_ids, offs, k), live_only=True)
    predicted = DC.predicted_derivable(g, edge_died_alone)
    r2, p2 = g.correct_reads(fq)
    ids2, out2 = check_corrected(eng, vocab, read_ids, r2, p2)
    eng.adopt_corrected()
    eng.build(k)
    derived = eng.counts()["derived"]
    check_graph(eng, oracle_arrays(GeneMerGraph(r2, k, p2), vocab, ids2, out2["read_offsets"], k))
    return predicted, derived, graph_state(eng)


@pytest.mark.parametrize("name", sorted(DC.CASES))
def test_verdict_and_graph(eng, monkeypatch, name):
    predicted, derived, state = run_case(eng, name)
    print(f"verdict {name}: predicted {int(predicted)} derived {derived}")
    if name in DC.NEVER_DERIVED:
        assert derived == 0, name
    else:
        assert derived == int(predicted), (name, predicted, derived)
        assert predicted == DC.CASES[name][3]
    monkeypatch.setenv("AMG_NO_DERIVE", "1")
    _, derived_off, state_off = run_case(eng, name)
    assert derived_off == 0
    same_state(state, state_off, name)


@pytest.mark.parametrize("name,thr", [("front_reads_dropped_65", (2, 1)), ("short_reads", (2, 1)),
                                      ("self_loop_and_flip", (2, 1))])
def test_derived_after_a_filtered_build(eng, name, thr):
    """the graph at hand was made by build_filtered (its component labels are those of the graph BEFORE the filter:
    three vanished reads come first in front_reads_dropped and hold labels 1 .. 3): the derived graph's labels are its
    own"""
    predicted, derived, _ = run_case(eng, name, first_build=thr)
    assert predicted and derived == 1


# ------------------------------------------------------------------ b. going on from a derived graph
SWEEPS = {"seed7": (7, 400, 30, 300, 5, 0.03), "seed11": (11, 400, 24, 200, 3, 0.03), "nine": ("nine", 3)}


def sweep_inputs(which):
    spec = SWEEPS[which]
    if which == "nine":
        calls, pos = P.fixture("nine")
        lengths = {r: (pos[r][-1][1] + 200 if pos[r] else 100) for r in pos}
        return calls, pos, P.FakeFastq(lengths), spec[1]
    seed, N, L, V, k, err = spec
    reads, pos, fq = P.synth_inputs(seed, N, L, V, err)
    return reads, pos, fq, k


@pytest.mark.parametrize("no_derive", [False, True])
@pytest.mark.parametrize("which", sorted(SWEEPS))
def test_second_iteration_from_the_derived_graph(eng, monkeypatch, which, no_derive):
    """filter(3, 1), correct, adopt, build, clip, correct, adopt, build — twice, the second time from the (derived) third
    graph without set_reads; every step against the oracle, positions and removed ids included"""
    if no_derive:
        monkeypatch.setenv("AMG_NO_DERIVE", "1")
    reads, pos, fq, k = sweep_inputs(which)
    verdicts = []
    g1, vocab, ids, offs = sweep_begin(eng, reads, pos, fq, k)
    g3, ids3, offs3, _ = sweep_iteration(eng, g1, vocab, ids, offs, fq, k, verdicts=verdicts)
    sweep_iteration(eng, g3, vocab, ids3, offs3, fq, k, verdicts=verdicts)
    print(f"verdicts {which} no_derive={int(no_derive)}: (predicted, derived) per rebuild {verdicts}")
    assert len(verdicts) == 4
    if no_derive:
        assert [d for _, d in verdicts] == [0, 0, 0, 0]
    else:
        assert verdicts[1][1] == 1                                   # the third graph of the first iteration
        assert [d for _, d in verdicts] == [int(p) for p, _ in verdicts]


@pytest.mark.parametrize("no_derive", [False, True])
def test_two_derived_rebuilds_in_a_row(eng, monkeypatch, no_derive):
    """both_ends_cut_deep clipped at k, corrected, rebuilt, clipped at DEEP_CLIP, corrected, rebuilt: the second
    derived graph is made from a derived one (read sources and first-seen values already in moved coordinates)"""
    from amira_oracle import GeneMerGraph
    if no_derive:
        monkeypatch.setenv("AMG_NO_DERIVE", "1")
    reads, k, procedure, _, _ = DC.case("both_ends_cut_deep")
    vocab, offs, ids, pos, fq = load(eng, reads)
    eng.build(k)
    g = GeneMerGraph(reads, k, pos)
    derived = []
    for step in (procedure[0], ("clip", DC.DEEP_CLIP)):
        DC.run_procedure(g, [step], eng)
        compare_engine_to_oracle(eng, oracle_arrays(g, vocab, ids, offs, k), live_only=True)
        assert DC.predicted_derivable(g, False)
        r2, p2 = g.correct_reads(fq)
        ids, out = check_corrected(eng, vocab, ids, r2, p2)
        offs = out["read_offsets"]
        assert out["changed"].sum() >= 3
        eng.adopt_corrected()
        eng.build(k)
        derived.append(eng.counts()["derived"])
        g = GeneMerGraph(r2, k, p2)
        check_graph(eng, oracle_arrays(g, vocab, ids, offs, k))
    assert derived == ([0, 0] if no_derive else [1, 1])


# ------------------------------------------------------------------ the derived graphs the tests below work on
class Source:
    """a read set, what brings an engine to the derived graph of its corrected reads, and the oracle's corrected reads
    (computed once; every test makes its own oracle graph of them)"""

    def __init__(self, which):
        from amira_oracle import GeneMerGraph
        if which in SWEEPS:
            self.reads, pos, self.fq, self.k = sweep_inputs(which)
            self.steps = None
            arrays = self._sweep_arrays(pos)
        else:
            self.reads, self.k, self.steps, _, _ = DC.case(which)
            arrays = DC.inputs(self.reads)
            pos, self.fq = arrays[7:]
        self.vocab, self.toks, self.offs, self.read_ids, self.gs, self.ge, self.rl = arrays[:7]
        k = self.k
        g = GeneMerGraph(self.reads, k, {r: list(v) for r, v in pos.items()})
        if self.steps is None:          # the sweep: filter(3, 1), correct, rebuild, clip at k, correct
            g.filter_graph(3, 1)
            r2, p2 = g.correct_reads(self.fq)
            g = GeneMerGraph(r2, k, p2)
            g.remove_short_linear_paths(k)
        else:
            DC.run_procedure(g, self.steps)
        assert DC.predicted_derivable(g, False)
        self.r, self.p = g.correct_reads(self.fq)
        self.ids = list(self.r)
        self.new_offs = np.concatenate([[0], np.cumsum([len(self.r[x]) for x in self.ids])]).astype(np.int64)

    def _sweep_arrays(self, pos):
        from amira_amd import tokenize
        from helpers import flat_positions
        vocab, toks, offs, read_ids = tokenize(self.reads)
        gs, ge = flat_positions(read_ids, self.reads, pos)
        rl = np.asarray([len(self.fq[r]["sequence"]) for r in read_ids], dtype=np.int64)
        return vocab, toks, offs, read_ids, gs, ge, rl

    def oracle(self, k=None):
        """a fresh oracle graph of the corrected reads (its own position lists: correct_reads rewrites them)"""
        from amira_oracle import GeneMerGraph
        return GeneMerGraph(self.r, k or self.k, {x: list(v) for x, v in self.p.items()})

    def arrays(self, g, k=None):
        return oracle_arrays(g, self.vocab, self.ids, self.new_offs, k or self.k)

    def to_derive_ready(self, eng, device=None, pos32=False):
        """the engine alone up to adopt_corrected of the derivable correction.  device: torch tensors (tokens, offsets,
        starts, ends, read lengths) handed over as borrowed device pointers"""
        k = self.k
        if device is not None:
            d = device
            eng.set_reads_device(d[0].data_ptr(), d[1].data_ptr(), len(self.offs) - 1, self.vocab.two_v, borrow=True)
            eng.set_positions_device(d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), borrow=True)
        else:
            eng.set_reads(self.toks, self.offs, self.vocab.two_v)
            if pos32:
                eng.set_positions(self.gs.astype(np.int32), self.ge.astype(np.int32), self.rl)
            else:
                eng.set_positions(self.gs, self.ge, self.rl)
        eng.build(k)
        if self.steps is None:
            eng.filter(3, 1)
            eng.correct_reads()
            eng.adopt_corrected()
            eng.build(k)
            eng.remove_short_linear_paths(k)
        else:
            for step in self.steps:
                assert step[0] in ("filter", "clip", "components")
                {"filter": eng.filter, "clip": eng.remove_short_linear_paths,
                 "components": eng.remove_low_coverage_components}[step[0]](*step[1:])
        n = eng.correct_reads()
        assert n == (len(self.ids), int(self.new_offs[-1]))
        eng.adopt_corrected()

    def to_derived(self, eng, **kw):
        self.to_derive_ready(eng, **kw)
        eng.build(self.k)
        assert eng.counts()["derived"] == 1


_SOURCES = {}


def source(which):
    if which not in _SOURCES:
        _SOURCES[which] = Source(which)
    return _SOURCES[which]


ON = ["both_ends_cut_deep", "seed7"]


@pytest.mark.parametrize("which", ON)
def test_the_derived_graph_is_the_oracles(eng, which):
    """(what every test below starts from)"""
    s = source(which)
    s.to_derived(eng)
    check_graph(eng, s.arrays(s.oracle()))


# ------------------------------------------------------------------ c. the derived graph under every consumer
@pytest.mark.parametrize("which", ON)
def test_component_filter_on_a_derived_graph(eng, which):
    s = source(which)
    s.to_derived(eng)
    g = s.oracle()
    n = [len(g.get_nodes())]
    for m in (5, 10 ** 6):
        eng.remove_low_coverage_components(m)
        g.remove_low_coverage_components(m)
        compare_engine_to_oracle(eng, s.arrays(g), live_only=True)
        n.append(len(g.get_nodes()))
    print("live nodes", n)
    check_corrected(eng, s.vocab, s.ids, *g.correct_reads(s.fq))


@pytest.mark.parametrize("patch", [True, False])
@pytest.mark.parametrize("which", ON)
def test_listed_removals_and_rethreading_on_a_derived_graph(eng, monkeypatch, which, patch):
    """every ninth live node goes, the reads are corrected (re-threaded: the live lists exist now), every ninth of the
    rest goes, corrected again: the lists are brought up to date in place or made again (AMG_NO_LADJ_PATCH=1)"""
    if not patch:
        monkeypatch.setenv("AMG_NO_LADJ_PATCH", "1")
    monkeypatch.setenv("AMG_CORR_ROUTES", "1")
    s = source(which)
    s.to_derived(eng)
    g, g0 = s.oracle(), s.oracle()
    order = list(g.get_nodes())
    first = order[4::9]
    for h in first:
        g.remove_node(g.get_node_by_hash(h))
        g0.remove_node(g0.get_node_by_hash(h))
    eng.remove_nodes(list(range(len(order)))[4::9])
    compare_engine_to_oracle(eng, s.arrays(g), live_only=True)
    check_corrected(eng, s.vocab, s.ids, *g0.correct_reads(s.fq))
    assert eng.correct_routes()["gapped"] > 0
    live = [i for i, h in enumerate(order) if h in g.get_nodes()]
    victims = live[::9]
    assert len(victims) > 5
    for i in victims:
        g.remove_node(g.get_node_by_hash(order[i]))
    eng.remove_nodes(victims)
    compare_engine_to_oracle(eng, s.arrays(g), live_only=True)
    check_corrected(eng, s.vocab, s.ids, *g.correct_reads(s.fq))


@pytest.mark.parametrize("components", [False, True])
@pytest.mark.parametrize("which", ON)
def test_tip_clipping_on_a_derived_graph(eng, monkeypatch, which, components):
    if components:
        monkeypatch.setenv("AMG_CLIP_COMPONENTS", "1")
    s = source(which)
    s.to_derived(eng)
    g = s.oracle()
    order = {h: i for i, h in enumerate(g.get_nodes())}
    total = 0
    for length in (s.k, 2 * s.k):
        got = sorted(eng.remove_short_linear_paths(length).tolist())
        want = sorted(order[h] for h in g.remove_short_linear_paths(length))
        assert got == want, length
        total += len(want)
        compare_engine_to_oracle(eng, s.arrays(g), live_only=True)
    assert total > 0
    check_corrected(eng, s.vocab, s.ids, *g.correct_reads(s.fq))


@pytest.mark.parametrize("which", ON)
def test_match_patterns_on_a_derived_graph(eng, which):
    """amg_match_patterns against find_sublist_indices over every read, tokens and node ids — rows from the oracle"""
    s = source(which)
    s.to_derived(eng)
    want = s.arrays(s.oracle())
    toks = np.asarray([s.vocab.token(x) for r in s.ids for x in s.r[r]], np.int32)
    offs = s.new_offs
    rng = random.Random(3)
    for kind, seq, tail in ((0, toks, 0), (1, want["tok_node"], s.k - 1)):
        rows = [seq[offs[r]:offs[r + 1] - tail].tolist() for r in range(len(s.ids))]
        pats = []
        for _ in range(120):
            row = rows[rng.randrange(len(rows))]
            if len(row) < 2:
                continue
            m = rng.randint(1, min(6, len(row)))
            at = rng.randrange(len(row) - m + 1)
            pats.append(row[at:at + m])
        pats += [[10 ** 6], [rows[0][0], 10 ** 6], []]
        off, hr, hp = eng.match_patterns(kind, pats)
        for j, p in enumerate(pats):
            hits = [(r, i) for r, row in enumerate(rows) for i in range(len(row) - len(p) + 1)
                    if p and row[i:i + len(p)] == p]
            got = list(zip(hr[off[j]:off[j + 1]].tolist(), hp[off[j]:off[j + 1]].tolist()))
            assert got == hits, (kind, j)


@pytest.mark.parametrize("which", ON)
def test_finalize_on_a_derived_graph(eng, which):
    s = source(which)
    s.to_derived(eng)
    eng.finalize()
    g = s.oracle()
    assert eng.counts()["n_components"] == g.get_number_of_component()
    check_graph(eng, s.arrays(g))


# ------------------------------------------------------------------ d. build_filtered on a derive-ready context
@pytest.mark.parametrize("which", ON)
def test_build_filtered_on_a_derive_ready_context(eng, monkeypatch, which):
    """derive, then amg_filter: the live graph is the oracle's GeneMerGraph(...) + filter_graph(3, 1), the correction
    that follows is the oracle's, and both are what a twin gets from build + filter with AMG_NO_DERIVE=1"""
    from amira_amd import Engine
    s = source(which)
    s.to_derive_ready(eng)
    eng.build_filtered(s.k, 3, 1)
    assert eng.counts()["derived"] == 1
    g = s.oracle()
    n0 = len(g.get_nodes())
    g.filter_graph(3, 1)
    assert 0 < len(g.get_nodes()) < n0
    compare_engine_to_oracle(eng, s.arrays(g), live_only=True)
    mine = live_arrays(eng)
    ids, out = check_corrected(eng, s.vocab, s.ids, *g.correct_reads(s.fq))
    twin = Engine(0)
    try:
        monkeypatch.setenv("AMG_NO_DERIVE", "1")
        s.to_derive_ready(twin)
        twin.build(s.k)
        assert twin.counts()["derived"] == 0
        twin.filter(3, 1)
        theirs = live_arrays(twin)
        for key in theirs:
            assert np.array_equal(mine[key], theirs[key]), key
        n = twin.correct_reads()
        other = twin.corrected(*n, True)
        for key in out:
            assert np.array_equal(out[key], other[key]), key
    finally:
        twin.close()


# ------------------------------------------------------------------ e. leaving the derived state
@pytest.mark.parametrize("which", ON + ["circular"])
def test_another_k_on_a_derive_ready_context(eng, which):
    """build(k + 2) is an ordinary build, and the plain build(k) after it (the flag is used up) is one too.  In
    `circular` a derive at k + 2 would pass every check derive_local makes: only the comparison of k stops it"""
    s = source(which)
    s.to_derive_ready(eng)
    for k in (s.k + 2, s.k):
        eng.build(k)
        assert eng.counts()["derived"] == 0 and eng.counts()["k"] == k
        check_graph(eng, s.arrays(s.oracle(k), k))


def test_fresh_reads_after_a_derived_build(eng):
    """table and count hints left by a (small) derived graph must not break the build of a larger read set"""
    from amira_oracle import GeneMerGraph
    source("both_ends_cut_deep").to_derived(eng)
    reads, pos, fq = P.synth_inputs(11, 400, 24, 200, 0.03)
    g1, vocab, ids, offs = sweep_begin(eng, reads, pos, fq, 3)
    c = eng.counts()
    assert c["derived"] == 0 and c["n_nodes"] == len(g1.get_nodes()), f"build_retries {c['build_retries']}"
    print("build_retries", c["build_retries"])
    eng.build(3)                         # nothing adopted: a plain build again
    assert eng.counts()["derived"] == 0
    check_graph(eng, oracle_arrays(GeneMerGraph(reads, 3, pos), vocab, ids, offs, 3))


# ------------------------------------------------------------------ f. borrowed inputs, int32 positions
@pytest.mark.parametrize("how", ["borrowed", "pos32"])
def test_positions_through_a_derived_rebuild(eng, how):
    """the correction that follows the derived build re-threads a read (filter(2, 1) on both_ends_cut_deep): its
    positions — slices of the caller's arrays, cut twice, and carried-over ones — against the oracle"""
    import torch
    s = source("both_ends_cut_deep")
    device = keep = None
    if how == "borrowed":
        device = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (s.toks, s.offs, s.gs, s.ge, s.rl)]
        keep = [t.clone() for t in device]
    s.to_derived(eng, device=device, pos32=how == "pos32")
    g = s.oracle()
    check_graph(eng, s.arrays(g))
    eng.filter(2, 1)
    g.filter_graph(2, 1)
    compare_engine_to_oracle(eng, s.arrays(g), live_only=True)
    assert not DC.predicted_derivable(g, False)
    r3, p3 = g.correct_reads(s.fq)
    ids3, out3 = check_corrected(eng, s.vocab, s.ids, r3, p3)
    assert any(r3[x] != s.r[x] and len(r3[x]) == len(s.r[x]) for x in r3)      # a re-threaded read
    if how == "pos32":
        n = (len(ids3), int(out3["read_offsets"][-1]))
        narrow = eng.corrected(*n, True, pos32=True)
        assert narrow["gene_start"].dtype == np.int32
        for key in out3:
            assert np.array_equal(out3[key], narrow[key]), key
    eng.adopt_corrected()
    eng.build(s.k)
    assert eng.counts()["derived"] == 0
    from amira_oracle import GeneMerGraph
    check_graph(eng, oracle_arrays(GeneMerGraph(r3, s.k, p3), s.vocab, ids3, out3["read_offsets"], s.k))
    if keep is not None:
        torch.cuda.synchronize()
        for a, b in zip(device, keep):
            assert torch.equal(a, b)
