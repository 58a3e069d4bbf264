"""GPU: the two component labellers (ensure_components, amg_adjacency.hip; bx_components_from_claims,
amg_build_x_comp.hip) and what reads their labels, on ARBITRARY graphs: tests/graph_shapes.py turns an edge list into
reads at gene-mer size 1.  The other tests that compare labels cut their reads out of one to four synthetic genomes:
there the run pre-link does nearly all the work, the union-find proper sees a handful of pairs, there are at most four
components and a few thousand nodes.  Here the graphs have 200 000 nodes (all XCDs, three times the grid of
k_comp_hist), up to 130 000 components, deep trees, one contended root, or nothing but runs.

Every check is exact equality: with the sequential C oracle (token_oracle.Sweep) through compare_engine_to_sweep,
which covers labels, the count, adjacency (the star's 70 000-entry row included) and everything else, and with
graph_shapes.labels, which knows nothing of either.  tests/test_graph_shapes_cpu.py holds the three references to
each other.

The union kernels loop until they succeed: a defect there can show as a hang, not as a wrong label."""
import numpy as np
import pytest

import graph_shapes as G
import read_walk_oracle as RW
import token_oracle
from helpers import compare_engine_to_sweep, live_arrays

pytestmark = pytest.mark.gpu


class Frozen:
    """what compare_engine_to_sweep asks of an oracle, read out once: the references are shared between the tests"""

    def __init__(self, s):
        self._c, self._n, self._e = s.counts(), s.nodes(), s.edges()
        self._rn, self._adj, self._fix = s.read_nodes(), s.node_adj(), s.reads_to_correct()

    def counts(self):
        return self._c

    def nodes(self):
        return self._n

    def edges(self):
        return self._e

    def read_nodes(self):
        return self._rn

    def node_adj(self):
        return self._adj

    def reads_to_correct(self):
        return self._fix


class Ref:
    def __init__(self, shape, seed):
        self.shape, self.D = shape, shape.D
        self.tokens = G.shape_tokens(shape, seed)
        self.component, self.n_components = G.labels(shape.D, shape.pairs)
        s = self.sweep()
        self.built = Frozen(s)
        s.close()

    def sweep(self):
        """a C oracle of its own, built, for the tests that go on to change the graph"""
        s = token_oracle.Sweep(*self.tokens)
        s.build(1)
        return s


_REFS = {}


def ref_of(name, D):
    if (name, D) not in _REFS:
        _REFS[name, D] = Ref(G.make(name, D), 100)
    return _REFS[name, D]


@pytest.fixture(scope="module")
def eng():
    from amira_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def check_labels(e, ref, what):
    assert e.counts()["n_nodes"] == ref.D, what
    assert e.counts()["n_components"] == ref.n_components, (what, e.counts()["n_components"], ref.n_components)
    got = e.nodes()["component"]
    bad = np.flatnonzero(got != ref.component)
    assert len(bad) == 0, (what, len(bad), bad[:5], got[bad[:5]], ref.component[bad[:5]])


def build_and_check(e, ref, what):
    e.set_reads(*ref.tokens)
    e.build(1)
    check_labels(e, ref, what)
    compare_engine_to_sweep(e, ref.built, what)


# ------------------------------------------------------------------ the labeller of a plain build
@pytest.mark.parametrize("name,D", G.CASES)
def test_labels_of_arbitrary_graphs(eng, name, D):
    build_and_check(eng, ref_of(name, D), (name, D))


ROUTE_CASES = [(s + "+isolated", G.WORKING_D) for s in G.ROUTE_SHAPES] + [("sparse_random", d) for d in G.SMALL_D]


@pytest.mark.parametrize("name,D", ROUTE_CASES)
def test_fingerprint_keys_same_labels(eng, monkeypatch, name, D):
    ref = ref_of(name, D)
    monkeypatch.setenv("AMG_KEY_MODE", "fp")
    build_and_check(eng, ref, (name, D, "fp"))
    assert eng.counts()["exact_keys"] == 0


def test_same_engine_twice(eng):
    """scratch sized for 66 668 roots serves a graph with one"""
    build_and_check(eng, ref_of("triples", G.WORKING_D), "triples first")
    build_and_check(eng, ref_of("ascending_chain", G.WORKING_D), "one run after 66 668 roots")
    build_and_check(eng, ref_of("triples", 257), "87 roots after one")


# ------------------------------------------------------------------ the labeller of a filtered build (claim space)
@pytest.mark.parametrize("name,D", ROUTE_CASES)
def test_filtered_build_keeps_unfiltered_labels(eng, name, D):
    """build_filtered(1, 2, 1): the nodes that only the prefix names (coverage 1) are never made; the survivors carry
    the labels of the unfiltered graph, and n_components counts the unfiltered graph's components"""
    ref = ref_of(name, D)
    orc = ref.sweep()
    orc.filter(2, 1)
    keep = orc.nodes()["alive"] != 0
    eng.set_reads(*ref.tokens)
    eng.build_filtered(1, 2, 1)
    c = eng.counts()
    assert c["exact_keys"] == 1 and c["n_nodes"] == c["n_live_nodes"] == int(keep.sum())    # only the survivors exist
    if D == G.WORKING_D:
        assert ref.D - int(keep.sum()) >= 1000      # (not the unfiltered case)
    assert c["n_components"] == ref.n_components
    got = eng.nodes()
    assert np.array_equal(got["tokens"][:, 0], ref.D - 1 - np.flatnonzero(keep))    # survivor j is the j-th live node
    assert np.array_equal(got["component"], orc.nodes()["component"][keep])
    assert np.array_equal(got["component"], ref.component[keep])
    a, b = live_arrays(eng), live_arrays(orc)
    for key in b:
        assert np.array_equal(a[key], b[key]), (name, D, key)
    orc.close()


# ------------------------------------------------------------------ merged builds: the labeller on every rank
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name,D", ROUTE_CASES)
def test_merged_build_labels_on_every_rank(name, D, world):
    from amira_amd import Engine
    from amira_amd.dist import dist_build_loopback
    from test_gpu_dist import make_shards
    ref = ref_of(name, D)
    toks, offs, two_v = ref.tokens
    want = ref.built.nodes()
    engines = []
    try:
        for t, o, lo, hi in make_shards(toks, offs, world):
            e = Engine(0)
            e.set_reads(t, o, two_v)
            engines.append(e)
        dist_build_loopback(engines, 1)
        for r, e in enumerate(engines):
            check_labels(e, ref, (name, D, world, r))
            got = e.nodes()
            for key in ("tokens", "coverage", "first_dir", "alive"):
                assert np.array_equal(got[key], want[key]), (name, D, world, r, key)
    finally:
        for e in engines:
            e.close()


# ------------------------------------------------------------------ the consumers, many components, past 65 536 nodes
@pytest.mark.parametrize("name", ["sparse_random", "sparse_random_m3", "triples"])
def test_remove_low_coverage_components(eng, name):
    """k_comp_hist's per-component counters (a thread meets several nodes and several ids: the flush when the id
    changes) and k_kill_low_components with tens of thousands of components of either fate"""
    shape, m = G.low_coverage_case(name)
    tokens = G.shape_tokens(shape, 200)
    orc = token_oracle.Sweep(*tokens)
    orc.build(1)
    orc.remove_low_coverage_components(m)
    eng.set_reads(*tokens)
    eng.build(1)
    eng.remove_low_coverage_components(m)
    compare_engine_to_sweep(eng, orc, (name, m))
    # and without the C oracle: a component lives iff one of its nodes has coverage m or more
    comp, n_comp = G.labels(shape.D, shape.pairs)
    got = eng.nodes()
    assert np.array_equal(got["component"], comp)
    high = np.zeros(n_comp + 1, bool)
    high[comp[got["coverage"] >= m]] = True
    assert np.array_equal(got["alive"] != 0, high[comp])
    kept = int(high.sum())
    assert kept >= n_comp // 10 and n_comp - kept >= n_comp // 4
    orc.close()


@pytest.mark.parametrize("way", ["pristine", "labels", "filtered"])
def test_clip_whole_component_guard(eng, monkeypatch, way):
    """remove_short_linear_paths(4) on the caterpillar with islands (40 001 components): the legs go, an island is
    its whole component and stays.  pristine: the walk's own rows answer, no labels; labels: AMG_CLIP_COMPONENTS=1,
    k_comp_hist feeds comp_live; filtered: after filter(3, 1) comp_live counts live nodes among dead ones"""
    shape, parts = G.clip_case(way == "filtered")
    tokens = G.shape_tokens(shape, 300)
    if way == "labels":
        monkeypatch.setenv("AMG_CLIP_COMPONENTS", "1")
    orc = token_oracle.Sweep(*tokens)
    orc.build(1)
    eng.set_timing(True)
    eng.set_reads(*tokens)
    eng.build(1)
    if way == "filtered":
        orc.filter(3, 1)
        eng.filter(3, 1)
    want = orc.remove_short_linear_paths(G.CLIP_MIN_LENGTH)
    got = eng.remove_short_linear_paths(G.CLIP_MIN_LENGTH)
    stages = [s for s, _ in eng.timings()]
    assert "clip" in stages
    if way == "pristine":
        assert "components" not in stages       # no labels were made for it
    if way == "labels":
        assert "components" in stages
    assert np.array_equal(np.sort(got), np.sort(want))
    compare_engine_to_sweep(eng, orc, way)
    alive = eng.nodes()["alive"] != 0
    legs = np.concatenate([parts["leg_mid"], parts["leg_tip"]])
    assert int(np.isin(got, legs).sum()) >= 10_000 and int(alive[parts["island"]].all(1).sum()) * 2 >= 10_000
    assert not np.isin(got, parts["island"]).any()
    orc.close()


def test_component_amr_reads_with_66668_labels(eng):
    """tests/test_gpu_read_walk.py stops at the LDS slots' component counts and makes a component per read; here 66 668
    labels from a graph whose components are three reads each"""
    ref = ref_of("triples", G.WORKING_D)
    tokens, off, two_v = ref.tokens
    flags = (np.random.default_rng(41).random(ref.D) < 0.1).astype(np.uint8)
    eng.set_reads(*ref.tokens)
    eng.build(1)
    check_labels(eng, ref, "triples")
    nodes = eng.nodes()
    n_reads, n_long = eng.component_amr_reads(flags, 2)
    w_reads, w_long = RW.component_amr_reads(tokens, off, eng.read_node_ids(), nodes["alive"], nodes["component"],
                                             ref.n_components, 1, flags, 2)
    assert np.array_equal(n_reads, w_reads) and np.array_equal(n_long, w_long)
    assert int((w_reads > 0).sum()) > 10_000 and int((w_reads == 0).sum()) > 10_000 and 0 < w_long.sum() < w_reads.sum()
