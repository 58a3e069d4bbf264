"""GPU: the 256-bit names of nodes and edges made on the device (amg_node_names, amg_edge_names, amg_names_probe;
amira_amd/csrc/amg_names.hip) against pickle + hashlib + hash() (tests/names_oracle.py): arbitrary rows over the
boundaries of pickle's integer encodings through the probe, the nodes and edges of built graphs, dead ids, refusals,
and GeneMerGraph named on the device against the same graph named on the host."""
import functools

import numpy as np
import pytest

import names_oracle as O
import procedures as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from amira_amd import Engine
    e = Engine(0)
    yield e
    e.close()


@functools.lru_cache(maxsize=None)
def boundary_names(protocol):
    from amira_amd.engine import GeneNames
    return GeneNames(O.boundary_table(), 0, protocol)


def assert_names(got, want_digests, want_hash, what):
    digests, py_hash = got
    assert digests.shape == want_digests.shape and digests.dtype == np.uint8 and py_hash.dtype == np.int64
    bad = np.flatnonzero((digests != want_digests).any(axis=1))
    assert len(bad) == 0, (what, "first of", len(bad), "at", int(bad[0]))
    assert np.array_equal(py_hash, want_hash), what


@pytest.mark.parametrize("protocol", O.PROTOCOLS)
@pytest.mark.parametrize("k", O.KS)
def test_probe_on_the_boundary_vocabulary(eng, k, protocol):
    rows, want, want_hash = O.boundary_case(k, protocol)
    assert_names(eng.names_probe(boundary_names(protocol), rows), want, want_hash, (k, protocol))


@pytest.mark.parametrize("k", (2, 5, 17))
def test_probe_row_counts_and_chunks(eng, k):
    """a lone lane, a wave less one, a full wave, a wave and one, a workgroup and one (idle lanes in the last wave and
    the last workgroup); three chunks with a short last one"""
    protocol = O.PROTOCOLS[0]
    rows, want, want_hash = O.boundary_case(k, protocol)
    names = boundary_names(protocol)
    for n in (0, 1, 63, 64, 65, 257):
        assert_names(eng.names_probe(names, rows[:n]), want[:n], want_hash[:n], (k, n))
    assert_names(eng.names_probe(names, rows[:257], chunk_names=100), want[:257], want_hash[:257], (k, "chunks"))
    assert_names(eng.names_probe(names, rows[:257], chunk_names=257), want[:257], want_hash[:257], (k, "one chunk"))


def test_probe_real_vocabulary(eng):
    from amira_amd.tokens import Vocabulary
    v = Vocabulary([f"gene{i}" for i in range(300)])
    rows = O.random_rows(7, v.two_v, 10000, 5)
    want, want_hash = O.names_of_rows(v.hashes, rows)
    assert_names(eng.names_probe(v.gene_names(0), rows), want, want_hash, "300 names")
    assert v.gene_names(0) is v.gene_names(0)


def test_probe_refusals(eng):
    from amira_amd import _ffi
    from amira_amd.engine import GeneNames
    names = boundary_names(4)
    V = len(O.MAGNITUDES)
    for rows in (np.zeros((3, 257), np.int32), np.full((3, 4), 2 * V, np.int32), np.full((3, 4), -1, np.int32)):
        with pytest.raises(_ffi.AmgError) as err:
            eng.names_probe(names, rows)
        assert err.value.code == _ffi.E_ARG
    for n_genes, protocol in ((0, 4), (V, 3), (V, 6)):
        with pytest.raises(_ffi.AmgError) as err:
            GeneNames(O.boundary_table()[:n_genes], 0, protocol)
        assert err.value.code == _ffi.E_ARG


# ---------------------------------------------------------------- built graphs
@functools.lru_cache(maxsize=None)
def read_set():
    """400 synthetic reads of 30 genes, and four reads that repeat one gene (either strand) often enough to give a node
    an edge to itself at every k of this file"""
    from amira_amd.tokens import tokenize
    reads, _, _ = P.synth_inputs(7, 400, 30, 300, 0.03)
    reads = dict(reads)
    genes = [g[1:] for g in next(iter(reads.values()))[:2]]
    reads["loop_a"], reads["loop_b"] = ["+" + genes[0]] * 20, ["-" + genes[1]] * 20
    reads["loop_c"], reads["loop_d"] = ["+" + genes[0]] * 18, ["-" + genes[1]] * 18
    vocab, toks, offs, _ = tokenize(reads)
    return reads, vocab, toks, offs


@functools.lru_cache(maxsize=None)
def graph_oracle(k):
    """(nodes, edges, node digests, node hashes, edge digests, edge hashes) of the unfiltered graph at k: the engine's
    arrays named by pickle + hashlib (made on the first GPU case of a k, shared, never changed)"""
    from amira_amd import Engine
    _, vocab, toks, offs = read_set()
    e = Engine(0)
    try:
        e.set_reads(toks, offs, vocab.two_v)
        e.build(k)
        nodes, edges = e.nodes(), e.edges()
    finally:
        e.close()
    nd, nh = O.names_of_rows(vocab.hashes, nodes["tokens"])
    ints = [int.from_bytes(d.tobytes(), "big") for d in nd]
    raw = [O.edge_name(ints[s], ints[t], sd, td) for s, t, sd, td in zip(
        edges["src"].tolist(), edges["tgt"].tolist(), edges["sdir"].tolist(), edges["tdir"].tolist())]
    ed = np.frombuffer(b"".join(raw), np.uint8).reshape(len(raw), 32).copy()
    eh = np.asarray([hash(int.from_bytes(d, "big")) for d in raw], np.int64)
    return nodes, edges, nd, nh, ed, eh


@pytest.mark.parametrize("k", (3, 5, 15))
def test_nodes_and_edges_of_a_graph(eng, k):
    from amira_amd import _ffi
    from amira_amd.engine import GeneNames
    _, vocab, toks, offs = read_set()
    nodes, edges, nd, nh, ed, eh = graph_oracle(k)
    D, E = len(nd), len(ed)
    assert D > 100 and E > 100
    assert (edges["src"] == edges["tgt"]).any()                                      # a node with an edge to itself
    assert {(1, 1), (1, -1), (-1, 1), (-1, -1)} <= set(zip(edges["sdir"].tolist(), edges["tdir"].tolist()))
    names = vocab.gene_names(0)
    eng.set_reads(toks, offs, vocab.two_v)
    eng.build(k)
    assert np.array_equal(eng.nodes()["tokens"], nodes["tokens"]) and np.array_equal(eng.edges()["src"], edges["src"])
    assert_names(eng.node_names(names), nd, nh, "all nodes")
    assert_names(eng.edge_names(names), ed, eh, "all edges")
    rng = np.random.default_rng(k)
    for n_all, call, wd, wh in ((D, eng.node_names, nd, nh), (E, eng.edge_names, ed, eh)):
        for ids in (np.arange(n_all - 1, -1, -1), rng.integers(0, n_all, 700), np.asarray([5, 5, 0, 5, n_all - 1]),
                    np.zeros(0, np.int64)):
            assert_names(call(names, ids), wd[ids], wh[ids], (call.__name__, len(ids)))
    # ---- refusals leave the graph as it was
    before = eng.counts()
    other = GeneNames(vocab.digest_bytes()[:-1], 0)
    for call, n_all in ((eng.node_names, D), (eng.edge_names, E)):
        for bad, handle in (([0, n_all], names), ([-1], names), ([0], other)):
            with pytest.raises(_ffi.AmgError) as err:
                call(handle, np.asarray(bad))
            assert err.value.code == _ffi.E_ARG
        with pytest.raises(_ffi.AmgError) as err:
            call(other)
        assert err.value.code == _ffi.E_ARG
    other.close()
    assert eng.counts() == before and np.array_equal(eng.nodes()["alive"], nodes["alive"])
    assert_names(eng.node_names(names, [3, 1]), nd[[3, 1]], nh[[3, 1]], "after the refusals")
    # ---- after a filter: zeros exactly at the dead ids
    eng.filter(3, 1)
    n_alive, e_alive = eng.nodes()["alive"] != 0, eng.edges()["alive"] != 0
    assert 0 < n_alive.sum() < D and 0 < e_alive.sum() < E
    for got, alive, wd, wh in ((eng.node_names(names), n_alive, nd, nh), (eng.edge_names(names), e_alive, ed, eh)):
        assert_names(got, np.where(alive[:, None], wd, 0).astype(np.uint8), np.where(alive, wh, 0), "after filter(3, 1)")
    some = rng.integers(0, E, 300)
    assert_names(eng.edge_names(names, some), np.where(e_alive[some, None], ed[some], 0).astype(np.uint8),
                 np.where(e_alive[some], eh[some], 0), "ids after filter(3, 1)")


def _object_view(monkeypatch, on_host):
    from amira_amd import GeneMerGraph
    reads, _, _, _ = read_set()
    if on_host:
        monkeypatch.setenv("AMG_NAMES_ON_HOST", "1")
    else:
        monkeypatch.delenv("AMG_NAMES_ON_HOST", raising=False)
    with GeneMerGraph(dict(reads), 5) as g:
        nodes, edges = list(g.get_nodes()), list(g.get_edges())
        lists = [(n.get_forward_edge_hashes(), n.get_backward_edge_hashes()) for n in g.get_nodes().values()]
        read_nodes = {r: list(v) for r, v in g.get_readNodes().items()}
        return nodes, edges, lists, read_nodes, g.names_from_device


def test_gene_mer_graph_named_on_the_device_equals_named_on_the_host(monkeypatch):
    host = _object_view(monkeypatch, True)
    device = _object_view(monkeypatch, False)
    assert host[4] == 0
    assert device[4] > 0          # (without that the comparison shows nothing)
    for a, b, what in zip(host[:4], device[:4], ("nodes", "edges", "edge lists", "readNodes")):
        assert a == b, what
    assert len(host[0]) > 100 and len(host[1]) > 100
