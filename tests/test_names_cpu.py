"""The rule of the 256-bit node / edge names (amira_amd/csrc/amg_names.h) without a device: the host twin amg_names_host
against pickle + hashlib + hash() (tests/names_oracle.py) on the boundaries of pickle's integer encodings and of SHA's
padding, edge names composed from node names, the agreement check of the Python layer, the refusals, and an object
view that takes its names in bulk from a source (served by the host twin here) against the same view without one."""
import functools

import numpy as np
import pytest

import names_oracle as O
import procedures as P
from helpers import oracle_arrays
from test_graph_view_cpu import Source

def host(table, rows, protocol=None):
    from amira_amd.names import names_host
    return names_host(table, rows, protocol)


rows_of = O.boundary_rows


@pytest.mark.parametrize("protocol", O.PROTOCOLS)
@pytest.mark.parametrize("k", O.KS)
def test_host_twin_equals_pickle_and_hashlib_on_the_boundary_vocabulary(k, protocol):
    rows, want, want_hash = O.boundary_case(k, protocol)
    assert len(rows) == (2500 if k == 2 else 5000)
    digests, py_hash = host(O.boundary_table(), rows, protocol)
    bad = np.flatnonzero((digests != want).any(axis=1))
    assert len(bad) == 0, (k, protocol, rows[bad[0]].tolist())
    assert np.array_equal(py_hash, want_hash)


@pytest.mark.parametrize("protocol", O.PROTOCOLS)
def test_rows_cover_the_lengths_where_the_padding_takes_another_block(protocol):
    """by pickle itself: the messages of the rows at k = 3, 4, 5 have lengths of every residue around SHA's padding
    boundary (55 is the last length whose padding fits the block; 63, 0, 1 are around a full block)"""
    values = O.MAGNITUDES
    signed = [-v for v in reversed(values)] + values
    seen = set()
    for k in (3, 4, 5):
        for row in rows_of(k).tolist():
            seen.add(O.message_length([signed[t] for t in row], protocol) % 64)
    assert {54, 55, 56, 57, 63, 0, 1} <= seen
    assert len(seen) == 64


@functools.lru_cache(maxsize=None)
def real_vocabulary():
    from amira_amd.tokens import Vocabulary
    return Vocabulary([f"gene{i}" for i in range(300)])


def test_a_real_vocabulary_at_k_5():
    v = real_vocabulary()
    table = v.digest_bytes()
    assert table.shape == (300, 32) and [int.from_bytes(r.tobytes(), "big") for r in table] == v.hashes
    rows = O.random_rows(7, v.two_v, 2000, 5)
    digests, py_hash = host(table, rows)
    want, want_hash = O.names_of_rows(v.hashes, rows)
    assert np.array_equal(digests, want) and np.array_equal(py_hash, want_hash)
    from amira_amd.graph_view import node_hash_of_tokens
    for row, d in zip(rows[:50].tolist(), digests[:50]):
        assert node_hash_of_tokens(v, row) == int.from_bytes(d.tobytes(), "big")


def test_from_ranked_keeps_the_loaders_digests():
    from amira_amd.tokens import Vocabulary
    v = real_vocabulary()
    given = v.digest_bytes().copy()
    again = Vocabulary.from_ranked(v.names, given)
    assert np.array_equal(again.digest_bytes(), given) and again.hashes == v.hashes


def test_edge_names_compose_from_node_names():
    """an edge's name is the smaller of two k = 2 rows over the table of NODE names: (s, t) and (-s, -t)"""
    from amira_amd.construct_edge import Edge
    v = real_vocabulary()
    node_rows = O.random_rows(11, v.two_v, 40, 3)
    node_digests, _ = host(v.digest_bytes(), node_rows)
    names = [int.from_bytes(d.tobytes(), "big") for d in node_digests]
    rng = np.random.default_rng(3)
    n = 500
    src, tgt = rng.integers(0, 40, n), rng.integers(0, 40, n)
    src[:20] = tgt[:20]                                   # self loops
    sdir, tdir = rng.choice([-1, 1], n), rng.choice([-1, 1], n)
    V = len(names)
    tok = lambda i, d: np.where(d > 0, V + i, V - 1 - i)  # noqa: E731
    pairs = np.stack([tok(src, sdir), tok(tgt, tdir)], -1).astype(np.int32)
    flipped = np.stack([tok(src, -sdir), tok(tgt, -tdir)], -1).astype(np.int32)
    a, _ = host(node_digests, pairs)
    b, _ = host(node_digests, flipped)   # (a table is any list of digests: it need not be in rank order)

    class N:
        def __init__(self, h):
            self.h = h

        def __hash__(self):
            return self.h

    for i in range(n):
        got = min(a[i].tobytes(), b[i].tobytes())
        assert got == O.edge_name(names[src[i]], names[tgt[i]], int(sdir[i]), int(tdir[i]))
        want = Edge(N(names[src[i]]), N(names[tgt[i]]), int(sdir[i]), int(tdir[i])).__hash__()
        assert int.from_bytes(got, "big") == want


def test_names_ok_on_this_interpreter():
    from amira_amd.names import names_ok
    assert names_ok() is True


def test_refusals():
    from amira_amd import _ffi
    table = O.boundary_table()
    V = len(table)

    def call(table, n_genes, protocol, rows, k):
        rows = np.ascontiguousarray(rows, np.int32)
        n = len(rows) // max(k, 1) if rows.ndim == 1 else len(rows)
        d, h = np.zeros((max(n, 1), 32), np.uint8), np.zeros(max(n, 1), np.int64)
        return _ffi.lib.amg_names_host(_ffi.ptr(table), n_genes, protocol, _ffi.ptr(rows), n, k, _ffi.ptr(d), _ffi.ptr(h))

    good = np.zeros((2, 3), np.int32)
    assert call(table, V, 4, good, 3) == 0
    assert call(table, V, 3, good, 3) == _ffi.E_ARG            # protocol 3
    assert call(table, V, 6, good, 3) == _ffi.E_ARG
    assert call(table, 0, 4, good, 3) == _ffi.E_ARG            # no genes
    assert call(table, V, 4, np.zeros(4, np.int32), 0) == _ffi.E_ARG            # k = 0
    assert call(table, V, 4, np.zeros((1, 257), np.int32), 257) == _ffi.E_ARG   # k = 257
    assert call(table, V, 4, np.zeros((1, 256), np.int32), 256) == 0
    bad = good.copy()
    bad[1, 2] = 2 * V                                          # a token of 2V
    assert call(table, V, 4, bad, 3) == _ffi.E_ARG
    bad[1, 2] = -1
    assert call(table, V, 4, bad, 3) == _ffi.E_ARG
    bad[1, 2] = 2 * V - 1
    assert call(table, V, 4, bad, 3) == 0


# ---------------------------------------------------------------- the object view with names in bulk
class NamingSource(Source):
    """the stub array source of tests/test_graph_view_cpu.py with node_names / edge_names served by the host twin, as the
    device serves them: zeros for what is not alive"""

    def __init__(self, arr, vocab, **dead):
        super().__init__(arr, **dead)
        self.table = vocab.digest_bytes()
        self.V = vocab.V

    def node_names(self, ids):
        self.calls.append("node_names")
        ids = np.asarray(ids, np.int64)
        digests, py_hash = host(self.table, self.arr["tokens"][ids])
        dead = self.node_alive[ids] == 0
        digests[dead], py_hash[dead] = 0, 0
        return digests, py_hash

    def edge_names(self, ids):
        self.calls.append("edge_names")
        ids = np.asarray(ids, np.int64)
        a = self.arr
        ends = np.concatenate([a["src"][ids], a["tgt"][ids]])
        names, _ = host(self.table, a["tokens"][ends])
        n = len(ids)
        idx = np.arange(n)

        def rows(flip):
            s = np.where(a["sdir"][ids] * flip > 0, 2 * n + idx, 2 * n - 1 - idx)
            t = np.where(a["tdir"][ids] * flip > 0, 2 * n + n + idx, 2 * n - 1 - (n + idx))
            return np.stack([s, t], -1).astype(np.int32)

        if n == 0:
            return np.zeros((0, 32), np.uint8), np.zeros(0, np.int64)
        one, h1 = host(names, rows(1))
        two, h2 = host(names, rows(-1))
        first = np.asarray([x.tobytes() < y.tobytes() for x, y in zip(one, two)])
        digests, py_hash = np.where(first[:, None], one, two), np.where(first, h1, h2)
        dead = self.edge_alive[ids] == 0
        digests[dead], py_hash[dead] = 0, 0
        return digests, py_hash


@functools.lru_cache(maxsize=None)
def _case(name, k):
    from amira_amd.tokens import tokenize
    from amira_oracle import GeneMerGraph as Oracle
    calls, pos = P.fixture(name)
    vocab, _, offs, ids = tokenize(calls)
    o = Oracle(dict(calls), k, {r: list(v) for r, v in pos.items()})
    return oracle_arrays(o, vocab, ids, offs, k), vocab, ids, offs, calls


def _views(name, k, monkeypatch, **dead):
    from amira_amd import graph_view
    from amira_amd.graph_view import _RowIndex, _View
    arr, vocab, ids, offs, calls = _case(name, k)
    monkeypatch.setattr(graph_view, "NAMES_BATCH_MIN", 8)
    monkeypatch.setattr(graph_view, "NAMES_ONE_BY_ONE", 8)
    plain = _View(Source(arr, **dead), vocab, k, ids, offs, None, {}, _RowIndex(calls, ids), {})
    src = NamingSource(arr, vocab, **dead)
    named = _View(src, vocab, k, ids, offs, None, {}, _RowIndex(calls, ids), {})
    return plain, named, src, arr


@pytest.mark.parametrize("name,k", [("eight", 3), ("nine", 5)])
def test_a_view_named_in_bulk_equals_the_view_named_on_the_host(name, k, monkeypatch):
    arr = _case(name, k)[0]
    dead_nodes = set(range(0, len(arr["coverage"]), 7))
    dead_edges = set(range(0, len(arr["src"]), 5)) | {
        e for e in range(len(arr["src"])) if int(arr["src"][e]) in dead_nodes or int(arr["tgt"][e]) in dead_nodes}
    plain, named, src, arr = _views(name, k, monkeypatch, dead_nodes=dead_nodes, dead_edges=dead_edges)
    assert plain._names_source is None and named._names_source is src
    D = len(arr["coverage"])
    live = [i for i in range(D) if i not in dead_nodes]
    # ---- a few single asks stay on the host, a batch goes to the source, dead nodes and ids -1 / -2 stay None
    assert named.hash_at(live[0]) == plain.hash_at(live[0]) and named.names_from_device == 0
    some = np.asarray(live[1:40:2] + sorted(dead_nodes)[:3] + [-1, -2], np.int64)
    t_named, t_plain = named.node_hash_table(some), plain.node_hash_table(some)
    assert t_named[some].tolist() == t_plain[some].tolist()
    assert t_named[-1] is None and t_named[-2] is None and all(t_named[i] is None for i in sorted(dead_nodes)[:3])
    assert named.names_from_device == len(live[1:40:2]) and "node_names" in src.calls
    assert [named.node_of_hash[t_plain[i]] for i in live[1:40:2]] == live[1:40:2]
    # ---- hash() of the names without the ints: the source's own py_hash
    ids = np.asarray(live[::3] + live[:5], np.int64)
    assert named.py_hash_of(ids).tolist() == [hash(plain.hash_at(i)) for i in ids.tolist()]
    assert plain.py_hash_of(ids).tolist() == named.py_hash_of(ids).tolist()
    # ---- edge lists of single nodes (a handful of edges each: the host recipe), then everything
    for i in live[:6]:
        assert named.node_at(i).get_forward_edge_hashes() == plain.node_at(i).get_forward_edge_hashes()
        assert named.node_at(i).get_backward_edge_hashes() == plain.node_at(i).get_backward_edge_hashes()
    assert list(named.nodes) == list(plain.nodes) and list(named.edges) == list(plain.edges)
    assert "edge_names" in src.calls
    for h, want in plain.nodes.items():
        got = named.nodes[h]
        assert got.get_forward_edge_hashes() == want.get_forward_edge_hashes()
        assert got.get_backward_edge_hashes() == want.get_backward_edge_hashes()
        assert got._amg_id == want._amg_id
    for h, want in plain.edges.items():
        got = named.edge_by_hash(h)
        assert got is named.edges[h] and got._amg_id == want._amg_id and got.__hash__() == h
    assert list(named.readNodes) == list(plain.readNodes)
    for rid in plain.readNodes:
        assert named.readNodes[rid] == plain.readNodes[rid]
    assert named.node_hash == plain.node_hash and named.edge_hash == plain.edge_hash
    assert all(named.node_hash[i] is None for i in dead_nodes) and all(named.edge_hash[e] is None for e in dead_edges)
    assert plain.names_from_device == 0 and named.names_from_device > 0


def test_a_fresh_view_takes_every_name_from_the_source(monkeypatch):
    plain, named, src, arr = _views("eight", 3, monkeypatch)
    assert list(named.edges) == list(plain.edges)            # edges first: their names need no Node or Edge object
    D, E = len(arr["coverage"]), len(arr["src"])
    assert src.calls.count("edge_names") == 1
    h = plain.edge_hash[E // 2]
    assert named.edge_by_hash(h)._amg_id == E // 2
    assert list(named.nodes) == list(plain.nodes)
    alone = D - len(np.unique(np.concatenate([arr["src"], arr["tgt"]])))   # nodes without an edge: named with `nodes`,
    assert 0 < alone < 8                                                   # too few of them for a call of their own
    assert named.names_from_device == D + E - alone


def test_many_single_asks_end_in_one_call_for_all_that_is_left(monkeypatch):
    plain, named, src, arr = _views("eight", 3, monkeypatch)
    D = len(arr["coverage"])
    for i in range(9):
        assert named.hash_at(i) == plain.hash_at(i)
    assert named.names_from_device == 0 and "node_names" not in src.calls
    assert named.hash_at(9) == plain.hash_at(9)              # more than NAMES_ONE_BY_ONE by now: every live node left
    assert src.calls.count("node_names") == 1 and named.names_from_device == D - 9
    assert all(named.node_hash[i] == plain.hash_at(i) for i in range(D)) and not named._nodes_complete


def test_the_switch_keeps_a_view_on_the_host(monkeypatch):
    monkeypatch.setenv("AMG_NAMES_ON_HOST", "1")
    plain, named, src, _ = _views("eight", 3, monkeypatch)
    assert named._names_source is None
    assert list(named.nodes) == list(plain.nodes) and list(named.edges) == list(plain.edges)
    assert named.names_from_device == 0 and not {"node_names", "edge_names"} & set(src.calls)
