"""The reference-shaped object view of a device graph: dicts keyed by sha256 node / edge hashes, Node / Edge objects
and per-read lists, made lazily from the device's integer arrays (DESIGN.md "Data layout").

A _View is built from an ARRAY SOURCE — anything with nodes(), edges(), node_adj(), read_node_ids(), read_dirs(),
node_reads() and read_node_ids_of(); in production the Engine — and from plain facts about the reads.  It never sees
the GeneMerGraph that owns it, so it cannot keep that graph alive, and it can be built without a device."""
from collections.abc import Mapping, Sequence

import numpy as np

from .construct_edge import Edge
from .construct_gene import Gene, hashlib_hash
from .construct_gene_mer import GeneMer
from .construct_node import Node
from .io import TokenizedReads


def node_hash_of_tokens(vocab, toks):
    """THE node hash of a row of canonical tokens (a list of ints): the reference's hashlib/pickle recipe over the
    signed gene hashes"""
    signed = vocab.signed_hash
    return hashlib_hash(tuple([signed(t) for t in toks]))


def gene_obj(cache, vocab, token):
    """the Gene object of a token, one per token and graph (`cache` is the graph's, shared with its views)"""
    g = cache.get(token)
    if g is None:
        g = cache[token] = Gene(vocab.gene(token))
    return g


class _RowIndex:
    """read name -> row over ALL reads of a graph, made the first time somebody needs it (shared by the graph and its
    views): the mapping's own table when the reads came as one (same reads, same order)"""
    __slots__ = ("_reads", "_ids", "_table")

    def __init__(self, reads, read_ids):
        self._reads, self._ids, self._table = reads, read_ids, None

    def made(self):
        if self._table is None:
            src, ids = self._reads, self._ids
            same = isinstance(src, TokenizedReads) and len(src.read_ids) == len(ids)
            self._table = src._idx() if same else dict(zip(ids, range(len(ids))))
        return self._table


class _LazyReadLists(Mapping):
    """dict-like {read id: per-window list} over the reads that have a window, whose lists are built
    from the device arrays the first time a read is looked up (read-path clustering touches a few
    thousand of millions).  The key list and the id -> row index are only made when asked for."""

    def __init__(self, view, make):
        self._view, self._make, self._cache = view, make, {}
        self._ids = None       # reads with >= 1 window, in read order (+ reads added by hand)
        self._extra = []       # reads added through add_node_to_read

    def _row(self, rid):
        v = self._view
        r = v._known_rows.get(rid)      # reads the clustering has met already (no name -> row table of ALL reads)
        if r is None:
            r = v._row_index.made().get(rid)
        if r is None:
            return None
        off = v._read_off
        return r if off[r + 1] - off[r] >= v._k else None

    def __getitem__(self, rid):
        got = self._cache.get(rid)
        if got is None:
            r = self._row(rid)
            if r is None:
                raise KeyError(rid)
            got = self._cache[rid] = self._make(r)
        return got

    def __setitem__(self, rid, value):  # remove_node_from_reads / add_node_to_read style updates
        if rid not in self._cache and self._row(rid) is None:   # a read the build did not see (:165-178)
            self._extra.append(rid)
            if self._ids is not None:
                self._ids.append(rid)
        self._cache[rid] = value

    def _keys(self):
        if self._ids is None:
            v = self._view
            rows = np.flatnonzero(np.diff(v._read_off) >= v._k).tolist() if len(v._read_off) > 1 else []
            self._ids = [v._read_ids[r] for r in rows] + self._extra
        return self._ids

    def __iter__(self):
        return iter(self._keys())

    def __len__(self):
        return len(self._keys())

    def __contains__(self, rid):
        return rid in self._cache or self._row(rid) is not None


class _LazyHashes(Sequence):
    """node hashes of the rows of a token matrix, computed on first use (a list from then on)"""

    def __init__(self, token_rows, vocab):
        self._rows, self._vocab, self._made = token_rows, vocab, None

    def _list(self):
        if self._made is None:
            self._made = [node_hash_of_tokens(self._vocab, row) for row in self._rows.tolist()]
            self._rows = None
        return self._made

    def __len__(self):
        return len(self._rows) if self._made is None else len(self._made)

    def __getitem__(self, i):
        return self._list()[i]

    def __iter__(self):
        return iter(self._list())

    def __eq__(self, other):
        return self._list() == (other._list() if isinstance(other, _LazyHashes) else other)

    def __repr__(self):
        return repr(self._list())


def _graph_closed():
    raise RuntimeError("this Node's lists were never looked at while its GeneMerGraph was open, and the graph has been "
                       "closed (its device arrays are gone); read them before close() or keep the graph")


class _GraphNode(Node):
    """Node view whose read list is cut out of the device's node->reads CSR on first use."""

    def _lazy(self, maker):
        self._reads_maker, self._reads_list = maker, None

    @property
    def listOfReads(self):
        if self._reads_list is None:
            self._reads_list = self._reads_maker() if getattr(self, "_reads_maker", None) else []
        return self._reads_list

    @listOfReads.setter
    def listOfReads(self, value):
        self._reads_list = value

    # the forward / backward edge-hash lists are made (and their edges hashed) the first time they are looked at:
    # read-path clustering asks for the neighbours of a few hundred nodes of tens of thousands
    def _lazy_edges(self, forward_maker, backward_maker):
        self._fw_maker, self._bw_maker = forward_maker, backward_maker
        self._fw = self._bw = None

    @property
    def forwardEdgeHashes(self):
        if self._fw is None:
            self._fw = self._fw_maker() if self._fw_maker else []   # (no maker: a node made by hand, add_node)
        return self._fw

    @forwardEdgeHashes.setter
    def forwardEdgeHashes(self, value):
        self._fw = value

    @property
    def backwardEdgeHashes(self):
        if self._bw is None:
            self._bw = self._bw_maker() if self._bw_maker else []
        return self._bw

    @backwardEdgeHashes.setter
    def backwardEdgeHashes(self, value):
        self._bw = value


class _LazyArrays(dict):
    """the arrays of a view by name; those that are big and rarely wanted — the per-window node ids (240 MB per million
    reads), the window directions (60 MB), the node -> reads lists (computed on the device for ALL nodes, 4 bytes per
    window) — are fetched from the array source the first time they are asked for: read-path clustering asks the
    device for the windows of the reads it looks at instead (read_node_ids_of)"""

    FETCHES = {"tok_node": ("read_node_ids", ("tok_node",)), "tok_dir": ("read_dirs", ("tok_dir",)),
               "node_reads_off": ("node_reads", ("node_reads_off", "node_reads")),
               "node_reads": ("node_reads", ("node_reads_off", "node_reads"))}

    def __init__(self, source, *a, **k):
        super().__init__(*a, **k)
        self.source = source   # (None once the view's graph is closed)

    def __missing__(self, key):
        if key not in self.FETCHES or self.source is None:
            raise KeyError(key)
        fetch, names = self.FETCHES[key]
        got = getattr(self.source, fetch)()
        self.update(zip(names, got if len(names) > 1 else (got,)))
        return dict.__getitem__(self, key)


class _HashToId:
    """{node hash: device node id} over the nodes of a view; hashes the view has not made yet are settled by making
    every node (see _View)."""

    __slots__ = ("_view",)

    def __init__(self, view):
        self._view = view

    def get(self, h, default=None):
        v = self._view
        i = v._id_of.get(h)
        if i is None and not v._nodes_complete:
            v.nodes   # (makes them all)
            i = v._id_of.get(h)
        return default if i is None else i

    def __getitem__(self, h):
        i = self.get(h)
        if i is None:
            raise KeyError(h)
        return i

    def __contains__(self, h):
        return self.get(h) is not None


class _View:
    """Reference-shaped object view of the device graph (see module docstring).  Node objects (a sha256 and a dozen
    small objects each) and Edge objects (two sha256 each) are made when somebody looks at them — read-path
    clustering touches the few thousand nodes its genes' reads run through, of tens of thousands: one by one through
    node_at / hash_at / node_by_hash and a node's edge lists, all of them — in the reference's insertion order — the
    first time the node / edge dict itself is asked for."""

    __slots__ = ("_nodes", "_nodes_complete", "_node_obj", "_id_of", "node_of_hash", "_edges", "_edges_complete",
                 "_edge_obj", "_n_edges", "readNodes", "readNodeDirections", "readNodePositions", "node_hash",
                 "edge_hash", "alive", "arrays", "_nh_table", "_vocab", "_k", "_read_ids", "_read_off", "_positions",
                 "_known_rows", "_row_index", "_gene_cache", "_single_rows")

    def __init__(self, source, vocab, k, read_ids, read_off, positions, known_rows, row_index, gene_cache):
        """positions: the flat (gene starts, gene ends) aligned with the tokens, or None; known_rows / row_index: the
        two name -> row lookups of the per-read lists, the cheap one first (a dict, a _RowIndex)"""
        self._vocab, self._k, self._read_ids, self._read_off, self._positions = vocab, k, read_ids, read_off, positions
        self._known_rows, self._row_index, self._gene_cache = known_rows, row_index, gene_cache
        nodes, edges = source.nodes(), source.edges()
        adj_off, adj_edge = source.node_adj()
        self.arrays = _LazyArrays(source, {"nodes": nodes, "edges": edges, "adj_off": adj_off, "adj_edge": adj_edge})
        D, E = len(nodes["coverage"]), len(edges["coverage"])
        self.alive = nodes["alive"]
        self.node_hash, self._node_obj, self._nh_table = [None] * D, [None] * D, None
        self._nodes, self._nodes_complete, self._id_of = {}, False, {}
        self.node_of_hash = _HashToId(self)
        self.edge_hash, self._edge_obj = [None] * E, [None] * E
        self._edges, self._edges_complete, self._n_edges = {}, False, E
        self._single_rows = 0
        self.readNodes = _LazyReadLists(self, self._read_nodes)
        self.readNodeDirections = _LazyReadLists(self, self._read_dirs)
        self.readNodePositions = _LazyReadLists(self, self._read_positions)

    def dispose(self):
        """called when the graph is closed: let go of the array source and cut the view's reference cycles (its lists
        and nodes point back at it) so that it is freed the moment its graph lets go of it, not when the cyclic
        collector next walks the heap"""
        self.arrays.source = self.node_of_hash = None
        self.readNodes = self.readNodeDirections = self.readNodePositions = None
        for node in self._nodes.values():   # (the nodes made so far)
            if isinstance(node, _GraphNode):
                # lists that were looked at stay as they are; the others can no longer be made: say so instead of
                # answering with an empty list
                node._reads_maker = node._fw_maker = node._bw_maker = _graph_closed
        self._node_obj, self._edge_obj = [], []

    # ---- nodes
    def _note_hash(self, i, h):
        self.node_hash[i] = h
        self._id_of[h] = i
        if self._nh_table is not None:
            self._nh_table[i] = h

    def _hash_node(self, i):
        if not self.alive[i]:
            return None
        h = node_hash_of_tokens(self._vocab, self.arrays["nodes"]["tokens"][i].tolist())
        self._note_hash(i, h)
        return h

    def _make_node(self, i):
        if not self.alive[i]:
            return None
        nodes, vocab, cache, flip = self.arrays["nodes"], self._vocab, self._gene_cache, self._vocab.flip
        toks = nodes["tokens"][i].tolist()
        canon = [gene_obj(cache, vocab, t) for t in toks]
        rc = [gene_obj(cache, vocab, flip(t)) for t in reversed(toks)]
        h = self.node_hash[i]
        if h is None:
            h = node_hash_of_tokens(vocab, toks)
        node = _GraphNode(GeneMer._from_parts(canon, rc, int(nodes["first_dir"][i]), h))
        node.nodeCoverage = int(nodes["coverage"][i])
        node._component_ID = int(nodes["component"][i])
        node._lazy(lambda: self._reads_of_node(i))
        node._amg_id = i
        adj_off = self.arrays["adj_off"]
        lo, mid, hi = int(adj_off[2 * i]), int(adj_off[2 * i + 1]), int(adj_off[2 * i + 2])
        node._lazy_edges(lambda: self._edge_list(lo, mid), lambda: self._edge_list(mid, hi))
        self._node_obj[i] = self._nodes[h] = node
        self._note_hash(i, h)
        return node

    def _reads_of_node(self, i):
        a, read_ids = self.arrays, self._read_ids
        return [read_ids[r] for r in a["node_reads"][a["node_reads_off"][i]:a["node_reads_off"][i + 1]].tolist()]

    def _edge_list(self, lo, hi):
        """hashes of the live edges among adj_edge[lo:hi]: a node's forward list, or its backward list"""
        alive = self.arrays["edges"]["alive"]
        return [self.edge_hash_of(e) for e in self.arrays["adj_edge"][lo:hi].tolist() if alive[e]]

    def node_at(self, i):
        """the node with device id i (None: removed)"""
        if self._nodes_complete:
            h = self.node_hash[i]
            return None if h is None else self._nodes[h]
        node = self._node_obj[i]
        return node if node is not None else self._make_node(i)

    def hash_at(self, i):
        h = self.node_hash[i]
        if h is None and not self._nodes_complete:
            h = self._hash_node(i)
        return h

    def ensure_hashes(self, ids):
        """node_hash[i] filled in for every id >= 0 of `ids` (an iterable of ints) — the hash alone (one sha256 of the
        node's tokens); the Node object with its genes is made when somebody asks for the node itself"""
        if self._nodes_complete:
            return
        nh, hash_node = self.node_hash, self._hash_node
        for i in ids:
            if i >= 0 and nh[i] is None:
                hash_node(i)

    @property
    def nodes(self):
        if not self._nodes_complete:
            ordered = {}
            for i in range(len(self.node_hash)):
                node = self.node_at(i)
                if node is not None:
                    ordered[self.node_hash[i]] = node
            self._nodes, self._nodes_complete = ordered, True
        return self._nodes

    def node_by_hash(self, h, default=None):
        got = self._nodes.get(h)
        if got is None and not self._nodes_complete:
            i = self._id_of.get(h)          # hashed already (ensure_hashes), object not made yet
            got = self.node_at(i) if i is not None else self.nodes.get(h)
        return default if got is None else got

    def node_hash_table(self, ids=None):
        """node hashes as an object array indexed by device node id, two None entries at the end (ids -2 and -1:
        a window without a node); with `ids` (an int array) only those entries are promised"""
        if not self._nodes_complete:
            if ids is None:
                self.nodes
            else:
                self.ensure_hashes(np.unique(ids).tolist())
        if self._nh_table is None:
            t = np.empty(len(self.node_hash) + 2, dtype=object)
            t[:len(self.node_hash)] = self.node_hash
            self._nh_table = t
        return self._nh_table

    # ---- edges
    def _make_edge(self, e):
        edges = self.arrays["edges"]
        edge = Edge(self.node_at(int(edges["src"][e])), self.node_at(int(edges["tgt"][e])),
                    int(edges["sdir"][e]), int(edges["tdir"][e]))
        edge.edgeCoverage = int(edges["coverage"][e])
        edge._amg_id = e
        return edge

    def edge_hash_of(self, e):
        h = self.edge_hash[e]
        if h is None:
            edge = self._edge_obj[e] = self._make_edge(e)
            h = self.edge_hash[e] = edge.__hash__()
            self._edges[h] = edge
        return h

    @property
    def edges(self):
        if not self._edges_complete:
            alive = self.arrays["edges"]["alive"]
            ordered = {}
            for e in range(self._n_edges):
                if alive[e]:
                    h = self.edge_hash_of(e)
                    ordered[h] = self._edge_obj[e]
            self._edges, self._edges_complete = ordered, True
        return self._edges

    def edge_by_hash(self, h):
        got = self._edges.get(h)
        return got if got is not None else self.edges[h]

    # ---- per-read lists (the makers of readNodes, readNodeDirections, readNodePositions; r is a read's row)
    def window_ids(self, r):
        """(first token, number of windows, node id per window) of a read"""
        offs, arrays = self._read_off, self.arrays
        a, n = int(offs[r]), int(offs[r + 1] - offs[r]) - self._k + 1
        if n > 0 and self._single_rows < 64 and not dict.__contains__(arrays, "tok_node"):
            # the first few reads somebody looks up are gathered on the device one by one (read-path clustering asks
            # for one read per allele); whoever keeps asking gets the whole per-window array, once
            self._single_rows += 1
            return a, n, arrays.source.read_node_ids_of([a], [n])[0].tolist()
        return a, n, arrays["tok_node"][a:a + n].tolist()   # (fetched on first use)

    def _read_nodes(self, r):
        _, _, ids = self.window_ids(r)
        self.ensure_hashes(ids)
        nh = self.node_hash
        return [nh[x] if x >= 0 else None for x in ids]

    def _read_dirs(self, r):
        a, n, ids = self.window_ids(r)
        return [d if x >= 0 else None for d, x in zip(self.arrays["tok_dir"][a:a + n].tolist(), ids)]

    def _read_positions(self, r):
        a, n, ids = self.window_ids(r)
        if self._positions is None:
            return [None] * n
        k = self._k
        s, e = self._positions[0][a:a + n].tolist(), self._positions[1][a + k - 1:a + k - 1 + n].tolist()
        return [(s[j], e[j]) if ids[j] >= 0 else None for j in range(n)]
