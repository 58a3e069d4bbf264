"""The reference-shaped object view of a device graph: dicts keyed by sha256 node / edge hashes, Node / Edge objects
and per-read lists, made lazily from the device's integer arrays (DESIGN.md "Data layout").

A _View is built from an ARRAY SOURCE — anything with nodes(), edges(), node_adj(), read_node_ids(), read_dirs(),
node_reads() and read_node_ids_of(); in production the Engine — and from plain facts about the reads.  It never sees
the GeneMerGraph that owns it, so it cannot keep that graph alive, and it can be built without a device."""
import os
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


# Where naming on the device overtakes the host recipe (tools/names_probe.py, profiles/names_host_vs_device.json; DESIGN.md
# section 4): a batch of at least NAMES_BATCH_MIN unnamed nodes or edges is named in one device call, smaller asks keep
# the host recipe; once a view has named more than NAMES_ONE_BY_ONE of them one by one, the next ask names every live one
# still unnamed in one call (the policy window_ids has for rows).  Measured on an MI355X: a call for 64 ids costs 83 us
# (nodes) / 105 us (edges) against 103 / 100 us of hashing them on the host, for 128 ids 88 / 110 us against 209 / 204 us,
# and the device stays below from there on; 128 is the first power of two at which it is below for both kinds.
NAMES_BATCH_MIN = 128
NAMES_ONE_BY_ONE = 128


def ints_of_digests(digests):
    """the rows of a uint8 [n, 32] array as Python ints (big-endian)"""
    raw, from_bytes = digests.tobytes(), int.from_bytes
    return [from_bytes(raw[a:a + 32], "big") for a in range(0, len(raw), 32)]


def hashes_of_token_rows(vocab, rows, row_names=None):
    """node hashes of the rows of a token matrix: from NAMES_BATCH_MIN rows on in one device call when there is a namer
    (row_names: rows -> (digests, py_hash), or None when it cannot serve), else one by one on the host"""
    if row_names is not None and len(rows) >= NAMES_BATCH_MIN:
        got = row_names(rows)
        if got is not None:
            return ints_of_digests(got[0])
    return [node_hash_of_tokens(vocab, row) for row in rows.tolist()]


class NamedSource:
    """an array source (the Engine) with the gene table of one vocabulary bound to its naming calls: what a
    GeneMerGraph hands its views, so that they can name nodes and edges in bulk"""

    def __init__(self, engine, names):
        self._engine, self._names = engine, names

    def __getattr__(self, name):
        return getattr(self._engine, name)

    def node_names(self, ids):
        return self._engine.node_names(self._names, ids)

    def edge_names(self, ids):
        return self._engine.edge_names(self._names, ids)

    def row_names(self, rows):
        return self._engine.names_probe(self._names, rows)


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

    def __init__(self, token_rows, vocab, row_names=None):
        self._rows, self._vocab, self._made, self._row_names = token_rows, vocab, None, row_names

    def _list(self):
        if self._made is None:
            self._made = hashes_of_token_rows(self._vocab, self._rows, self._row_names)
            self._rows = self._row_names = None
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
                 "_known_rows", "_row_index", "_gene_cache", "_single_rows", "_names_source", "names_from_device",
                 "_one_by_one", "_edge_id_of", "_py_hash", "_py_known")

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
        # naming in bulk: a source that offers node_names(ids) / edge_names(ids) -> (digests uint8 [n, 32], py_hash int64
        # [n]) names batches (NAMES_BATCH_MIN); one without them, or AMG_NAMES_ON_HOST=1 when the view is made, keeps
        # the host recipe for every name
        named = hasattr(source, "node_names") and hasattr(source, "edge_names")
        self._names_source = source if named and os.environ.get("AMG_NAMES_ON_HOST") != "1" else None
        self.names_from_device = 0       # names (nodes and edges) this view took from the device
        self._one_by_one = [0, 0]        # nodes, edges named on the host so far
        self._edge_id_of = {}            # edge hash -> device edge id, of the edges hashed so far
        self._py_hash, self._py_known = None, None   # hash() of the node hashes by device id (py_hash_of)
        self.readNodes = _LazyReadLists(self, self._read_nodes)
        self.readNodeDirections = _LazyReadLists(self, self._read_dirs)
        self.readNodePositions = _LazyReadLists(self, self._read_positions)

    def dispose(self):
        """called when the graph is closed: let go of the array source and cut the view's reference cycles (its lists
        and nodes point back at it) so that it is freed the moment its graph lets go of it, not when the cyclic
        collector next walks the heap"""
        self.arrays.source = self.node_of_hash = self._names_source = None
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
        """the host recipe for one node"""
        if not self.alive[i]:
            return None
        h = node_hash_of_tokens(self._vocab, self.arrays["nodes"]["tokens"][i].tolist())
        self._note_hash(i, h)
        return h

    def _names_from_device(self, ids, by_rows):
        """the names of the live nodes `ids` in one device call, as ints, or None when the device does not hold the
        graph this view was made of any more (a live node came back without a name).  by_rows: from the view's own
        token rows (ids the device may have removed since)"""
        src = self._names_source
        if by_rows:
            digests, py = src.row_names(self.arrays["nodes"]["tokens"][ids])
        else:
            digests, py = src.node_names(np.asarray(ids, np.int32))
        if len(ids) and not digests.any(axis=1).all():
            return None
        if self._py_hash is None:
            self._py_hash, self._py_known = np.zeros(len(self.node_hash), np.int64), np.zeros(len(self.node_hash), bool)
        self._py_hash[ids], self._py_known[ids] = py, True
        self.names_from_device += len(ids)
        return ints_of_digests(digests)

    def _name_batch(self, kind, todo, host_one, device_many, all_unnamed):
        """the policy of both kinds of names (kind 0: nodes, 1: edges) for `todo`, distinct live ids without a name:
        one device call from NAMES_BATCH_MIN on, the host recipe below — until the view has named more than
        NAMES_ONE_BY_ONE that way, when every live id still unnamed is named in one call"""
        if not todo:
            return
        if self._names_source is not None:
            if len(todo) < NAMES_BATCH_MIN and self._one_by_one[kind] > NAMES_ONE_BY_ONE and all_unnamed is not None:
                todo = all_unnamed()
            if (len(todo) >= NAMES_BATCH_MIN or self._one_by_one[kind] > NAMES_ONE_BY_ONE) and device_many(todo):
                return
        self._one_by_one[kind] += len(todo)
        for i in todo:
            host_one(i)

    def _device_nodes(self, todo, by_rows=False):
        got = self._names_from_device(todo, by_rows)
        if got is None:
            return False
        note = self._note_hash
        for i, h in zip(todo, got):
            note(i, h)
        return True

    def _make_node(self, i):
        if not self.alive[i]:
            return None
        nodes, vocab, cache, flip = self.arrays["nodes"], self._vocab, self._gene_cache, self._vocab.flip
        toks = nodes["tokens"][i].tolist()
        canon = [gene_obj(cache, vocab, t) for t in toks]
        rc = [gene_obj(cache, vocab, flip(t)) for t in reversed(toks)]
        h = self.node_hash[i]
        if h is None:
            self._name_nodes((i,))
            h = self.node_hash[i]
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
        live = [e for e in self.arrays["adj_edge"][lo:hi].tolist() if alive[e]]
        self.ensure_edge_hashes(live)
        eh = self.edge_hash
        return [eh[e] for e in live]

    def node_at(self, i):
        """the node with device id i (None: removed)"""
        if self._nodes_complete:
            h = self.node_hash[i]
            return None if h is None else self._nodes[h]
        node = self._node_obj[i]
        return node if node is not None else self._make_node(i)

    def hash_at(self, i):
        h = self.node_hash[i]
        if h is None and not self._nodes_complete and self.alive[i]:
            self._name_nodes((i,))
            h = self.node_hash[i]
        return h

    def _name_nodes(self, ids, removed_since=False):
        nh, alive = self.node_hash, self.alive
        todo = list(dict.fromkeys(i for i in ids if i >= 0 and nh[i] is None and alive[i]))
        if removed_since:
            self._name_batch(0, todo, self._hash_node, lambda t: self._device_nodes(t, True), None)
        else:
            self._name_batch(0, todo, self._hash_node, self._device_nodes,
                             lambda: [i for i in np.flatnonzero(alive).tolist() if nh[i] is None])

    def ensure_hashes(self, ids, removed_since=False):
        """node_hash[i] filled in for every id >= 0 of `ids` (an iterable of ints) — the hash alone; the Node object
        with its genes is made when somebody asks for the node itself.  A batch of NAMES_BATCH_MIN ids or more is
        named in one device call where the source offers one (_name_batch).  removed_since: the device may have
        removed nodes of `ids` since the view was made (tip clipping's answer): they are named from the view's rows"""
        if self._nodes_complete:
            return
        self._name_nodes(ids, removed_since)

    def py_hash_of(self, ids):
        """int64 array: Python's hash() of the node hash of every id of `ids` (live nodes), without making the big
        ints where the names come from the device"""
        ids = np.asarray(ids, np.int64)
        self.ensure_hashes(np.unique(ids).tolist())
        if self._py_hash is None:
            self._py_hash, self._py_known = np.zeros(len(self.node_hash), np.int64), np.zeros(len(self.node_hash), bool)
        new = np.unique(ids[~self._py_known[ids]])
        if len(new):
            nh = self.node_hash
            self._py_hash[new] = [hash(nh[i]) for i in new.tolist()]
            self._py_known[new] = True
        return self._py_hash[ids]

    @property
    def nodes(self):
        if not self._nodes_complete:
            self._name_nodes(range(len(self.node_hash)))
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

    def _hash_edge(self, e):
        """the host recipe for one edge: the Edge object of its two Node objects, and its __hash__"""
        edge = self._edge_obj[e] = self._make_edge(e)
        h = self.edge_hash[e] = edge.__hash__()
        self._edges[h] = edge
        self._edge_id_of[h] = e

    def _device_edges(self, todo):
        """edge_hash filled for the live edges `todo` from one device call: no Edge, no Node object is made for it"""
        digests, _ = self._names_source.edge_names(np.asarray(todo, np.int32))
        if not digests.any(axis=1).all():
            return False   # (the device holds another graph by now: see _names_from_device)
        eh, id_of = self.edge_hash, self._edge_id_of
        for e, h in zip(todo, ints_of_digests(digests)):
            eh[e] = h
            id_of[h] = e
        self.names_from_device += len(todo)
        return True

    def ensure_edge_hashes(self, ids):
        """edge_hash[e] filled in for every LIVE edge of `ids`: in one device call for NAMES_BATCH_MIN edges or more
        where the source offers one (_name_batch), else edge by edge from the objects"""
        eh, alive = self.edge_hash, self.arrays["edges"]["alive"]
        todo = list(dict.fromkeys(e for e in ids if eh[e] is None and alive[e]))
        self._name_batch(1, todo, self._hash_edge, self._device_edges,
                         lambda: [e for e in np.flatnonzero(alive).tolist() if eh[e] is None])

    def edge_hash_of(self, e):
        h = self.edge_hash[e]
        if h is None:
            self.ensure_edge_hashes((e,))
            h = self.edge_hash[e]
        return h

    def _edge_at(self, e):
        """the Edge object of the live, hashed edge e (made on first use)"""
        edge = self._edge_obj[e]
        if edge is None:
            edge = self._edge_obj[e] = self._make_edge(e)
            self._edges.setdefault(self.edge_hash[e], edge)
        return edge

    @property
    def edges(self):
        if not self._edges_complete:
            alive = self.arrays["edges"]["alive"]
            live = np.flatnonzero(alive).tolist()
            self.ensure_edge_hashes(live)
            ends = self.arrays["edges"]
            self._name_nodes(np.unique(np.concatenate([ends["src"][live], ends["tgt"][live]])).tolist())  # (the objects' nodes)
            eh, ordered = self.edge_hash, {}
            for e in live:
                ordered[eh[e]] = self._edge_at(e)
            self._edges, self._edges_complete = ordered, True
        return self._edges

    def edge_by_hash(self, h):
        got = self._edges.get(h)
        if got is None:
            e = self._edge_id_of.get(h)   # hashed already (on the device: no object yet)
            got = self._edge_at(e) if e is not None else self.edges[h]
        return got

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
