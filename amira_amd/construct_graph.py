"""GeneMerGraph — drop-in for amira/construct_graph.py (reference v0.11.0) on MI355X.

Same constructor, accessors and passes as the reference class; the work is done by
libamg.so (HIP, gfx950) through amira_amd.engine:

    __init__                          amg_set_reads / amg_set_positions / amg_build
    __init__(..., _filter=(n, m))     amg_build_filtered (= __init__ + filter_graph in one device pass)
    filter_graph                      amg_filter
    remove_node & friends             amg_remove_nodes
    remove_short_linear_paths         amg_remove_short_linear_paths
    remove_low_coverage_components    amg_remove_low_coverage_components
    correct_reads                     amg_correct_reads (+ amg_get_corrected)
    remove_junk_reads,
    get_valid_reads_only              amg_select_reads

The device keeps the graph as integer arrays (DESIGN.md "Data layout").  The reference's
object API (dicts keyed by 256-bit sha256 hashes, Node / Edge objects, per-read lists) is a
VIEW that is materialised lazily from those arrays the first time an accessor needs it and
dropped whenever a device pass changes the graph.  Hashes are computed on the host with the
reference's own hashlib/pickle recipe, once per distinct node / edge.

There is no CPU build path: constructing a graph without libamg.so or without a HIP device
raises.  Host-side methods only do what the reference also does in Python on top of a
built graph (unitig gene strings, linear-path walks, anchor / block logic of the read-path
clustering).

Layout: this module keeps the build and build_many, close and pickling, the pass runner (_run_pass: a device
pass is called, logged and replayed by its Engine method name), the accessors, the incremental mutators, topology,
the removals and the filter.  The object view (_View, built from arrays, never from a graph) is graph_view.py; the
rest are mixins, one concern each: read_correction.ReadCorrection, graph_paths.PathsAndOutput (gene strings, GML,
linear paths, coverages, components), read_clustering.ReadClustering, bubble_popping.BubblePopping.
"""
import os
import statistics
import sys

import numpy as np

from . import _ffi
from .bubble_popping import BubblePopping
from .construct_edge import Edge
from .construct_read import Read  # noqa: F401  (re-exported like the reference)
from .engine import Engine, _ENGINE_POOL, acquire_engine as _acquire_engine, release_engine as _release_engine  # noqa: F401
from .graph_paths import PathsAndOutput
from .graph_view import (NamedSource, _GraphNode, _LazyHashes, _RowIndex, _View, hashes_of_token_rows,  # noqa: F401
                         node_hash_of_tokens)
from .io import TokenizedPositions, TokenizedReads
from .read_clustering import ReadClustering
from .read_correction import ReadCorrection
from .tokens import tokenize

sys.setrecursionlimit(50000)  # construct_graph.py:27


def _flat_positions(positions):
    """flat (gene starts, gene ends) of a TokenizedPositions: int64, or int32 as they are (amg_set_positions32)"""
    keep32 = positions.gene_start.dtype == np.int32 and positions.gene_end.dtype == np.int32
    dtype = np.int32 if keep32 else np.int64
    return np.ascontiguousarray(positions.gene_start, dtype), np.ascontiguousarray(positions.gene_end, dtype)


def _palindrome_as_assertion(err):
    """an engine error of a build, as the reference reports it (construct_gene_mer.py:23-25)"""
    if err.code == _ffi.E_PALINDROME:
        return AssertionError("Gene-mer and reverse complement gene-mer are identical")
    return err


class GeneMerGraph(BubblePopping, ReadCorrection, PathsAndOutput, ReadClustering):
    # ------------------------------------------------------------------ build
    def __init__(self, readDict, kmerSize, gene_positions=None, device=None, _filter=None):
        """_filter = (minNodeCoverage, minEdgeCoverage): the graph comes out as GeneMerGraph(...).filter_graph(...)
        would leave it, with the filter applied during the build (amg_build_filtered; graph_utils.build_filtered_graph)"""
        self._init_fields(readDict, kmerSize, gene_positions, device)
        if isinstance(readDict, TokenizedReads):
            readDict = readDict.settled()   # (reads replaced by hand — bubble popping — are spelled into the arrays)
        on_device = readDict.device_source() if isinstance(readDict, TokenizedReads) else None
        if on_device is not None and on_device.engine().device == self._engine.device:
            # the output of a correct_reads that never left the GPU: taken over device to device, positions included
            # when they come from the same correction (amira_amd.io.DeviceCorrected)
            ids = readDict.read_ids
            self._vocab, self._read_off, self._read_ids = readDict.vocab, readDict.read_offsets, (ids if isinstance(ids, list) else list(ids))
            self._engine.set_reads_from_corrected(on_device.engine())
            same = isinstance(gene_positions, TokenizedPositions) and gene_positions.device_source() is on_device
            if not same:
                self._host_positions(gene_positions)
                self._upload_positions()
        else:
            self._upload_reads(readDict, gene_positions)
        try:
            if _filter is None:
                self._engine.build(self._kmer_for_device())
            else:
                self._build_filter = (int(_filter[0]), int(_filter[1]))
                self._minNodeCoverage, self._minEdgeCoverage = _filter
                self._engine.build_filtered(self._kmer_for_device(), max(int(_filter[0]), 0), max(int(_filter[1]), 0))
        except _ffi.AmgError as err:
            raise _palindrome_as_assertion(err) from None
        self._note_short_reads()

    def _upload_reads(self, readDict, gene_positions):
        """tokenise the reads (unless they came as arrays) and hand them and their positions to the engine"""
        if isinstance(readDict, TokenizedReads):
            r = readDict
            self._vocab, toks, offs, self._read_ids = r.vocab, r.tokens, r.read_offsets, list(r.read_ids)
        else:
            self._vocab, toks, offs, self._read_ids = tokenize(readDict)
        self._read_off, self._tokens_val = offs, toks
        self._engine.set_reads(toks, offs, self._vocab.two_v)
        self._host_positions(gene_positions)
        self._upload_positions()

    @classmethod
    def build_many(cls, readDict, kmerSizes, gene_positions=None, device=None):
        """[GeneMerGraph(readDict, k, gene_positions) for k in kmerSizes] — the seven graphs of choose_kmer_size
        (graph_utils.py:258-296) — with the reads tokenised and uploaded ONCE (amg_build_multi: every graph is built by
        the ordinary build on an engine of its own; the graphs after the first read the first one's device arrays and
        keep it alive)."""
        kmerSizes = list(kmerSizes)
        first = cls.__new__(cls)
        first._init_fields(readDict, kmerSizes[0], gene_positions, device)
        first._upload_reads(readDict, gene_positions)
        graphs = [first]
        for k in kmerSizes[1:]:
            g = cls.__new__(cls)
            g._init_fields(readDict, k, gene_positions, device)
            g._vocab, g._read_ids, g._read_off, g._tokens_val = (first._vocab, first._read_ids, first._read_off,
                                                                 first._tokens_val)
            g._read_index_ = first._read_index_
            g._gs_val, g._ge_val = first._gs, first._ge
            g._positions_pending = g._gs_val is not None   # uploaded when a correction asks for them
            g._reads_owner = first
            first._borrowers += 1
            graphs.append(g)
        try:
            Engine.build_multi([g._engine for g in graphs], [g._kmer_for_device() for g in graphs])
        except _ffi.AmgError as err:
            for g in graphs:
                g.close()
            raise _palindrome_as_assertion(err) from None
        for g in graphs:
            g._note_short_reads()
        return graphs

    def _init_fields(self, readDict, kmerSize, gene_positions, device):
        self._reads = readDict
        self._kmerSize = kmerSize
        self._minNodeCoverage = 1
        self._minEdgeCoverage = 1
        self._genePositions = gene_positions
        self._view = None
        self._names_taken = 0      # names taken from the device by views dropped since and outside views (names_from_device)
        self._host_edits = False   # add_node / add_edge / remove_edge ... changed the host view
        self._lone_edges = set()   # directed edges removed one at a time (remove_edge) on the device
        self._known_rows = {}      # read name -> row for the reads the native clustering has looked at
        self._pass_log = []        # device passes applied since the build, in order (replayed by __setstate__)
        self._build_filter = None  # _filter of the build
        self._extra_to_correct = set()
        self._gene_cache = {}
        self._read_index_ = None
        self._tokens_val = self._gs_val = self._ge_val = None   # host copies: see the properties below
        self._positions_pending = False
        self._reads_owner = None   # build_many: the graph whose engine holds the reads this one's engine borrows
        self._borrowers = 0        # build_many: graphs that borrow this one's reads
        self._close_pending = False
        dev = int(os.environ.get("AMG_DEVICE", "0")) if device is None else int(device)
        self._engine = _acquire_engine(dev)

    def _kmer_for_device(self):
        # GeneMerGraph({}, 0) is legal in the reference: nothing to build
        return 1 if (self._kmerSize < 1 and int(self._read_off[-1]) == 0) else self._kmerSize

    # host copies of the genes and their positions: made at once when the caller handed dicts or host arrays over, on
    # first use when the reads came straight from another graph's correction on the device
    @property
    def _tokens(self):
        if self._tokens_val is None:
            self._tokens_val = self._reads.tokens
        return self._tokens_val

    def _positions_from_mapping(self):
        if self._gs_val is None and isinstance(self._genePositions, TokenizedPositions) \
                and self._genePositions.as_made() and self._genePositions._gs is not None:
            self._gs_val, self._ge_val = _flat_positions(self._genePositions)

    @property
    def _gs(self):
        self._positions_from_mapping()
        return self._gs_val

    @property
    def _ge(self):
        self._positions_from_mapping()
        return self._ge_val

    def _host_positions(self, gene_positions):
        """flat int64 (start, end) per gene, aligned with the tokens"""
        offs = self._read_off
        if isinstance(gene_positions, TokenizedPositions):
            gene_positions = gene_positions.settled()   # (redirected / hand-set reads gathered into arrays of their own)
            self._gs_val, self._ge_val = _flat_positions(gene_positions)
            assert len(self._gs_val) == int(offs[-1]) == len(self._ge_val), "positions do not match the gene calls"
        elif gene_positions:
            n = int(offs[-1])
            gs, ge = np.empty(n, np.int64), np.empty(n, np.int64)
            for r, rid in enumerate(self._read_ids):
                a, b = int(offs[r]), int(offs[r + 1])
                if b > a:
                    p = gene_positions[rid]
                    # Read.get_geneMers indexes positions[i] / positions[i + k - 1] (construct_read.py:48-52)
                    gs[a:b] = [x[0] for x in p[: b - a]]
                    ge[a:b] = [x[1] for x in p[: b - a]]
            self._gs_val, self._ge_val = gs, ge

    def _upload_positions(self):
        if self._gs_val is not None:
            self._engine.set_positions(self._gs_val, self._ge_val, None)
        self._positions_pending = False

    def _note_short_reads(self):
        offs = self._read_off
        short = np.flatnonzero(np.diff(offs) < self._kmerSize).tolist() if len(offs) > 1 else []
        self._shortReads = {self._read_ids[r]: self._reads[self._read_ids[r]] for r in short}   # :53-55

    def _row_index(self):
        if self._read_index_ is None:
            self._read_index_ = _RowIndex(self._reads, self._read_ids)
        return self._read_index_

    @property
    def _read_index(self):
        return self._row_index().made()

    def close(self):
        """hand the device engine back (the graph can no longer be queried); also done when the object dies"""
        view, self._view = getattr(self, "_view", None), None
        if view is not None:
            view.dispose()
        owner, self._reads_owner = getattr(self, "_reads_owner", None), None
        if getattr(self, "_borrowers", 0) > 0:   # graphs of build_many still read this one's device arrays
            self._close_pending = True
            return
        engine, self._engine = getattr(self, "_engine", None), None
        _release_engine(engine)   # (pooled once no correct_reads output lives in its buffers any more)
        if owner is not None:
            owner._borrowers -= 1
            if owner._borrowers == 0 and getattr(owner, "_close_pending", False):
                owner.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass

    # ------------------------------------------------------------------ pickling (graph_utils.py:108-122: loky workers
    # hand whole GeneMerGraph objects back to the parent)
    def __getstate__(self):
        """What travels is what the graph was made FROM — the reads and positions (array-backed mappings fetch what
        still lives on the device), the gene-mer size, the filter of a filtered build — and the device passes
        applied since, in order.  The device arrays themselves stay behind: every pass is deterministic, so the
        receiving process builds the graph on its own GPU and replays the passes (__setstate__)."""
        if self._host_edits:
            raise TypeError("a GeneMerGraph edited by hand (add_node / add_edge / ...) lives in host objects of this "
                            "process only and cannot be pickled")
        for obj in (self._reads, self._genePositions):
            if isinstance(obj, TokenizedReads):
                obj.tokens          # noqa: B018  (fetches a DeviceCorrected)
            elif isinstance(obj, TokenizedPositions):
                obj.gene_start      # noqa: B018
        # the positions the graph was BUILT with: correct_reads replaces the positions of the reads it changes in the
        # caller's mapping (:1282-1284, :1328) while the graph keeps its reads, so the mapping as it is now may no
        # longer match them; the flat arrays made at construction do
        gs, ge = self._gs_val, self._ge_val
        if gs is None and isinstance(self._genePositions, TokenizedPositions):
            self._genePositions._from_device()
            gs, ge = self._genePositions._gs, self._genePositions._ge
        return {"reads": self._reads, "k": self._kmerSize, "positions": self._genePositions, "built_with": (gs, ge),
                "filter": self._build_filter, "passes": list(self._pass_log),
                "min_cov": (self._minNodeCoverage, self._minEdgeCoverage), "device": self._engine.device,
                "extra_to_correct": set(self._extra_to_correct), "lone_edges": set(self._lone_edges)}

    def __setstate__(self, state):
        gs, ge = state["built_with"]
        reads = state["reads"]
        built_with = None
        if gs is not None:
            ids = reads.read_ids if isinstance(reads, TokenizedReads) else list(reads)
            offs = reads.read_offsets if isinstance(reads, TokenizedReads) else None
            if offs is None:
                offs = np.zeros(len(ids) + 1, np.int64)
                np.cumsum([len(reads[r]) for r in ids], out=offs[1:])
            built_with = TokenizedPositions(ids, offs, gs, ge)
        self.__init__(reads, state["k"], built_with, device=state.get("device"), _filter=state["filter"])
        self._genePositions = state["positions"]
        for name, args in state["passes"]:   # (the log's names are Engine method names: _run_pass)
            getattr(self._engine, name)(*args)
        self._pass_log = list(state["passes"])
        self._minNodeCoverage, self._minEdgeCoverage = state["min_cov"]
        self._extra_to_correct = set(state["extra_to_correct"])
        self._lone_edges = set(state.get("lone_edges", ()))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ------------------------------------------------------------------ view plumbing
    def _invalidate(self):
        if self._view is not None:
            self._names_taken += self._view.names_from_device
        self._view = None

    @property
    def names_from_device(self):
        """node and edge names this graph took from the device in bulk so far (the others were hashed on the host)"""
        return self._names_taken + (self._view.names_from_device if self._view is not None else 0)

    def _names_source(self):
        """the engine with the vocabulary's gene table bound to its naming calls (what views name batches with), or the
        bare engine where the device's names cannot be relied on: an interpreter whose pickle or hash() differ from the
        restated recipe (amira_amd.names.names_ok), a vocabulary without genes"""
        from .names import names_ok
        make = getattr(self._vocab, "gene_names", None)
        names = make(self._engine.device) if make is not None and names_ok() else None
        return self._engine if names is None else NamedSource(self._engine, names)

    def _row_namer(self):
        """rows of tokens -> (digests, py_hash) in one device call, for hashes that are made without a view; answers
        None once the graph is closed (the caller then hashes on the host), None itself under AMG_NAMES_ON_HOST=1"""
        if os.environ.get("AMG_NAMES_ON_HOST") == "1":
            return None

        def namer(rows):
            if getattr(self, "_engine", None) is None:
                return None
            source = self._names_source()
            if not isinstance(source, NamedSource):
                return None
            self._names_taken += len(rows)
            return source.row_names(rows)
        return namer

    def _settle_leases(self):
        """What an earlier correct_reads of this graph left on the device (amira_amd.io.DeviceCorrected: the lazy
        mappings it handed back) is brought to the host before a pass that changes the graph: every such pass
        invalidates the engine's corrected set (amg_filter, amg_remove_nodes, amg_remove_short_linear_paths,
        amg_remove_low_coverage_components, amg_correct_reads), and the mappings must keep answering afterwards as
        the reference's dicts do."""
        for lease in list(self._engine._leases):
            lease.fetch()

    def _device_pass(self, what):
        """The incremental mutators of the reference class (add_node, add_edge, remove_edge,
        remove_node_from_reads, ... — used by its unit tests and its multi-process merge) edit the
        HOST view only; the device arrays no longer describe that graph, so device passes refuse it."""
        if self._host_edits:
            raise RuntimeError(f"{what}: this graph was edited through add_node / add_edge / remove_edge on the "
                               "host; build a GeneMerGraph from reads to run device passes")
        self._settle_leases()

    def _run_pass(self, name, *args):
        """Run the device pass Engine.<name>(*args) and log it as (name, args), which is what __setstate__ replays.
        Leases are settled here; a pass that refuses a hand-edited graph calls _device_pass itself, first thing, so that
        it refuses before it does anything else.  Dropping the view is the caller's business."""
        self._settle_leases()
        result = getattr(self._engine, name)(*args)
        self._pass_log.append((name, args))
        return result

    def _hash_of_tokens(self, toks):
        return node_hash_of_tokens(self._vocab, toks)

    def _v(self):
        if self._view is None:
            gs = self._gs
            self._view = _View(self._names_source(), self._vocab, self._kmerSize, self._read_ids, self._read_off,
                               None if gs is None else (gs, self._ge), self._known_rows, self._row_index(),
                               self._gene_cache)
        return self._view

    def _node_arrays(self):
        """the node arrays: the view's if there is one, else fetched from the engine"""
        return self._view.arrays["nodes"] if self._view is not None else self._engine.nodes()

    def _node_id(self, node_or_hash):
        h = node_or_hash if isinstance(node_or_hash, int) else node_or_hash.__hash__()
        return self._v().node_of_hash[h]

    # ------------------------------------------------------------------ accessors (:104-163)
    def get_reads(self):
        return self._reads

    def get_short_read_annotations(self):
        return self._shortReads

    def get_gene_positions(self):
        return self._genePositions

    def get_short_read_gene_positions(self):
        return {r: self._genePositions[r] for r in self._shortReads}

    def get_readNodes(self):
        return self._v().readNodes

    def get_readNodeDirections(self):
        return self._v().readNodeDirections

    def get_readNodePositions(self):
        return self._v().readNodePositions

    def get_kmerSize(self):
        return self._kmerSize

    def get_minEdgeCoverage(self):
        return self._minEdgeCoverage

    def get_minNodeCoverage(self):
        return self._minNodeCoverage

    def set_minNodeCoverage(self, minNodeCoverage):
        self._minNodeCoverage = minNodeCoverage
        return self._minNodeCoverage

    def set_minEdgeCoverage(self, minEdgeCoverage):
        self._minEdgeCoverage = minEdgeCoverage
        return self._minEdgeCoverage

    def get_nodes(self):
        return self._v().nodes

    def get_edges(self):
        return self._v().edges

    def get_reads_to_correct(self):
        flags = self._engine.reads_to_correct()
        out = {self._read_ids[r] for r in np.nonzero(flags)[0].tolist()}
        out |= self._extra_to_correct
        return out

    def all_nodes(self):
        for h in self.get_nodes():
            yield self.get_nodes()[h]

    def get_reads_for_nodes(self, list_of_nodes):
        reads = set()
        for h in list_of_nodes:
            reads.update(self.get_node_by_hash(h).get_list_of_reads())
        return reads

    def get_nodes_containing_read(self, readId):
        v = self._v()
        found = [v.node_by_hash(h) for h in self.get_readNodes()[readId] if h is not None]
        return [n for n in found if n is not None]

    def get_node_by_hash(self, nodeHash):
        node = self._v().node_by_hash(nodeHash)
        if node is None:
            raise KeyError(nodeHash)
        return node

    def get_node(self, geneMer):
        node = self._v().node_by_hash(geneMer.__hash__())
        assert node is not None, "This gene-mer is not in the graph"
        return node

    def get_edge_by_hash(self, edgeHash):
        return self._v().edge_by_hash(edgeHash)

    def get_total_number_of_nodes(self):
        return self._engine.counts()["n_live_nodes"]

    def get_total_number_of_edges(self):
        return self._engine.counts()["n_live_edges"]

    def get_total_number_of_reads(self):
        return len(self._reads)

    def get_nodes_containing(self, geneOfInterest):
        """nodes whose canonical gene-mer holds the gene, in node order (:223-244)."""
        assert not (geneOfInterest[0] == "+" or geneOfInterest[0] == "-"), (
            "Strand information cannot be present for any specified genes")
        assert isinstance(geneOfInterest, str), "Gene of interest is the wrong type"
        v = self._v()
        ids = self._node_ids_containing([geneOfInterest])
        return [v.node_at(i) for i in ids]

    def _node_ids_containing(self, genes):
        v = self._v()
        toks = []
        for g in genes:
            r = self._vocab.rank.get(g)
            if r is not None:
                V = max(self._vocab.V, 1)
                toks += [V + r, V - 1 - r]
        nt = v.arrays["nodes"]["tokens"]
        if not toks or nt.size == 0:
            return []
        mask = np.isin(nt, np.asarray(toks, dtype=nt.dtype)).any(axis=1) & (v.alive != 0)
        return np.nonzero(mask)[0].tolist()

    # ------------------------------------------------------------------ incremental construction (:165-324)
    # The reference builds its graph through these calls; here the device builds it and they remain
    # for callers that edit a graph by hand (the reference's unit tests, its multi-process merge).
    # They work on the materialised host view and switch the graph to host-only (_device_pass).
    def add_node_to_read(self, node, readId, node_direction, node_position=None):
        v = self._v()
        self._host_edits = True
        if readId not in v.readNodes:
            v.readNodes[readId], v.readNodeDirections[readId], v.readNodePositions[readId] = [], [], []
        v.readNodes[readId].append(node.__hash__())
        v.readNodeDirections[readId].append(node_direction)
        v.readNodePositions[readId].append(node_position)
        return v.readNodes[readId]

    def add_node_to_nodes(self, node, nodeHash):
        self._host_edits = True
        self._v().nodes[nodeHash] = node

    def add_node(self, geneMer, reads):
        """insert-or-find by hash; the first GeneMer object seen stays on the node (:196-212)"""
        nodes = self._v().nodes
        h = geneMer.__hash__()
        node = nodes.get(h)
        if node is None:
            node = _GraphNode(geneMer)
            node._lazy(None)
            node.listOfReads = []
            self.add_node_to_nodes(node, h)
        for r in reads:
            node.add_read(r)
            self._host_edits = True
        return node

    def create_edges(self, sourceNode, targetNode, sourceGeneMerDirection, targetGeneMerDirection):
        """the adjacency as seen from either end: (A, B, dA, dB) and (B, A, -dB, -dA) (:246-262)"""
        return (Edge(sourceNode, targetNode, sourceGeneMerDirection, targetGeneMerDirection),
                Edge(targetNode, sourceNode, targetGeneMerDirection * -1, sourceGeneMerDirection * -1))

    def add_edge_to_edges(self, edge):
        edges = self._v().edges
        h = edge.__hash__()
        if h not in edges:   # the first object of a class is the one that stays (:268-277)
            self._host_edits = True
            edges[h] = edge
        return edges[h]

    def add_edges_to_graph(self, sourceToTargetEdge, reverseTargetToSourceEdge):
        return self.add_edge_to_edges(sourceToTargetEdge), self.add_edge_to_edges(reverseTargetToSourceEdge)

    def add_edge_to_node(self, node, edge):
        """forward or backward list by the STORED edge's source direction (:287-298)"""
        self._host_edits = True
        if edge.get_sourceNodeDirection() == 1:
            node.add_forward_edge_hash(edge.__hash__())
        if edge.get_sourceNodeDirection() == -1:
            node.add_backward_edge_hash(edge.__hash__())
        return node

    def add_edge(self, sourceGeneMer, targetGeneMer):
        sourceNode = self.add_node(sourceGeneMer, [])
        targetNode = self.add_node(targetGeneMer, [])
        forward, backward = self.add_edges_to_graph(*self.create_edges(
            sourceNode, targetNode, sourceGeneMer.get_geneMerDirection(), targetGeneMer.get_geneMerDirection()))
        self.add_edge_to_node(sourceNode, forward)
        self.add_edge_to_node(targetNode, backward)
        return forward, backward

    def remove_edge_from_edges(self, edgeHash):
        self._host_edits = True
        del self._v().edges[edgeHash]

    def remove_edge(self, edgeHash):
        """drop an edge from the graph and from its source node's list; unknown hashes are ignored (:409-428).
        On a graph that has not been edited by hand the edge is removed ON THE DEVICE (amg_remove_edges), so that
        device passes keep working afterwards, as filter_graph does after remove_edge in the reference."""
        edges = self._v().edges
        if edgeHash not in edges:
            return
        edge = edges[edgeHash]
        if not self._host_edits and getattr(edge, "_amg_id", None) is not None:
            last = self._pass_log[-1] if self._pass_log else None
            self._run_pass("remove_edges", [int(edge._amg_id)])
            # a loop that removes many edges one at a time replays as ONE device call (pickling: rebuild + replay)
            if last is not None and last[0] == "remove_edges":
                last[1][0].extend(self._pass_log.pop()[1][0])
            # (source id, target id, source direction, target direction): tip clipping wants to know whether the twin
            # of every edge removed one at a time is gone as well
            self._lone_edges.add((edge.get_sourceNode()._amg_id, edge.get_targetNode()._amg_id,
                                  edge.get_sourceNodeDirection(), edge.get_targetNodeDirection()))
            # the view follows in place instead of being thrown away (re-fetching every array of the graph per removed
            # edge made such a loop quadratic): the edge's alive flag, which the lazily made edge lists look at, the
            # source node's list if it exists already, and the edge's entry
            v = self._v()
            source = edge.get_sourceNode()   # (a list not made yet is made here, WITH the edge, and loses it below)
            if edge.get_sourceNodeDirection() == 1:
                source.remove_forward_edge_hash(edgeHash)
            if edge.get_sourceNodeDirection() == -1:
                source.remove_backward_edge_hash(edgeHash)
            v.arrays["edges"]["alive"][edge._amg_id] = 0
            del v.edges[edgeHash]
            return
        source = edge.get_sourceNode()
        if edge.get_sourceNodeDirection() == 1:
            source.remove_forward_edge_hash(edgeHash)
        if edge.get_sourceNodeDirection() == -1:
            source.remove_backward_edge_hash(edgeHash)
        self.remove_edge_from_edges(edgeHash)

    def remove_node_from_reads(self, node_to_remove):
        """every occurrence of the node becomes None on its reads, which join the reads to correct (:442-461)"""
        v = self._v()
        self._host_edits = True
        h = node_to_remove.__hash__()
        for read_id in node_to_remove.get_reads():
            keep = [x != h for x in v.readNodes[read_id]]
            for lists in (v.readNodes, v.readNodeDirections, v.readNodePositions):
                lists[read_id] = [x if k else None for x, k in zip(lists[read_id], keep)]
            self._extra_to_correct.add(read_id)

    def dfs_component(self, start, component_id, visited=None):
        visited = set() if visited is None else visited
        visited.add(start.__hash__())
        start.set_component(component_id)
        for neighbor in self.get_all_neighbors(start):
            if neighbor.__hash__() not in visited:
                self.dfs_component(neighbor, component_id, visited)

    def assign_component_ids(self):
        """component ids 1, 2, ... in order of each component's first node (:920-927); the device
        build has already done this — the method re-labels the host view (after host edits)"""
        visited, component_id = set(), 1
        for h, node in self.get_nodes().items():
            if h not in visited:
                self.dfs_component(node, component_id, visited)
                component_id += 1

    def calculate_mean_node_coverage(self):
        return statistics.mean(self.get_all_node_coverages())

    # ------------------------------------------------------------------ topology (:326-400)
    def get_degree(self, node):
        return len(node.get_forward_edge_hashes()) + len(node.get_backward_edge_hashes())

    def get_forward_edges(self, node):
        return [self.get_edge_by_hash(h) for h in node.get_forward_edge_hashes()]

    def get_backward_edges(self, node):
        return [self.get_edge_by_hash(h) for h in node.get_backward_edge_hashes()]

    def get_forward_neighbors(self, node):
        return [e.get_targetNode() for e in self.get_forward_edges(node)]

    def get_backward_neighbors(self, node):
        return [e.get_targetNode() for e in self.get_backward_edges(node)]

    def get_all_neighbors(self, node):
        return self.get_forward_neighbors(node) + self.get_backward_neighbors(node)

    def get_all_neighbor_hashes(self, node):
        return set(n.__hash__() for n in self.get_all_neighbors(node))

    def check_if_nodes_are_adjacent(self, sourceNode, targetNode):
        return (targetNode.__hash__() in self.get_all_neighbor_hashes(sourceNode)
                and sourceNode.__hash__() in self.get_all_neighbor_hashes(targetNode))

    def get_edge_hashes_between_nodes(self, sourceNode, targetNode):
        """(source->target hash, target->source hash); a pair of LISTS when either side has
        several (the reference's multi-edge quirk, :364-386)."""
        assert self.check_if_nodes_are_adjacent(sourceNode, targetNode)
        s2t = [e.__hash__() for e in self.get_forward_edges(sourceNode) + self.get_backward_edges(sourceNode)
               if e.get_targetNode() == targetNode]
        t2s = [e.__hash__() for e in self.get_forward_edges(targetNode) + self.get_backward_edges(targetNode)
               if e.get_targetNode() == sourceNode]
        if not (len(s2t) > 1 or len(t2s) > 1):
            return (s2t[0], t2s[0])
        return (s2t, t2s)

    def get_edges_between_nodes(self, sourceNode, targetNode):
        a, b = self.get_edge_hashes_between_nodes(sourceNode, targetNode)
        if not (isinstance(a, list) or isinstance(b, list)):
            return self.get_edge_by_hash(a), self.get_edge_by_hash(b)
        return [self.get_edge_by_hash(h) for h in a], [self.get_edge_by_hash(h) for h in b]

    # ------------------------------------------------------------------ removals + filter
    def remove_node(self, node):
        """remove a node, its edges (both directions) and mask it on its reads (:463-484)."""
        h = node.__hash__()
        assert h in self.get_nodes(), "This node is not in the graph"
        assert node == self.get_node_by_hash(h)
        if self._host_edits:   # host-edited graph: the reference's own steps on the view
            self.remove_node_from_reads(node)
            for edge_hash in set(node.get_forward_edge_hashes() + node.get_backward_edge_hashes()):
                target = self.get_edge_by_hash(edge_hash).get_targetNode()
                for e in self.get_edge_hashes_between_nodes(node, target):
                    self.remove_edge(e)
            del self.get_nodes()[h]
            return
        self._run_pass("remove_nodes", [int(self._node_id(h))])
        self._invalidate()

    def _remove_node_ids(self, ids):
        if len(ids):
            self._run_pass("remove_nodes", np.asarray(ids, dtype=np.int32))
            self._invalidate()

    def list_nodes_to_remove(self, minNodeCoverage):
        return {n for n in self.all_nodes() if not n.get_node_coverage() > minNodeCoverage - 1}

    def list_edges_to_remove(self, minEdgeCoverage, nodesToRemove):
        doomed = set()
        for h, e in self.get_edges().items():
            if not e.get_edge_coverage() > minEdgeCoverage - 1:
                doomed.add(h)
            if e.get_sourceNode() in nodesToRemove or e.get_targetNode() in nodesToRemove:
                doomed.add(h)
        return doomed

    def filter_graph(self, minNodeCoverage, minEdgeCoverage):
        """device coverage filter: nodes with coverage < minNodeCoverage, edges with coverage
        < minEdgeCoverage or a removed endpoint; reads through removed nodes are masked and
        queued for correction (:523-540)."""
        self._device_pass("filter_graph")
        self.set_minNodeCoverage(minNodeCoverage)
        self.set_minEdgeCoverage(minEdgeCoverage)
        self._run_pass("filter", max(int(minNodeCoverage), 0), max(int(minEdgeCoverage), 0))
        self._invalidate()
        return self

    def remove_low_coverage_components(self, min_component_coverage):
        self._device_pass("remove_low_coverage_components")
        self._run_pass("remove_low_coverage_components", max(int(min_component_coverage), 0))
        self._invalidate()

    def remove_short_linear_paths(self, min_length, sample_genesOfInterest={}, _lazy_hashes=False):
        """tip clipping on the device (:679-720); returns the hashes of the removed nodes (a list, as the reference
        does; _lazy_hashes: the drivers of graph_utils, which ignore the result, ask for a Sequence whose hashes are
        only made when somebody looks at them)."""
        self._device_pass("remove_short_linear_paths")
        if any((t, s_, -td, -sd) not in self._lone_edges for (s_, t, sd, td) in self._lone_edges):
            # the walk of the device kernel takes an adjacency from either end; the reference's, on a graph where
            # remove_edge took ONE direction of an adjacency away, depends on which end it comes from
            raise RuntimeError("remove_short_linear_paths: remove_edge has removed one direction of an adjacency and "
                               "left its twin; remove the twin (the edge target -> source with both directions "
                               "negated) as well, as filter_graph and remove_node do")
        protect = None
        if sample_genesOfInterest:
            ids = self._node_ids_containing(list(sample_genesOfInterest))
            if ids:
                protect = np.zeros(self._engine.counts()["n_nodes"], np.uint8)
                protect[ids] = 1
        v = self._view   # the object view is NOT made for this: the hashes of the removed nodes come from their tokens
        tokens = None if v is not None else self._engine.nodes()["tokens"]
        removed = self._run_pass("remove_short_linear_paths", int(min_length), protect)
        if v is not None:
            v.ensure_hashes(removed.tolist(), removed_since=True)   # (a batch: one device call over the view's rows)
            hashes = [v.hash_at(i) for i in removed.tolist()]
        elif _lazy_hashes:
            # (the drivers, which ignore the result): the hashes — a sha256 per removed node, tens of thousands of
            # them in a first sweep — are made when somebody looks at them, a batch of them in one device call
            hashes = _LazyHashes(tokens[removed], self._vocab, self._row_namer())
        else:
            hashes = hashes_of_token_rows(self._vocab, tokens[removed], self._row_namer())
        if len(hashes):
            self._invalidate()
        return hashes

    def _gene_flags(self, genes):
        """a byte per gene rank, 1 for the genes named (what the engine's read walks take); unknown names flag nothing"""
        flags = np.zeros(self._vocab.two_v // 2, np.uint8)
        for g in genes:
            r = self._vocab.rank.get(g)
            if r is not None:
                flags[r] = 1
        return flags

    def remove_non_AMR_associated_nodes(self, genesOfInterest):
        """drop every node none of whose reads touches a node holding a gene of interest (:2941-2959)."""
        if not self._host_edits:
            # one walk over the reads on the device (amg_remove_non_amr_nodes): no view, no id list
            if self._run_pass("remove_non_amr_nodes", self._gene_flags(list(genesOfInterest))):
                self._invalidate()
            return
        v = self._v()
        amr_ids = self._node_ids_containing(list(genesOfInterest))
        tok_node = v.arrays["tok_node"]
        D = len(v.alive)
        is_amr = np.zeros(D + 1, bool)
        is_amr[amr_ids] = True
        live = tok_node >= 0
        read_of_tok = np.repeat(np.arange(len(self._read_ids)), np.diff(self._read_off))
        reads_hit = np.zeros(len(self._read_ids), bool)
        reads_hit[read_of_tok[live & is_amr[np.where(live, tok_node, D)]]] = True
        node_hit = np.zeros(D, bool)
        node_hit[tok_node[live & reads_hit[read_of_tok]]] = True
        self._remove_node_ids(np.nonzero((v.alive != 0) & ~node_hit)[0])

    def remove_junk_reads(self, error_rate):
        """split reads by their fraction of masked nodes; Python round() (:1398-1420)."""
        if not self._host_edits:
            return self._remove_junk_reads_arrays(error_rate)
        new_reads, new_positions, rejected_reads, rejected_read_positions = {}, {}, {}, {}
        for read_id, nodes in self.get_readNodes().items():
            allowed = round(len(nodes) * (1 - error_rate))
            masked = sum(1 for n in nodes if n is None)
            if masked <= allowed:
                new_reads[read_id] = self._reads[read_id]
                new_positions[read_id] = self._genePositions[read_id]
            else:
                rejected_reads[read_id] = self._reads[read_id]
                rejected_read_positions[read_id] = self._genePositions[read_id]
        return new_reads, new_positions, rejected_reads, rejected_read_positions

    def _remove_junk_reads_arrays(self, error_rate):
        """remove_junk_reads on the device (amg_select_reads, AMG_SELECT_JUNK): the masked windows of every read are
        counted where the per-window node ids live, and the table they are held against is the reference's own
        expression, allowed[w] = round(w * (1 - error_rate)) by the interpreter's round for every window count a read
        can have.  Array-backed inputs: the rejected reads (the inverted selection) are fetched at once, the kept ones
        stay on the device as a corrected set in which nothing changed (amira_amd.io.DeviceCorrected) for the next
        GeneMerGraph to take over.  Dict inputs: dicts, the rows taken from the verdicts."""
        offs, k = self._read_off, self._kmer_for_device()
        longest = max(int(np.diff(offs).max()) - k + 1, 0) if len(offs) > 1 else 0
        allowed = [round(w * (1 - error_rate)) for w in range(longest + 1)]
        eng = self._engine
        self._settle_leases()   # the selection overwrites the engine's corrected set
        arrays = self._tokenized_io(self._genePositions is not None) and self._genePositions is not None
        if arrays and not self._reads.edited() and self._genePositions.as_made():
            if self._positions_pending:   # a graph of build_many: its engine has not seen the positions yet
                self._upload_positions()
            _, n_reads, n_tokens = eng.select_reads(_ffi.SELECT_JUNK, True, allowed, want_verdict=False)
            rejected = self._selection_on_host(n_reads, n_tokens)
            _, n_reads, n_tokens = eng.select_reads(_ffi.SELECT_JUNK, False, allowed, want_verdict=False)
            kept = self._corrected_as_arrays(eng.corrected_index(n_reads), n_reads, n_tokens, True)
            return kept + rejected
        verdict, _, _ = eng.select_reads(_ffi.SELECT_JUNK, False, allowed)
        keep_rows, drop_rows = np.flatnonzero(verdict == _ffi.SEL_KEPT), np.flatnonzero(verdict == _ffi.SEL_REJECTED)
        if arrays:   # (mappings edited since the build: what they hold now, gathered on the host)
            return (self._reads.subset(keep_rows), self._genePositions.subset(keep_rows),
                    self._reads.subset(drop_rows), self._genePositions.subset(drop_rows))
        ids, reads, pos = self._read_ids, self._reads, self._genePositions
        keep = [ids[i] for i in keep_rows.tolist()]
        drop = [ids[i] for i in drop_rows.tolist()]
        return ({r: reads[r] for r in keep}, {r: pos[r] for r in keep},
                {r: reads[r] for r in drop}, {r: pos[r] for r in drop})

    def _selection_on_host(self, n_reads, n_tokens):
        """the engine's selected set as (reads, positions) over host arrays, fetched now, positions as int32 when they fit"""
        src = getattr(self._reads, "source_rows", None)
        source_ids = self._reads.read_ids if src is None else self._reads.source_ids
        if n_reads == 0:
            offs = np.zeros(1, np.int64)
            none = np.zeros(0, np.int32)
            return (TokenizedReads(self._vocab, none, offs, [], source_rows=np.zeros(0, np.int64), source_ids=source_ids),
                    TokenizedPositions([], offs, none, none))
        out = self._engine.corrected(n_reads, n_tokens, True, pos32=True)
        orig, offs = out["orig_read"], out["read_offsets"]
        ids = self._read_ids if len(orig) == len(self._read_ids) else self._names_of_rows(orig)
        reads = TokenizedReads(self._vocab, out["tokens"], offs, ids,
                               source_rows=orig.astype(np.int64) if src is None else src[orig], source_ids=source_ids)
        return reads, TokenizedPositions(ids, offs, out["gene_start"], out["gene_end"])

    def get_valid_reads_only(self):
        """the reads that are not marked for correction (:1422-1427).  Array-backed reads: selected on the device
        (amg_select_reads, AMG_SELECT_VALID) and handed back as a TokenizedReads over a DeviceCorrected"""
        if not self._host_edits and isinstance(self._reads, TokenizedReads) and not self._reads.edited():
            self._settle_leases()   # the selection overwrites the engine's corrected set
            _, n_reads, n_tokens = self._engine.select_reads(_ffi.SELECT_VALID, want_verdict=False)
            reads, _ = self._corrected_as_arrays(self._engine.corrected_index(n_reads), n_reads, n_tokens, False)
            return reads
        fix = self.get_reads_to_correct()
        return {r: g for r, g in self._reads.items() if r not in fix}
