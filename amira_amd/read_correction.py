"""Read correction of GeneMerGraph (a mixin, like bubble_popping.BubblePopping): correct_reads on the device
(amg_correct_reads + amg_get_corrected), its array-in / array-out form, and the reference's single-read host twin
with needleman_wunsch and replace_invalid_gene_positions."""
import ctypes as C
import os
import statistics
from itertools import product

import numpy as np

from . import _ffi
from .io import TokenizedPositions, TokenizedReads


class ReadCorrection:
    # ------------------------------------------------------------------ correction (:1123-1396)
    def correct_reads(self, fastq_data):
        """Re-thread every queued read through the filtered graph on the device and return
        (corrected gene calls, corrected gene positions) like the reference: untouched reads
        keep their original list objects, reads whose nodes were all removed disappear,
        self._genePositions is updated in place for changed reads."""
        self._device_pass("correct_reads")
        eng, vocab = self._engine, self._vocab
        have_pos = bool(self._genePositions)
        if self._positions_pending:   # a graph of build_many: its engine has not seen the positions yet
            self._upload_positions()
        if have_pos and hasattr(fastq_data, "lengths_array"):   # amira_amd.io.ReadLengths: no per-read loop
            eng.set_read_lengths(fastq_data.lengths_array(self._read_ids, getattr(self._reads, "source_rows", None),
                                                          getattr(self._reads, "source_ids", None)))
        elif have_pos:
            flags = eng.reads_to_correct()
            lengths = np.zeros(len(self._read_ids), np.int64)
            for r in np.nonzero(flags)[0].tolist():
                try:  # only consulted when a trailing gene needs an inferred end (:1685)
                    lengths[r] = len(fastq_data[self._read_ids[r]]["sequence"])
                except (KeyError, TypeError, IndexError):
                    lengths[r] = 0
            eng.set_read_lengths(lengths)
        n_reads, n_tokens = eng.correct_reads()   # (an earlier correction's output was fetched by _device_pass)
        if self._tokenized_io(have_pos):
            return self._corrected_as_arrays(eng.corrected_index(n_reads), n_reads, n_tokens, have_pos)
        out = eng.corrected(n_reads, n_tokens, have_pos)
        offs, toks = out["read_offsets"].tolist(), out["tokens"]
        corrected_genes, corrected_gene_positions = {}, {}
        for i, (orig, changed) in enumerate(zip(out["orig_read"].tolist(), out["changed"].tolist())):
            read_id = self._read_ids[orig]
            a, b = offs[i], offs[i + 1]
            if changed:
                corrected_genes[read_id] = vocab.decode(toks[a:b])
                if have_pos:
                    self._genePositions[read_id] = list(zip(out["gene_start"][a:b].tolist(),
                                                            out["gene_end"][a:b].tolist()))
            else:
                corrected_genes[read_id] = self._reads[read_id]
            if have_pos:
                corrected_gene_positions[read_id] = self._genePositions[read_id]
        return corrected_genes, corrected_gene_positions

    def _tokenized_io(self, have_pos):
        """the caller handed the reads (and positions) over as arrays (amira_amd.io.TokenizedReads /
        TokenizedPositions): corrections go back the same way, with no per-read Python work"""
        return isinstance(self._reads, TokenizedReads) and (not have_pos or isinstance(self._genePositions,
                                                                                         TokenizedPositions))

    def _corrected_as_arrays(self, out, n_reads, n_tokens, have_pos):
        """correct_reads' result for array inputs: the corrected calls as a TokenizedReads, their positions as a
        TokenizedPositions — both over a DeviceCorrected: the genes and positions stay on the device until somebody
        reads them on the host, and a GeneMerGraph built from the two takes them over device to device.  Reads the
        correction changed are redirected to their new positions in the caller's mapping (the reference updates
        gene_positions in place, :1282-1284, :1328)"""
        from .io import DeviceCorrected
        orig = out["orig_read"]
        if len(orig) == len(self._read_ids):   # nothing dropped (the order is kept): the very same reads
            ids = self._read_ids
        else:
            ids = self._read_ids_array()[orig].tolist()
        offs = out["read_offsets"]
        src = getattr(self._reads, "source_rows", None)
        on_device = DeviceCorrected(self._engine, n_reads, n_tokens, have_pos)
        reads = TokenizedReads(self._vocab, on_device, offs, ids,
                               source_rows=orig.astype(np.int64) if src is None else src[orig],
                               source_ids=self._reads.read_ids if src is None else self._reads.source_ids)
        if not have_pos:
            return reads, {}
        positions = TokenizedPositions(ids, offs, on_device, on_device)
        changed = np.flatnonzero(out["changed"])
        if len(changed):
            self._genePositions.replace_rows(orig[changed], positions, changed)
        return reads, positions

    def _read_ids_array(self):
        if getattr(self, "_read_ids_arr", None) is None:
            self._read_ids_arr = np.asarray(self._read_ids, dtype=object)
        return self._read_ids_arr

    def _names_of_rows(self, rows):
        """read names of a few rows (an int array), in that order: straight out of the list while the rows are few —
        an object array of a million names costs more to make than a few thousand lookups"""
        if getattr(self, "_read_ids_arr", None) is None and 8 * len(rows) < len(self._read_ids):
            ids = self._read_ids
            return [ids[i] for i in rows.tolist()]
        return self._read_ids_array()[rows].tolist()

    def correct_single_read(self, read_id, readNodes, fastq_data):
        """host twin of one read of the device correction (:1136-1151), for callers that correct a
        single read by hand; correct_reads runs all of them on the device"""
        if read_id not in self.get_reads_to_correct():
            return self.get_reads()[read_id]
        if all(n is None for n in readNodes[read_id]):
            return []
        start, end = self.find_read_boundaries(readNodes[read_id])
        new_genes_on_read = self.process_read_correction(read_id, readNodes, start, end, fastq_data)
        if self.get_gene_positions():
            assert len(new_genes_on_read) == len(self.get_gene_positions()[read_id])
        return new_genes_on_read

    def generate_replacement_dict(self, corrected, pair):
        first, last = pair
        return {pair: self.new_find_paths_between_nodes(corrected[first][0], corrected[last][0],
                                                        self.get_kmerSize() * 2, corrected[first][1])}

    def get_possible_paths(self, nodes_on_read, replacementDict, start, end):
        """every way of filling the read's None runs, as (node hashes, directions); windows without a
        node are skipped (the reference's upstream / downstream extension is disabled, :1205-1263)"""
        return [([n for n, _ in filled if n], [d for n, d in filled if n])
                for filled in self.insert_elements(nodes_on_read, replacementDict)]

    def process_read_correction(self, read_id, readNodes, start, end, fastq_data):
        k = self.get_kmerSize()
        directions = self.get_readNodeDirections()[read_id]
        nodes_on_read = [(readNodes[read_id][i], directions[i]) for i in range(len(readNodes[read_id]))]
        path_terminals = self.identify_path_terminals(readNodes[read_id], start, end)
        if len(path_terminals) == 0:   # only the ends were lost: slice genes and positions
            if self.get_gene_positions():
                self.get_gene_positions()[read_id] = self.get_gene_positions()[read_id][start:end + k]
            kept = nodes_on_read[start:end + 1]
            return self.get_annotation_for_read([n for n, _ in kept], [d for _, d in kept], read_id)
        replacementDict = {}
        for pair in path_terminals:
            replacementDict.update(self.generate_replacement_dict(nodes_on_read, pair))
        possible_paths = self.get_possible_paths(nodes_on_read, replacementDict, start, end)
        if possible_paths == []:
            return self.get_reads()[read_id]
        original = self.get_reads()[read_id]
        best_shared, best_coverage = 0, 0
        for nodes, dirs in possible_paths:   # most shared genes, then strictly higher mean coverage
            coverage = self.get_coverage_of_path(nodes)
            genes = self.get_annotation_for_read(nodes, dirs, read_id)
            shared = len(set(genes).intersection(original))
            if shared > best_shared or (shared == best_shared and coverage > best_coverage):
                closest, best_shared, best_coverage = genes, shared, coverage
        old_positions, taken, new_positions = self.get_gene_positions()[read_id], 0, []
        for new_gene, old_gene in self.needleman_wunsch(closest, original):
            if new_gene == "*":
                taken += 1
            elif old_gene != new_gene:
                new_positions.append((None, None))
            else:
                new_positions.append(old_positions[taken])
                taken += 1
        self.get_gene_positions()[read_id] = self.replace_invalid_gene_positions(new_positions, fastq_data, read_id)
        return closest

    def score(self, x, y):
        return int(x == y)

    def find_read_boundaries(self, readNode):
        start, end = 0, len(readNode) - 1
        for i, node in enumerate(readNode):
            if node:
                start = i
                break
        for i, node in enumerate(reversed(readNode)):
            if node:
                end = len(readNode) - 1 - i
                break
        return start, end

    def identify_path_terminals(self, corrected, start, end):
        terminals = []
        for i in range(len(corrected)):
            if start <= i <= end and not corrected[i]:
                if corrected[i - 1]:
                    path_start = i - 1
                if corrected[i + 1]:
                    terminals.append((path_start, i + 1))
        return terminals

    def insert_elements(self, base_list, insert_dict):
        if len(insert_dict) == 0:
            return [base_list]
        choices = [[(key, p) for p in paths] for key, paths in insert_dict.items()]
        results = []
        for combination in product(*choices):
            cur, shift = base_list[:], 0
            for (start, end), path in combination:
                cur[start + shift:end + shift + 1] = path
                shift += len(path) - (end - start + 1)
            results.append(cur)
        return results

    def new_find_paths_between_nodes(self, start_hash, end_hash, distance, current_direction,
                                     path=None, seen_nodes=None):
        """host twin of the device DFS in k_corr_gapped (:2292-2342)."""
        path = [] if path is None else path
        seen_nodes = set() if seen_nodes is None else seen_nodes
        path.append((start_hash, current_direction))
        seen_nodes.add(start_hash)
        if (end_hash and start_hash == end_hash and len(path) <= distance) or (
                end_hash is None and len(path) - 1 == distance):
            return [list(path)]
        if len(path) - 1 > distance:
            return []
        node = self.get_node_by_hash(start_hash)
        hops = (node.get_forward_edge_hashes() if current_direction == 1
                else node.get_backward_edge_hashes() if current_direction == -1 else [])
        found = []
        for edge_hash in hops:
            edge = self.get_edge_by_hash(edge_hash)
            nxt = edge.get_targetNode().__hash__()
            if nxt not in seen_nodes:
                found.extend(self.new_find_paths_between_nodes(
                    nxt, end_hash, distance, edge.get_targetNodeDirection(), list(path), seen_nodes | {nxt}))
        return found

    def get_coverage_of_path(self, path):
        return statistics.mean([self.get_node_by_hash(n).get_node_coverage() for n in path])

    def get_annotation_for_read(self, listOfNodes, listOfNodeDirections, read_id):
        assert len(listOfNodes) == len(listOfNodeDirections), (
            f"The number of nodes and node directions for read {read_id} are not the same")
        if not listOfNodeDirections:
            listOfNodeDirections = self.get_readNodeDirections()[read_id]
        oriented = lambda n, d: (self.get_gene_mer_genes(n) if d == 1 else self.get_reverse_gene_mer_genes(n))
        if len(listOfNodes) == 1:
            d = listOfNodeDirections[0]
            if d != 1 and d != -1:
                raise ValueError(f"Gene-mer direction for a node with 1 read cannot be {d}")
            return oriented(self.get_node_by_hash(listOfNodes[0]), d)
        genes = []
        for i, h in enumerate(listOfNodes):
            node, d = self.get_node_by_hash(h), listOfNodeDirections[i]
            if i == 0:
                genes += oriented(node, d)[:-1]
            if d:
                genes.append(oriented(node, d)[-1])
        assert None not in genes
        return genes

    def needleman_wunsch(self, x, y):
        """host twin of k_corr_nw: match 1 / mismatch 0 / gap -1, borders -index, ties broken
        by max over (score, pointer) tuples => UP > LEFT > DIAG (:1433-1480)."""
        N, M = len(x), len(y)
        if N * M > 16 and not os.environ.get("AMG_NW_PYTHON"):
            # beyond a handful of cells: the same recurrence and tie order on interned genes in libamg (amg_nw_align)
            code = {}
            try:
                xs = np.fromiter((code.setdefault(g, len(code)) for g in x), np.int32, N)
                ys = np.fromiter((code.setdefault(g, len(code)) for g in y), np.int32, M)
            except TypeError:
                xs = None   # (unhashable items: the table below compares them as they are)
            if xs is not None:
                ops, n_ops = np.empty(N + M, np.int8), C.c_int32(0)
                _ffi.check(_ffi.lib.amg_nw_align(_ffi.ptr(xs), N, _ffi.ptr(ys), M, _ffi.ptr(ops), C.byref(n_ops)))
                alignment, i, j = [], 0, 0
                for op in ops[:n_ops.value].tolist():
                    if op == 0:
                        alignment.append((x[i], y[j]))
                        i, j = i + 1, j + 1
                    elif op == 1:
                        alignment.append((x[i], "*"))
                        i += 1
                    else:
                        alignment.append(("*", y[j]))
                        j += 1
                return alignment
        DIAG, LEFT, UP = (-1, -1), (-1, 0), (0, -1)
        F, Ptr = {(-1, -1): 0}, {}
        for i in range(N):
            F[i, -1] = -i
        for j in range(M):
            F[-1, j] = -j
        for i in range(N):
            for j in range(M):
                F[i, j], Ptr[i, j] = max((F[i - 1, j - 1] + int(x[i] == y[j]), DIAG),
                                         (F[i - 1, j] - 1, LEFT), (F[i, j - 1] - 1, UP))
        alignment = []
        i, j = N - 1, M - 1
        while i >= 0 and j >= 0:
            step = Ptr[i, j]
            alignment.append((x[i], y[j]) if step == DIAG else (x[i], "*") if step == LEFT else ("*", y[j]))
            i, j = i + step[0], j + step[1]
        while i >= 0:
            alignment.append((x[i], "*"))
            i -= 1
        while j >= 0:
            alignment.append(("*", y[j]))
            j -= 1
        return alignment[::-1]

    def replace_invalid_gene_positions(self, new_positions, fastq_data, read_id):
        prev_end = 0
        for i, (start, end) in enumerate(new_positions):
            if end is not None:
                prev_end = end
            if start is None and end is None:
                next_start = next((p[0] for p in new_positions[i + 1:] if p[0] is not None), None)
                if next_start is not None:
                    new_positions[i] = (prev_end, next_start)
                else:
                    new_positions[i] = (prev_end, len(fastq_data[read_id]["sequence"]) - 1)
        return new_positions

