"""Paths and output of GeneMerGraph (a mixin, like bubble_popping.BubblePopping): gene strings of nodes and unitigs,
GML output, linear-path walks, coverage and component queries — what the reference does in Python on a built graph."""
import os
import statistics

import numpy as np

from .construct_gene import convert_int_strand_to_string


class PathsAndOutput:
    # ------------------------------------------------------------------ gene strings / unitigs
    def get_gene_mer_genes(self, sourceNode):
        return [convert_int_strand_to_string(g.get_strand()) + g.get_name()
                for g in sourceNode.get_canonical_geneMer()]

    def get_reverse_gene_mer_genes(self, sourceNode):
        return [convert_int_strand_to_string(g.get_strand()) + g.get_name()
                for g in sourceNode.get_reverse_geneMer()]

    def get_gene_mer_label(self, sourceNode):
        return "~~~".join(self.get_gene_mer_genes(sourceNode))

    def get_nodes_with_degree(self, degree):
        assert isinstance(degree, int), "The input degree must be an integer."
        return [n for n in self.all_nodes() if self.get_degree(n) == degree]

    def reverse_list_of_genes(self, list_of_genes):
        return [("-" if g[0] == "+" else "+") + g[1:] for g in reversed(list_of_genes)]

    def get_genes_in_unitig(self, listOfNodes):
        """gene strings spelled by a node path (:617-677): extend to the right, and if that
        fails at any step redo the whole path extending to the left."""
        if len(listOfNodes) == 1:
            return self.get_gene_mer_genes(self.get_node_by_hash(listOfNodes[0]))
        if not self._host_edits and not os.environ.get("AMG_BUBBLES_BY_OBJECTS"):
            genes = self._genes_in_unitig_from_arrays(listOfNodes)
            if genes is not None:
                return genes
        k1 = self._kmerSize - 1

        def first_orientation():
            a, b = self.get_node_by_hash(listOfNodes[0]), self.get_node_by_hash(listOfNodes[1])
            edge = self.get_edge_by_hash(self.get_edge_hashes_between_nodes(a, b)[0])
            return (self.get_gene_mer_genes(a) if edge.get_sourceNodeDirection() == 1
                    else self.get_reverse_gene_mer_genes(a))

        def walk(prepend):
            genes = []
            for n in range(len(listOfNodes) - 1):
                src = self.get_node_by_hash(listOfNodes[n])
                tgt = self.get_node_by_hash(listOfNodes[n + 1])
                self.get_edge_by_hash(self.get_edge_hashes_between_nodes(src, tgt)[0])
                if n == 0:
                    genes += first_orientation()
                fw, bw = self.get_gene_mer_genes(tgt), self.get_reverse_gene_mer_genes(tgt)
                if not prepend:
                    tail = genes[-k1:] if k1 else genes[0:]
                    if fw[:-1] == tail:
                        genes.append(fw[-1])
                    elif bw[:-1] == tail:
                        genes.append(bw[-1])
                    else:
                        return None
                else:
                    head = genes[:k1]
                    if fw[1:] == head:
                        genes.insert(0, fw[0])
                    elif bw[1:] == head:
                        genes.insert(0, bw[0])
                    else:
                        raise ValueError("Gene sequences do not match in alternative path.")
            return genes

        genes = walk(False)
        return genes if genes is not None else walk(True)

    def _genes_in_unitig_from_arrays(self, listOfNodes):
        """get_genes_in_unitig on the device's arrays (node tokens, live edge lists) instead of Node / Edge objects;
        None wherever the objects' way would not simply return (nodes that are not adjacent, several edges between
        two nodes, a path that spells nothing): it then runs and says what the reference says"""
        v = self._v()
        a = v.arrays
        n_tok, e_alive, e_tgt, e_sdir = a["nodes"]["tokens"], a["edges"]["alive"], a["edges"]["tgt"], a["edges"]["sdir"]
        adj_off, adj_edge = a["adj_off"], a["adj_edge"]
        id_of = v.node_of_hash
        ids = [id_of.get(h) for h in listOfNodes]
        if None in ids:
            return None
        flip = self._vocab.two_v - 1

        # per node, the first time a path runs over it: {target: (live edges to it, source direction of the first)} over
        # its forward list, then its backward list — what get_edge_hashes_between_nodes collects from — and its tokens
        # both ways
        node_info = a.setdefault("_unitig_nodes", {})

        def info(i):
            got = node_info.get(i)
            if got is None:
                lo, hi = int(adj_off[2 * i]), int(adj_off[2 * i + 2])
                es = adj_edge[lo:hi]
                es = es[e_alive[es] != 0]
                to = {}
                for t, sd in zip(e_tgt[es].tolist(), e_sdir[es].tolist()):
                    seen = to.get(t)
                    to[t] = (1, sd) if seen is None else (seen[0] + 1, seen[1])
                fw = n_tok[i].tolist()
                got = node_info[i] = (to, fw, [flip - t for t in reversed(fw)])
            return got

        infos = [info(i) for i in ids]
        k1 = self._kmerSize - 1
        genes = None
        for n in range(len(ids) - 1):
            there, back = infos[n][0].get(ids[n + 1]), infos[n + 1][0].get(ids[n])
            if there is None or back is None or there[0] != 1 or back[0] != 1:
                return None
            if n == 0:
                genes = list(infos[0][1] if there[1] == 1 else infos[0][2])
            _, fw, bw = infos[n + 1]
            tail = genes[-k1:] if k1 else genes[0:]
            if fw[:-1] == tail:
                genes.append(fw[-1])
            elif bw[:-1] == tail:
                genes.append(bw[-1])
            else:
                return None   # (the objects' way starts over, extending to the left)
        return self._vocab.decode(genes)

    # ------------------------------------------------------------------ GML output (:542-586, :873-909)
    def write_node_entry(self, node_id, node_string, node_coverage, reads, component_ID, nodeColor):
        rows = ["\tnode\t[", f"\t\tid\t{node_id}", f'\t\tlabel\t"{node_string}"',
                f"\t\tcoverage\t{node_coverage}"]
        if component_ID:
            rows.append(f"\t\tcomponent\t{component_ID}")
        rows.append('\t\treads\t"' + ",".join(reads) + '"')
        if nodeColor:
            rows.append(f'\t\tcolor\t"{nodeColor}"')
        rows.append("\t]")
        return "\n".join(rows)

    def write_edge_entry(self, source_node, target_node, source_edge_direction, target_edge_direction,
                         edge_coverage):
        return "\n".join(["\tedge\t[", f"\t\tsource\t{source_node}", f"\t\ttarget\t{target_node}",
                          f"\t\tsource_direction\t{source_edge_direction}",
                          f"\t\ttarget_direction\t{target_edge_direction}",
                          f"\t\tweight\t{edge_coverage}", "\t]"])

    def assign_Id_to_nodes(self):
        for i, node in enumerate(self.all_nodes()):
            assert node.assign_node_Id(i) == i, "This node was assigned an incorrect ID"

    def write_gml_to_file(self, output_file, gml_content):
        import os
        folder = os.path.dirname(output_file)
        if folder != "" and not os.path.exists(folder):
            os.mkdir(folder)
        with open(output_file + ".gml", "w") as fh:
            fh.write("\n".join(gml_content))

    def generate_gml(self, output_file, geneMerSize, min_node_coverage, min_edge_coverage):
        """nodes in dict order, each followed by its forward then backward edges (:873-909)"""
        graph_data = ["graph\t[", "multigraph 1"]
        self.assign_Id_to_nodes()
        for node in self.all_nodes():
            graph_data.append(self.write_node_entry(node.get_node_Id(), self.get_gene_mer_label(node),
                                                    node.get_node_coverage(), [r for r in node.get_reads()],
                                                    node.get_component(), node.get_color()))
            for edge in self.get_forward_edges(node) + self.get_backward_edges(node):
                if edge.get_edge_coverage() == 0:
                    continue
                graph_data.append(self.write_edge_entry(node.get_node_Id(), edge.get_targetNode().get_node_Id(),
                                                        edge.get_sourceNodeDirection(),
                                                        edge.get_targetNodeDirection(),
                                                        edge.get_edge_coverage()))
        graph_data.append("]")
        self.write_gml_to_file(".".join([output_file, str(geneMerSize), str(min_node_coverage),
                                         str(min_edge_coverage)]), graph_data)
        return graph_data

    # ------------------------------------------------------------------ linear paths (:722-861)
    def _linear_step(self, node, forward):
        hashes = node.get_forward_edge_hashes() if forward else node.get_backward_edge_hashes()
        if (forward and len(hashes) != 1) or (not forward and len(hashes) == 0):
            return False, None, None
        edge = self.get_edge_by_hash(hashes[0])
        target = edge.get_targetNode()
        extend = self.get_degree(target) in (1, 2) and target != node
        return extend, target, edge.get_targetNodeDirection()

    def get_forward_node_from_node(self, sourceNode):
        return self._linear_step(sourceNode, True)

    def get_backward_node_from_node(self, sourceNode):
        return self._linear_step(sourceNode, False)

    def get_forward_path_from_node(self, node, startDirection, wantBranchedNode=False):
        path = [node.__hash__()]
        extend, nxt, d = self._linear_step(node, startDirection == 1)
        while extend and path[0] != nxt.__hash__():
            path.append(nxt.__hash__())
            extend, nxt, d = self._linear_step(nxt, d == 1)
        if wantBranchedNode and nxt:
            path.append(nxt.__hash__())
        return path

    def get_backward_path_from_node(self, node, startDirection, wantBranchedNode=False):
        path = [node.__hash__()]
        extend, nxt, d = self._linear_step(node, startDirection != -1)
        while extend and path[-1] != nxt.__hash__():
            path.insert(0, nxt.__hash__())
            extend, nxt, d = self._linear_step(nxt, d != -1)
        if wantBranchedNode and nxt:
            path.insert(0, nxt.__hash__())
        return path

    def get_linear_path_for_node(self, node, wantBranchedNode=False):
        d0 = node.get_geneMer().get_geneMerDirection()
        backward = self.get_backward_path_from_node(node, -1 * d0, wantBranchedNode)
        assert backward[-1] == node.__hash__()
        forward = self.get_forward_path_from_node(node, d0, wantBranchedNode)
        assert forward[0] == node.__hash__()
        return backward[:-1] + [node.__hash__()] + forward[1:]

    def get_all_node_coverages(self):
        if self._host_edits:
            return [n.get_node_coverage() for n in self.all_nodes()]
        nodes = self._node_arrays()
        return nodes["coverage"][nodes["alive"] != 0].tolist()   # straight from the device arrays

    def get_mean_node_coverage(self):
        if self._host_edits:
            return statistics.mean(self.get_all_node_coverages())
        # statistics.mean of integers (:868-871) is the exact fraction, an int when it is one and the correctly rounded
        # float otherwise — which is what Python's own division of the two integers gives; the sum comes off the array
        nodes = self._node_arrays()
        cov = nodes["coverage"][nodes["alive"] != 0]
        if len(cov) == 0:
            return statistics.mean([])   # (StatisticsError, as the reference raises)
        total, n = int(cov.sum(dtype=np.int64)), int(len(cov))
        return total // n if total % n == 0 else total / n

    # ------------------------------------------------------------------ components (:911-958)
    def get_nodes_in_component(self, component):
        return [n for n in self.all_nodes() if n.get_component() == int(component)]

    def components(self):
        return sorted({n.get_component() for n in self.all_nodes()})

    def get_number_of_component(self):
        return len(self.components())

    def get_AMR_nodes(self, listOfGenes):
        out = {}
        for gene in listOfGenes:
            for node in self.get_nodes_containing(gene):
                out[node.__hash__()] = node
        return out

    def collect_reads_in_path(self, path):
        v = self._v()
        reads = set()
        for h in list(path):
            node = v.node_by_hash(h)
            if node is not None:
                reads.update(node.get_reads())   # (a list: added one by one, as the reference's loop does)
        return reads

