"""What amg_pop_rewrite must return for operations and reads chosen by the tests (tests/test_gpu_pop_rewrite.py), by
the pinned oracle's own methods on a bare instance, called in the order its correct_bubble_paths calls them
(oracle/amira_oracle/bubbles.py:329-359): compare_paths, the veto, reorient_alignment over get_gene_mer_strings,
get_path_to_alignment_mapping, longest_common_sublist, modify_alignment_subset, correct_genes_on_read and, for the
positions, the prefix / core / suffix helpers around get_new_gene_position_core — fed the INDEX of every gene of the
old read as its position, so that what comes back is the index whose position a gene keeps ((None, None): -1).

  expected     the answer for lists of gene strings
  encode       the same lists as the arrays of the C ABI
  from_arrays  the device's answer spelled back into the shape of `expected`
  planted      the operations and reads of the seeded fuzz"""
import random
from collections import Counter

import numpy as np


def _bare(k):
    from amira_oracle.graph import GeneMerGraph
    g = GeneMerGraph.__new__(GeneMerGraph)
    g._kmerSize = k
    g._reads = {}
    return g


def expected(k, operations, reads, read_op, interest=None):
    """operations: [(better genes, worse genes)]; reads: [genes]; read_op: the operation of every read; interest: gene
    NAMES (no strand) or None.  Returns {"op_veto", "status", "first_shared", "last_shared", "genes", "src", "info"}:
    lists over the operations / reads; genes and src are None unless status is 2; info[r] says which way the read was
    oriented ("fw" / "rv"), the two counts, and whether the second alignment ran."""
    g = _bare(k)
    interest = set(interest or ())
    plans, veto = [], []
    for better, worse in operations:
        fw, rv, _, _ = g.compare_paths(list(worse), list(better))
        veto.append(int(any(c[1][1:] in interest and c[0][1:] not in interest for c in fw)))
        mers = [tuple(worse[i:i + k]) for i in range(len(worse) - (k - 1))]
        plans.append((fw, rv, Counter(mers), Counter(tuple(g.reverse_list_of_genes(list(m))) for m in mers)))
    out = {"op_veto": veto, "status": [], "first_shared": [], "last_shared": [], "genes": [], "src": [], "info": []}

    def add(status, first=-1, last=-1, genes=None, src=None, info=None):
        for key, value in (("status", status), ("first_shared", first), ("last_shared", last), ("genes", genes),
                           ("src", src), ("info", info)):
            out[key].append(value)

    for r, genes_on_read in enumerate(reads):
        op = read_op[r]
        if veto[op]:
            add(0)
            continue
        fw, rv, fw_counter, bw_counter = plans[op]
        genes_on_read = list(genes_on_read)
        on_read = Counter(g.get_gene_mer_strings(genes_on_read))
        info = {"fw_count": len(on_read & fw_counter), "rv_count": len(on_read & bw_counter)}
        alignment = g.reorient_alignment(g.get_gene_mer_strings(genes_on_read), fw_counter, bw_counter, fw, rv)
        if alignment is None:
            add(1, info=info)
            continue
        info["way"] = "fw" if alignment is fw else "rv"
        _, lower_mapping = g.get_path_to_alignment_mapping(alignment)
        low_on_alignment = [a[1] for a in alignment if not a[1] == "*"]
        _, (start_path, end_path), (first, last) = g.longest_common_sublist(low_on_alignment, genes_on_read)
        subset = alignment[lower_mapping[start_path]:lower_mapping[end_path] + 1]
        modified = g.modify_alignment_subset(subset, genes_on_read[first:last + 1])
        info["second_alignment"] = modified is not subset
        assert len(modified) != 0
        new_genes = list(g.correct_genes_on_read(genes_on_read, first, last, modified, r))
        positions = list(range(len(genes_on_read)))
        core = g.get_new_gene_position_core(modified, g.get_gene_position_core(positions, first, last))
        joined = g.join_gene_position_ends_with_core(g.get_gene_position_prefix(positions, first),
                                                     g.get_gene_position_suffix(positions, last), core)
        src = [-1 if p == (None, None) else p for p in joined]
        assert len(src) == len(new_genes)
        info["core_src"] = [-1 if p == (None, None) else p for p in core]
        add(2, first, last, new_genes, src, info)
    return out


def mirrored(genes):
    return [("-" if x[0] == "+" else "+") + x[1:] for x in reversed(genes)]


def encode(vocab, operations, reads, read_op, interest=None):
    """the arguments of Engine.pop_rewrite after k and two_v"""
    def csr(lists):
        off = np.zeros(len(lists) + 1, np.int64)
        np.cumsum([len(x) for x in lists], out=off[1:])
        return np.asarray([vocab.token(x) for genes in lists for x in genes], np.int32), off

    flags = None
    if interest is not None:
        flags = np.zeros(vocab.two_v, np.uint8)
        for name in interest:
            flags[vocab.token("+" + name)] = flags[vocab.token("-" + name)] = 1
    return (*csr([b for b, _ in operations]), *csr([w for _, w in operations]), flags, *csr(reads),
            np.asarray(read_op, np.int32))


def from_arrays(vocab, got):
    """Engine.pop_rewrite's dict in the shape of expected() (without info)"""
    off = got["out_off"].tolist()
    status = got["status"].tolist()
    genes, src = [], []
    for r, s in enumerate(status):
        a, b = off[r], off[r + 1]
        genes.append(vocab.decode(got["out_tok"][a:b]) if s == 2 else None)
        src.append(got["out_src"][a:b].tolist() if s == 2 else None)
        assert s == 2 or a == b, "a read that was not rewritten has entries"
    return {"op_veto": got["op_veto"].tolist(), "status": status, "first_shared": got["first_shared"].tolist(),
            "last_shared": got["last_shared"].tolist(), "genes": genes, "src": src}


NAMES = ["g%d" % i for i in range(6)]
GENES = [s + n for n in NAMES for s in "+-"]


def with_errors(rng, genes, rate):
    """genes with substitutions, deletions and insertions, each at `rate`"""
    out = []
    for x in genes:
        u = rng.random()
        if u < rate:
            out.append(rng.choice(GENES))
        elif u < 2 * rate:
            continue
        elif u < 3 * rate:
            out += [x, rng.choice(GENES)]
        else:
            out.append(x)
    return out


def planted(seed, n_ops=40, reads_per_op=8, k=3):
    """operations cut from a planted path with errors on the worse side, lists of k .. 40 genes; reads that run along
    the worse path (either strand, whole or cut, with flanks of the planted path and errors of their own), that hold
    both strands of it, or that are strangers"""
    rng = random.Random(seed)
    path = [rng.choice(GENES) for _ in range(400)]
    operations, reads, read_op = [], [], []
    for op in range(n_ops):
        n = rng.randint(k, 40)
        at = rng.randrange(20, len(path) - n - 20)
        better = path[at:at + n]
        while True:
            worse = with_errors(rng, better, rng.choice((0.03, 0.08, 0.15)))
            if k <= len(worse) <= 40:
                break
        operations.append((better, worse))
        for _ in range(reads_per_op):
            u = rng.random()
            if u < 0.12:
                read = [rng.choice(GENES) for _ in range(rng.randint(0, 30))]
            else:
                a = rng.randint(0, max(0, len(worse) - k)) if rng.random() < 0.4 else 0
                b = rng.randint(min(len(worse), a + k), len(worse)) if rng.random() < 0.4 else len(worse)
                read = path[at - rng.randint(0, 8):at] * (a == 0) + worse[a:b] + path[at + n:at + n + rng.randint(0, 8)] * (b == len(worse))
                if rng.random() < 0.4:
                    read = with_errors(rng, read, 0.05)
                if rng.random() < 0.5:
                    read = mirrored(read)
                if u < 0.2:
                    read = read + mirrored(read[:rng.randint(k, k + 4)])
            reads.append(read)
            read_op.append(op)
    return operations, reads, read_op
