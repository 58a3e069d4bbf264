"""amg_select_reads (include/amg.h) stated in plain numpy / Python: what the call must answer for a read set, the
per-window node ids of its graph and the reads marked for correction.  The tests compute their expectations here, from
what amg_get_read_nodes / amg_get_reads_to_correct return or from an oracle graph — never from the call under test;
tests/test_select_oracle_cpu.py holds this statement to the pure-Python amira_oracle."""
import numpy as np

VALID, JUNK = 0, 1                   # AMG_SELECT_*
REJECTED, KEPT, UNLISTED = 0, 1, 2   # AMG_SEL_*


def allowed_table(error_rate, longest_windows):
    """allowed[w] = round(w * (1 - error_rate)), the reference's expression (construct_graph.py:1409) with the
    interpreter's own round (half to even), for w = 0 .. longest_windows"""
    return [round(w * (1 - error_rate)) for w in range(longest_windows + 1)]


def windows(read_offsets, k):
    return np.maximum(np.diff(np.asarray(read_offsets, np.int64)) - k + 1, 0)


def masked_windows(read_offsets, k, tok_node):
    """per read, the windows whose node id is negative (inside a read's windows: -2, the node was removed)"""
    off = np.asarray(read_offsets, np.int64)
    w = windows(off, k)
    return np.asarray([int((tok_node[a:a + n] < 0).sum()) for a, n in zip(off[:-1].tolist(), w.tolist())], np.int64)


def verdicts(read_offsets, k, tok_node, to_correct, mode, allowed=None):
    """a byte per read; None where the call must refuse the table (a read with w >= len(allowed))"""
    off = np.asarray(read_offsets, np.int64)
    n_reads = len(off) - 1
    if mode == VALID:
        return np.where(np.asarray(to_correct)[:n_reads] != 0, REJECTED, KEPT).astype(np.uint8)
    w, m = windows(off, k), masked_windows(off, k, tok_node)
    out = np.full(n_reads, UNLISTED, np.uint8)
    for r in range(n_reads):
        if w[r] == 0:
            continue
        if w[r] >= len(allowed):
            return None
        out[r] = KEPT if m[r] <= allowed[w[r]] else REJECTED
    return out


def select(tokens, read_offsets, k, tok_node, to_correct, mode, invert, allowed=None, gene_start=None, gene_end=None,
           pos_off=None):
    """the whole call: verdicts, the rows of the selected set (ascending), its CSR (tokens, read_offsets) and, with
    position arrays, its positions laid end to end and where each read's begin in the caller's arrays (pos_off[r], or
    the read's token offset without one).  None when the table must be refused."""
    off = np.asarray(read_offsets, np.int64)
    v = verdicts(off, k, tok_node, to_correct, mode, allowed)
    if v is None:
        return None
    rows = np.flatnonzero(v == (REJECTED if invert else KEPT))
    lens = np.diff(off)[rows]
    new_off = np.zeros(len(rows) + 1, np.int64)
    np.cumsum(lens, out=new_off[1:])
    flat = np.concatenate([np.arange(off[r], off[r + 1]) for r in rows.tolist()] + [np.zeros(0, np.int64)]).astype(np.int64)
    out = {"verdict": v, "rows": rows, "read_offsets": new_off, "tokens": np.asarray(tokens, np.int32)[flat],
           "n_reads": len(rows), "n_tokens": int(new_off[-1])}
    if gene_start is not None:
        begin = off[:-1] if pos_off is None else np.asarray(pos_off, np.int64)
        pflat = np.concatenate([np.arange(begin[r], begin[r] + off[r + 1] - off[r]) for r in rows.tolist()]
                               + [np.zeros(0, np.int64)]).astype(np.int64)
        out["pos_src"] = begin[rows]
        out["gene_start"], out["gene_end"] = np.asarray(gene_start)[pflat], np.asarray(gene_end)[pflat]
    return out


def node_bound_floor(read_offsets, k, tok_node, alive, rows):
    """what the next build's node bound must at least be: the distinct live nodes on the set's reads plus, at worst one
    new node each, their masked windows — and what the call reports: ALL alive nodes plus those masked windows"""
    off = np.asarray(read_offsets, np.int64)
    m = masked_windows(off, k, tok_node)
    return int(np.count_nonzero(alive)) + int(m[rows].sum())


# ------------------------------------------------------------------ the named case of the selection tests
CASE_LENS = [0, 2, 3, 4, 5, 8, 13, 21, 34, 55, 66, 67, 68, 90]
CASE_K = 3
CASE_RATES = (0.8, 0.75, 0.5, 1.0, 0.0)
# what the pure-Python oracle answers on the case after filter_graph(3, 1): (kept, rejected) per rate
CASE_WANT = {0.8: (245, 97), 0.75: (281, 61), 0.5: (325, 17), 1.0: (107, 235), 0.0: (342, 0)}


def named_case(n=None):
    """(reads, positions, fastq): P.synth_inputs(23, 400, 90, 120, 0.06), read i in dict order cut to its first
    CASE_LENS[i % 14] genes with its positions cut alike — window counts 0, 1, 64, 65, 66 and 88 among others at k = 3;
    n: only the first n reads"""
    import procedures as P
    reads, pos, fq = P.synth_inputs(23, 400, 90, 120, 0.06)
    ids = list(reads)[:n]
    cut = {r: list(reads[r])[:CASE_LENS[i % 14]] for i, r in enumerate(ids)}
    cut_pos = {r: [tuple(p) for p in pos[r]][:CASE_LENS[i % 14]] for i, r in enumerate(ids)}
    return cut, cut_pos, fq


def arrays_of_oracle_graph(g, reads):
    """(vocab, tokens, read_offsets, read ids, tok_node, to_correct flags) of an oracle graph built from `reads`: the
    engine's conventions (-1 no window, -2 a masked window, else any id >= 0)"""
    from amira_amd.tokens import tokenize
    vocab, toks, offs, ids = tokenize(reads)
    tok_node = np.full(int(offs[-1]), -1, np.int32)
    for r, rid in enumerate(ids):
        for i, h in enumerate(g.get_readNodes().get(rid, [])):
            tok_node[int(offs[r]) + i] = -2 if h is None else 0
    fix = g.get_reads_to_correct()
    return vocab, toks, offs, ids, tok_node, np.asarray([1 if r in fix else 0 for r in ids], np.uint8)
