"""The three read walks of amira_amd/csrc/amg_read_walk.hip in plain numpy and Python sets, from the arrays an Engine
hands out: tokens, read_off, Engine.read_node_ids() (tok_node) and Engine.nodes() (alive, component).  One loop per
read and a set per question: nothing of the kernel's chunks, ballots or first-occurrence tests is restated here.

Window i of read r starts at token read_off[r] + i, i = 0 .. len_r - k; it is LIVE when its node id is >= 0 and the node
alive, an AMR window when one of its k tokens is a flagged gene (rank of token t: t - V for t >= V, else V - 1 - t)."""
from fractions import Fraction

import numpy as np


def _reads(read_off, k):
    """(read, first token, windows) of every read"""
    read_off = np.asarray(read_off, np.int64)
    for r in range(len(read_off) - 1):
        a, b = int(read_off[r]), int(read_off[r + 1])
        yield r, a, b - a, max(b - a - k + 1, 0)


def token_flags(tokens, flags):
    """per token: is its gene flagged"""
    tokens, flags = np.asarray(tokens, np.int64), np.asarray(flags)
    V = len(flags)
    rank = np.where(tokens >= V, tokens - V, V - 1 - tokens)
    return flags[rank] != 0 if len(tokens) else np.zeros(0, bool)


def depth_by_length(read_off, tok_node, alive, k, min_genes):
    """A: (pairs, n_alive), pairs[j] = distinct (read, node) pairs with a live window, reads of >= min_genes[j] genes"""
    pairs = [0] * len(min_genes)
    for _, a, length, n_win in _reads(read_off, k):
        nodes = {int(d) for d in tok_node[a:a + n_win] if d >= 0 and alive[d]}
        for j, m in enumerate(min_genes):
            if length >= m:
                pairs[j] += len(nodes)
    return pairs, int(np.count_nonzero(alive))


def mean_of(pairs, n_alive):
    """what statistics.mean returns for n_alive ints that sum to pairs (0 for no node, as the drivers say)"""
    if n_alive == 0:
        return 0
    q = Fraction(pairs, n_alive)
    return int(q) if q.denominator == 1 else float(q)


def _live_amr(tokens, tok_node, alive, flags, a, n_win, k):
    """per window of one read: (node or -1 where not live, AMR window?)"""
    bit = token_flags(tokens[a:a + n_win + k - 1], flags) if n_win else np.zeros(0, bool)
    out = []
    for i in range(n_win):
        d = int(tok_node[a + i])
        out.append((d if d >= 0 and alive[d] else -1, bool(bit[i:i + k].any())))
    return out


def non_amr_nodes(tokens, read_off, tok_node, alive, k, flags):
    """B: ascending ids of the alive nodes that no read with a live AMR window has a live window on"""
    keep = np.zeros(len(alive), bool)
    for _, a, _, n_win in _reads(read_off, k):
        wins = _live_amr(tokens, tok_node, alive, flags, a, n_win, k)
        if any(d >= 0 and amr for d, amr in wins):
            for d, _ in wins:
                if d >= 0:
                    keep[d] = True
    return np.flatnonzero((np.asarray(alive) != 0) & ~keep).astype(np.int32)


def component_amr_reads(tokens, read_off, tok_node, alive, component, n_components, k, flags, min_genes):
    """C: (n_reads, n_long), entry c for the component with id c + 1 (ids start at 1)"""
    n_reads, n_long = np.zeros(n_components, np.int64), np.zeros(n_components, np.int64)
    for _, a, length, n_win in _reads(read_off, k):
        labels = {int(component[d]) for d, amr in _live_amr(tokens, tok_node, alive, flags, a, n_win, k) if d >= 0 and amr}
        for c in labels:
            n_reads[c - 1] += 1
            n_long[c - 1] += 1 if length >= min_genes else 0
    return n_reads, n_long


def components_valid(n_reads, n_long):
    """choose_kmer_size's test per component: no read, or at least 80 % of them long (the reference's float expression)"""
    return [n == 0 or m / n >= 0.8 for n, m in zip(n_reads.tolist(), n_long.tolist())]
