"""GPU: the read walks of amira_amd/csrc/amg_read_walk.hip — depth by read length (A), AMR trimming (B), AMR reads per
component (C) — against tests/read_walk_oracle.py on hand-made token arrays, and through the drop-in against the
pure-Python amira_oracle.  Integer equality throughout.

Not built, because the engine cannot reach it: a read whose AMR windows lie in two or three components.  Component ids
are those of the graph AS BUILT (the reference labels once, in __init__, and keeps the labels through every removal),
and the windows of a read are joined by edges when the graph is built: whatever is removed later, the live windows of
one read carry one label.  What a removal does leave — masked windows between AMR windows of one component, components
without an AMR read, a component without a live node — is tested below."""
import os
import pickle
import re

import numpy as np
import pytest

import procedures as P
import read_walk_oracle as RW

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = open(os.path.join(ROOT, "amira_amd", "csrc", "amg_read_walk.hip")).read()
READS_PER_WAVE = int(re.search(r"#define RW_READS_PER_WAVE (\d+)", _SRC).group(1))
LDS_GENES = 32 * int(re.search(r"#define RW_FLAG_WORDS_BUDGET (\d+)", _SRC).group(1))   # genes whose flags fit the LDS budget
CACHE_SLOTS = int(re.search(r"#define RW_CACHE_SLOTS (\d+)", _SRC).group(1))
E_ARG, E_STATE = -2, -3


@pytest.fixture(scope="module")
def engines():
    from amira_amd import Engine
    es = [Engine(0), Engine(0), Engine(0)]
    yield es
    for e in es:
        e.close()


# ------------------------------------------------------------------ read sets
def rc(seg, two_v):
    return (two_v - 1 - seg)[::-1]


def genome_reads(seed, lengths, n_genomes=3, ranks_per_genome=400, period=700, extra_ranks=8):
    """reads of the given lengths cut from n_genomes token sequences over disjoint genes (so: several components),
    either strand; every sequence repeats with `period`, so that a long read comes back to its nodes `period` windows
    later.  Returns (tokens, read_off, two_v, ranks used by every genome)."""
    rng = np.random.default_rng(seed)
    V = n_genomes * ranks_per_genome + extra_ranks
    two_v = 2 * V
    longest = max(max(lengths), 1) if len(lengths) else 1
    genomes = []
    for g in range(n_genomes):
        block = V + g * ranks_per_genome + rng.integers(0, ranks_per_genome, period)
        genomes.append(np.tile(block, longest // period + 2).astype(np.int32))
    rows = []
    for i, n in enumerate(lengths):
        seq = genomes[i % n_genomes]
        start = int(rng.integers(0, len(seq) - n + 1))
        seg = seq[start:start + n]
        rows.append(rc(seg, two_v) if rng.random() < 0.5 else seg)
    return pack(rows) + (two_v,)


def pack(rows):
    off = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=off[1:])
    toks = np.concatenate([np.asarray(r, np.int32) for r in rows]) if len(rows) and off[-1] else np.zeros(0, np.int32)
    return toks.astype(np.int32), off


def flags_for(two_v, ranks):
    f = np.zeros(two_v // 2, np.uint8)
    f[np.asarray(list(ranks), np.int64)] = 1
    return f


def ranks_of(tokens, two_v):
    V = two_v // 2
    tokens = np.asarray(tokens, np.int64)
    return np.where(tokens >= V, tokens - V, V - 1 - tokens)


def some_flags(tokens, two_v, seed):
    """none, all, and two sparse choices among the genes the reads hold"""
    V = two_v // 2
    rng = np.random.default_rng(seed)
    present = np.unique(ranks_of(tokens, two_v)) if len(tokens) else np.zeros(0, np.int64)
    out = [np.zeros(V, np.uint8), np.ones(V, np.uint8)]
    for n in (1, 5):
        if len(present):
            out.append(flags_for(two_v, rng.choice(present, min(n, len(present)), replace=False)))
    return out


# ------------------------------------------------------------------ the checks
def build(e, tokens, off, two_v, k, after=None):
    e.set_reads(tokens, off, two_v)
    e.build(k)
    if after is not None:
        after(e)


def lengths_asked(k):
    return [0, 1, k - 1, k, k + 1, 2 * k - 1, 63, 64, 65, 64 + k, 130, 131, 1100, 2500, 2501, 1 << 30]   # 16 of them


def check_a_and_c(e, tokens, off, two_v, k, flag_sets):
    tok_node, nodes = e.read_node_ids(), e.nodes()
    alive, comp, n_comp = nodes["alive"], nodes["component"], e.counts()["n_components"]
    mg = lengths_asked(k)
    pairs, n_alive = e.depth_by_length(mg)
    want_pairs, want_alive = RW.depth_by_length(off, tok_node, alive, k, mg)
    assert pairs.tolist() == want_pairs and n_alive == want_alive
    one, _ = e.depth_by_length([k])   # (a single length)
    assert one.tolist() == [want_pairs[3]]
    for flags in flag_sets:
        for m in (k, 2 * k - 1):
            n_reads, n_long = e.component_amr_reads(flags, m)
            w_reads, w_long = RW.component_amr_reads(tokens, off, tok_node, alive, comp, n_comp, k, flags, m)
            assert n_reads.dtype == np.int64 and n_reads.tolist() == w_reads.tolist(), (k, m)
            assert n_long.tolist() == w_long.tolist(), (k, m)
    return want_pairs, (tok_node, alive, comp, n_comp)


def check_b(e1, e2, tokens, off, two_v, k, flags, after=None, correct=True):
    """B against the route that exists: e1 gets the oracle's ids through remove_nodes, e2 the device call"""
    build(e1, tokens, off, two_v, k, after)
    build(e2, tokens, off, two_v, k, after)
    ids = RW.non_amr_nodes(tokens, off, e1.read_node_ids(), e1.nodes()["alive"], k, flags)
    e1.remove_nodes(ids)
    assert e2.remove_non_amr_nodes(flags) == len(ids)
    assert np.array_equal(e1.nodes()["alive"], e2.nodes()["alive"])
    assert np.array_equal(e1.edges()["alive"], e2.edges()["alive"])
    assert np.array_equal(e1.read_node_ids(), e2.read_node_ids())
    assert np.array_equal(e1.reads_to_correct(), e2.reads_to_correct())
    assert e1.counts() == e2.counts()
    assert e2.remove_non_amr_nodes(flags) == 0      # nothing is left to trim
    assert np.array_equal(e1.nodes()["alive"], e2.nodes()["alive"])
    if correct:
        (r1, t1), (r2, t2) = e1.correct_reads(), e2.correct_reads()
        assert (r1, t1) == (r2, t2)
        c1, c2 = e1.corrected(r1, t1, False), e2.corrected(r2, t2, False)
        for key in ("tokens", "read_offsets", "orig_read", "changed"):
            assert np.array_equal(c1[key], c2[key]), key
    return len(ids)


def check_all(engines, tokens, off, two_v, k, flag_sets, after=None, correct=True):
    e0, e1, e2 = engines
    build(e0, tokens, off, two_v, k, after)
    out = check_a_and_c(e0, tokens, off, two_v, k, flag_sets)
    removed = [check_b(e1, e2, tokens, off, two_v, k, flags, after, correct) for flags in flag_sets]
    return out, removed


# ------------------------------------------------------------------ read counts and lengths
@pytest.mark.parametrize("n_reads", [0, 1, READS_PER_WAVE - 1, READS_PER_WAVE, READS_PER_WAVE + 1, 4 * READS_PER_WAVE + 1, 300])
def test_read_counts(engines, n_reads):
    rng = np.random.default_rng(n_reads)
    lengths = rng.choice([0, 1, 2, 3, 4, 6, 9, 17, 40], n_reads).tolist()
    tokens, off, two_v = genome_reads(100 + n_reads, lengths, ranks_per_genome=60, period=90)
    check_all(engines, tokens, off, two_v, 3, some_flags(tokens, two_v, n_reads))


def read_lengths(k):
    return [0, k - 1, k, k + 1, 63, 64, 65, 64 + k - 1, 64 + k, 130, 1100, 2500]


@pytest.mark.parametrize("k", [3, 15])
def test_read_lengths(engines, k):
    lengths = read_lengths(k) + read_lengths(k)[::-1]   # every length from two genomes at least
    tokens, off, two_v = genome_reads(7 * k, lengths)
    (pairs, (tok_node, alive, _, _)), removed = check_all(engines, tokens, off, two_v, k, some_flags(tokens, two_v, k))
    # the long reads do come back to nodes they have visited: fewer pairs than live windows
    assert pairs[0] < int((tok_node >= 0).sum())
    assert removed[0] == int(alive.sum()) and removed[1] == 0   # no gene of interest: every node goes; all: none


def test_mixed_set_at_k9(engines):
    rng = np.random.default_rng(9)
    lengths = rng.choice([0, 5, 8, 9, 10, 17, 56, 64, 65, 72, 73, 130, 300], 120).tolist()
    tokens, off, two_v = genome_reads(99, lengths, period=150)
    check_all(engines, tokens, off, two_v, 9, some_flags(tokens, two_v, 9))


# ------------------------------------------------------------------ revisited nodes
def test_revisited_nodes_count_once(engines):
    k, V = 3, 3000
    two_v = 2 * V
    a, b, c = V + 1, V + 2, V + 3
    fill = iter(range(V + 10, two_v))

    def filler(n):
        return [next(fill) for _ in range(n)]

    rows = [[a, b, c, a, b, c],
            [a, b, c, two_v - 1 - c, two_v - 1 - b, two_v - 1 - a],          # the same node through its reverse complement
            [a, b, c] + filler(67) + [a, b, c],                              # 70 windows apart: the next chunk
            [a, b, c] + filler(1197) + [a, b, c],                            # 1 200 windows apart
            [V + 5] * 202,                                                   # one node 200 times
            [V + 6] * 70 + filler(3) + [V + 6] * 70]
    tokens, off = pack(rows)
    e0 = engines[0]
    build(e0, tokens, off, two_v, k)
    tok_node = e0.read_node_ids()
    pairs, n_alive = e0.depth_by_length([0])
    # per read: distinct nodes, counted by hand (second read: b c -c and c -c -b are one node as well)
    per_read = [3, 2, 70, 1200, 1, 6]
    assert [len(set(tok_node[off[r]:off[r + 1] - k + 1].tolist())) for r in range(len(rows))] == per_read
    assert pairs.tolist() == [sum(per_read)]
    flag_sets = [flags_for(two_v, [1]), flags_for(two_v, [5, 6]), flags_for(two_v, [V - 1])]
    check_all(engines, tokens, off, two_v, k, flag_sets)


# ------------------------------------------------------------------ genes of interest
def test_gene_positions_within_reads(engines):
    """a gene that occurs only as the first token of a read, only as the last, only in reads shorter than k"""
    k = 3
    tokens, off, two_v = genome_reads(21, [20, 30, 66, 70, 12, 9, 40, 64, 65, 2, 2], ranks_per_genome=50, period=80, extra_ranks=8)
    V = two_v // 2
    first, last, short = V - 1, V - 2, V - 3     # ranks no genome uses (extra_ranks)
    rows = [tokens[off[r]:off[r + 1]].copy() for r in range(len(off) - 1)]
    rows[2][0] = V + first           # '+' strand, first token of a 66-gene read
    rows[3][-1] = V - 1 - last       # '-' strand, last token of a 70-gene read (in its last window only, in the second chunk)
    rows[7][-1] = V + last           # last token of a 64-gene read
    rows[9][1] = V + short           # in reads of 2 genes only: no AMR window anywhere
    rows[10][0] = V - 1 - short
    tokens, off = pack(rows)
    flag_sets = [flags_for(two_v, [first]), flags_for(two_v, [last]), flags_for(two_v, [short]),
                 flags_for(two_v, [first, last, short])]
    e0 = engines[0]
    build(e0, tokens, off, two_v, k)
    _, (tok_node, alive, comp, n_comp) = check_a_and_c(e0, tokens, off, two_v, k, flag_sets)
    for flags, hits in zip(flag_sets, (1, 2, 0, 3)):
        assert int(e0.component_amr_reads(flags, 0)[0].sum()) == hits
    removed = [check_b(engines[1], engines[2], tokens, off, two_v, k, flags) for flags in flag_sets]
    assert removed[2] == int(alive.sum())


@pytest.mark.parametrize("V", [1, 37, LDS_GENES, LDS_GENES + 1, 50000])
def test_vocabulary_sizes(engines, V):
    """V = 1; V no multiple of 8 or 64; the flag bitmap on both sides of the LDS budget (and exactly at it)"""
    rng = np.random.default_rng(V)
    two_v = 2 * V
    lengths = rng.choice([2, 3, 4, 7, 30, 64, 70], 60).tolist()
    # reads over a few genes at both ends of the rank range, so that the last rank (the last bit of the bitmap) is in use
    pool = np.unique(np.concatenate([np.arange(min(V, 6)), V - 1 - np.arange(min(V, 6))]))
    rows = []
    for n in lengths:
        r = rng.choice(pool, n)
        rows.append(np.where(rng.random(n) < 0.5, V + r, V - 1 - r).astype(np.int32))
    tokens, off = pack(rows)
    flag_sets = [np.zeros(V, np.uint8), np.ones(V, np.uint8), flags_for(two_v, [V - 1]), flags_for(two_v, [0])]
    if V > 64:
        flag_sets.append(flags_for(two_v, [31, 32, 63, 64, V - 2]))   # flagged genes no read holds
    check_all(engines, tokens, off, two_v, 3, flag_sets)


# ------------------------------------------------------------------ after removals
def test_after_filter_and_listed_removals(engines):
    k = 3
    rng = np.random.default_rng(5)
    lengths = rng.choice([3, 5, 9, 20, 40, 66, 90], 240).tolist()
    tokens, off, two_v = genome_reads(55, lengths, n_genomes=4, ranks_per_genome=40, period=60)
    V = two_v // 2
    # genes of interest in genomes 0 and 2 only: the components of genomes 1 and 3 have no AMR read
    flag_sets = [flags_for(two_v, [3, 7, 2 * 40 + 5]), flags_for(two_v, [2 * 40 + 1]), np.ones(V, np.uint8)]
    state = {}

    def after(e):
        e.filter(3, 1)
        nodes = e.nodes()
        comp, alive = nodes["component"], nodes["alive"] != 0
        toks = nodes["tokens"]
        # every node of the last genome's largest component dies, and some nodes of the first genome's
        in_last = (ranks_of(toks[:, 0], two_v) >= 3 * 40) & alive
        label = np.bincount(comp[in_last]).argmax()
        ids = np.flatnonzero(comp == label)
        some = np.flatnonzero((ranks_of(toks[:, 0], two_v) < 40) & alive)[::5]
        e.remove_nodes(np.concatenate([ids, some]).astype(np.int32))
        state["dead_label"] = int(label)

    (_, (tok_node, alive, comp, n_comp)), removed = check_all(engines, tokens, off, two_v, k, flag_sets, after)
    assert (tok_node == -2).any()                                   # masked windows
    assert not alive[comp == state["dead_label"]].any()             # a component all of whose nodes are dead
    n_reads, _ = engines[0].component_amr_reads(flag_sets[2], 0)    # (engine 0 still holds the state after `after`)
    assert n_reads[state["dead_label"] - 1] == 0 and (n_reads > 0).any()
    n_reads, _ = engines[0].component_amr_reads(flag_sets[0], 0)
    labels_alive = np.unique(comp[alive != 0])
    assert any(n_reads[c - 1] == 0 for c in labels_alive)           # a live component without any AMR read
    # reads with several AMR windows of one component, some of them masked, count once
    bit = RW.token_flags(tokens, flag_sets[0])
    several = [r for r in range(len(off) - 1) if bit[off[r]:off[r + 1]].sum() >= 2
               and (tok_node[off[r]:off[r + 1]] == -2).any() and (tok_node[off[r]:off[r + 1]] >= 0).any()]
    assert several
    assert 0 < removed[0] and removed[2] == 0


def test_more_components_than_cache_slots(engines):
    """every read a component of its own, more of them than a workgroup sums up in LDS: the labels that find their slot
    taken go to global memory one by one"""
    n, k = 3 * CACHE_SLOTS + 17, 3
    V = 5 * n
    rows = [V + 5 * r + np.arange(5, dtype=np.int32) for r in range(n)]     # read r makes the component with id r + 1
    # then reads that come back to the components c, c + slots, c + 2 slots side by side: one workgroup, one slot
    rows += [rows[(j % 3) * CACHE_SLOTS + j // 3][:4] for j in range(96)]
    tokens, off = pack(rows)
    e0 = engines[0]
    build(e0, tokens, off, 2 * V, k)
    assert e0.counts()["n_components"] == n
    flags = np.ones(V, np.uint8)
    flags[5 * 7:5 * 8] = 0
    check_a_and_c(e0, tokens, off, 2 * V, k, [flags])
    n_reads, n_long = e0.component_amr_reads(flags, 5)
    want = np.ones(n, np.int64)
    for j in range(96):
        want[(j % 3) * CACHE_SLOTS + j // 3] += 1
    want[7] = 0
    assert n_reads.tolist() == want.tolist() and n_long.tolist() == [min(int(x), 1) for x in want]


# ------------------------------------------------------------------ refusals
def test_refusals(engines):
    import ctypes as C
    from amira_amd import Engine, _ffi
    fresh = Engine(0)
    try:
        fresh.set_reads(np.array([2, 3, 2], np.int32), np.array([0, 3], np.int64), 4)
        two, room, nc = np.ones(2, np.uint8), np.zeros(4, np.int64), C.c_int64(0)
        for call in (lambda: fresh.depth_by_length([3]), lambda: fresh.remove_non_amr_nodes(two),
                     lambda: _ffi.check(_ffi.lib.amg_component_amr_reads(fresh._h, _ffi.ptr(two), 3, 4, _ffi.ptr(room),
                                                                         _ffi.ptr(room), C.byref(nc)))):
            with pytest.raises(_ffi.AmgError) as err:
                call()
            assert err.value.code == E_STATE          # before a build
    finally:
        fresh.close()
    e = engines[0]
    tokens, off, two_v = genome_reads(1, [10, 20, 30, 8, 8, 8])
    build(e, tokens, off, two_v, 3)
    for mg in ([], list(range(17))):
        with pytest.raises(_ffi.AmgError) as err:
            e.depth_by_length(mg)
        assert err.value.code == E_ARG
    flags = np.ones(two_v // 2, np.uint8)
    n_comp = e.counts()["n_components"]
    assert n_comp >= 2
    room = np.full(n_comp, -7, np.int64)
    nc = C.c_int64(-1)
    rc_ = _ffi.lib.amg_component_amr_reads(e._h, _ffi.ptr(flags), 3, n_comp - 1, _ffi.ptr(room), _ffi.ptr(room), C.byref(nc))
    assert rc_ == E_ARG and nc.value == n_comp and (room == -7).all()     # the size is reported, nothing else written
    rc_ = _ffi.lib.amg_depth_by_length(e._h, None, 1, _ffi.ptr(room), C.byref(nc))
    assert rc_ == E_ARG
    rc_ = _ffi.lib.amg_remove_non_amr_nodes(e._h, _ffi.ptr(flags), None)
    assert rc_ == E_ARG
    assert e.remove_non_amr_nodes(flags) == 0      # (the graph is as it was)


# ------------------------------------------------------------------ through the drop-in
def _oracle():
    import types
    import amira_oracle
    from amira_oracle import driver
    return types.SimpleNamespace(GeneMerGraph=amira_oracle.GeneMerGraph, choose_kmer_size=driver.choose_kmer_size,
                                 get_overall_mean_node_coverages=driver.get_overall_mean_node_coverages)


def _product():
    import types
    import amira_amd
    from amira_amd import graph_utils as gu
    return types.SimpleNamespace(GeneMerGraph=amira_amd.GeneMerGraph, choose_kmer_size=gu.choose_kmer_size,
                                 get_overall_mean_node_coverages=gu.get_overall_mean_node_coverages)


GENES = [f"amr{j}" for j in range(4)]


@pytest.fixture(scope="module")
def synth():
    return P.synth_inputs(3, 300, 30, 300, 0.03, n_amr=4)


def test_drop_in_mean_coverages_values_and_types(synth):
    reads, pos, _ = synth
    got, want = [], []
    for impl, out in ((_product(), got), (_oracle(), want)):
        for k in (3, 5):
            g = impl.GeneMerGraph(dict(reads), k, dict(pos))
            out.append(impl.get_overall_mean_node_coverages(g))
            g.filter_graph(3, 1)
            out.append(impl.get_overall_mean_node_coverages(g))
    assert got == want
    assert [{k: type(v) for k, v in d.items()} for d in got] == [{k: type(v) for k, v in d.items()} for d in want]
    # a read set whose means are whole numbers: ints, as statistics.mean gives them
    whole = {f"r{i}": ["+a", "+b", "+c", "+d"] for i in range(6)}
    got = _product().get_overall_mean_node_coverages(_product().GeneMerGraph(whole, 3))
    assert got == _oracle().get_overall_mean_node_coverages(_oracle().GeneMerGraph(whole, 3))
    assert got[3] == 6 and type(got[3]) is int and got[5] == 0 and type(got[5]) is int


def test_drop_in_choose_kmer_size(synth):
    reads, pos, _ = synth
    assert _product().choose_kmer_size(25, reads, 1, pos, GENES) == _oracle().choose_kmer_size(25, reads, 1, pos, GENES)
    assert _product().choose_kmer_size(5, reads, 1, pos, GENES) == 3
    assert _product().choose_kmer_size(25, reads, 1, pos, ["no_such_gene"]) == 15     # no AMR read anywhere: every k is valid


def test_drop_in_choose_kmer_size_beyond_k5():
    """the long synthetic reads of procedures.p_drivers_synth, cut to ragged lengths so that the rule stops at a chosen
    k; a smaller set than the golden cases so that the pure-Python oracle builds its seven graphs in seconds"""
    for keep, at_least in (([40, 36, 30, 24, 18, 14, 13, 13, 13, 10], 7), ([44, 40, 36, 33, 31, 30, 29, 29, 29, 12], 9)):
        reads, pos, _ = P.synth_inputs(41, 90, 44, 120, 0.002, n_amr=4)
        for i, r in enumerate(list(reads)):
            n = keep[i % len(keep)]
            reads[r], pos[r] = reads[r][:n], pos[r][:n]
        got = _product().choose_kmer_size(25, reads, 1, pos, GENES)
        assert got == _oracle().choose_kmer_size(25, reads, 1, pos, GENES)
        assert got >= at_least


def test_choose_kmer_size_makes_no_object_view(synth, monkeypatch):
    from amira_amd import GeneMerGraph
    reads, pos, _ = synth
    made, graphs = [], []
    real_v, real_close = GeneMerGraph._v, GeneMerGraph.close

    def counting_v(self):
        made.append(self._kmerSize)
        return real_v(self)

    def noting_close(self):
        graphs.append((self._kmerSize, getattr(self, "_view", None)))
        return real_close(self)

    monkeypatch.setattr(GeneMerGraph, "_v", counting_v)
    monkeypatch.setattr(GeneMerGraph, "close", noting_close)
    _product().choose_kmer_size(25, reads, 1, pos, GENES)
    assert made == []
    assert sorted({k for k, _ in graphs}) == list(range(3, 16, 2)) and all(view is None for _, view in graphs)


def test_drop_in_trim_then_correct(synth):
    reads, pos, fq = synth
    out = []
    for impl in (_product(), _oracle()):
        g = impl.GeneMerGraph(dict(reads), 3, {r: list(v) for r, v in pos.items()})
        g.filter_graph(2, 1)
        g.remove_non_AMR_associated_nodes(GENES[:2])
        new_reads, new_pos = g.correct_reads(fq)
        out.append(({r: list(new_reads[r]) for r in new_reads}, {r: [tuple(p) for p in new_pos[r]] for r in new_pos},
                    len(g.get_nodes()), sorted(g.get_reads_to_correct())))
    assert out[0] == out[1]
    assert 0 < out[0][2]


def test_pickle_after_trim(synth):
    from amira_amd import GeneMerGraph
    reads, pos, _ = synth
    g = GeneMerGraph(dict(reads), 3, dict(pos))
    g.filter_graph(2, 1)
    before = int(g._engine.nodes()["alive"].sum())
    g.remove_non_AMR_associated_nodes(GENES[:1])
    assert g._view is None and int(g._engine.nodes()["alive"].sum()) < before
    h = pickle.loads(pickle.dumps(g))
    for key in ("alive", "coverage", "component", "tokens"):
        assert np.array_equal(g._engine.nodes()[key], h._engine.nodes()[key]), key
    assert np.array_equal(g._engine.edges()["alive"], h._engine.edges()["alive"])
    assert np.array_equal(g._engine.read_node_ids(), h._engine.read_node_ids())
    assert np.array_equal(g._engine.reads_to_correct(), h._engine.reads_to_correct())
    g.remove_non_AMR_associated_nodes(["no_such_gene"])      # unknown names flag nothing: every node goes
    assert g.get_total_number_of_nodes() == 0
    g.close()
    h.close()
