"""GPU: the batched sub-list search (amg_match_patterns / k_match, amg_match.hip) against a plain numpy reference
(match_oracle.py) in every regime the kernel has: rows longer than the 64 lanes of a wave, row ends and the last k - 1
places of a read, read counts around the batches of four and the grid stride, the first-symbol bitmap in LDS and in
global memory, long buckets, duplicated and self-overlapping patterns, one-node patterns over the node ids of a
graph, the two-call protocol, the limits of the packed hits, and the chunks of the host wrapper.  Everything is
integer equality of (offsets, hit_read, hit_pos), the order of the hits included.  Every case that is meant for a
regime asserts from the reference's result, or from the launch formulas below, that it is in it, and the last test of
the module asserts that every regime was met (it needs the whole module to have run)."""
import numpy as np
import pytest

import procedures as P
from match_oracle import match_reference, match_reference_single

pytestmark = pytest.mark.gpu

WAVE = 64                # positions of a row a wave looks at before it decides to walk it
MATCH_BATCH = 4          # rows a wave loads per iteration
READS_PER_BLOCK = 16     # 4 waves x MATCH_BATCH
MAX_BLOCKS = 4096
LDS_WORDS = 12288        # MATCH_LDS_WORDS: bitmap words staged in LDS
POS_BITS = 20
PAT_BITS = 16
E_ARG, E_STATE = -2, -3
K = 5                    # odd: no gene-mer is its own reverse complement
LENGTHS = [63, 64, 65, 127, 128, 129, 150]

SEEN = set()  # regimes met by the cases of this module (test_every_regime_was_seen)
REGIMES = ({f"{w}: {x}" for w in ("tokens", "nodes") for x in
            ("hit beyond 63", "row with hits only beyond 63", "one long row in a batch of four",
             "every row length", "pattern is a whole row", "pattern ends on the last symbol")}
           | {"match only by running into the tail", "pattern longer than every row", "row shorter than k", "empty row",
              "no reads", "one batch a wave", "second batch of a wave", "third batch of a wave",
              "last batch of 1", "last batch of 2", "last batch of 3", "hit in the last row of a partial batch",
              "hits either side of read 65536", "bitmap in LDS, last domain", "bitmap in global memory",
              "first symbol in the last bit", "first symbol in the last full word", "bucket of 2000",
              "pattern given three times", "overlapping hits", "more hits than lanes", "1000 patterns a bucket",
              "every live node", "every live node after a filter", "hit at the last position of 2^20",
              "two chunks of the host wrapper"})


def launch(n_reads):
    """(workgroups, waves, batches) of k_match over n_reads"""
    blocks = min(-(-n_reads // READS_PER_BLOCK), MAX_BLOCKS)
    return blocks, 4 * blocks, -(-n_reads // MATCH_BATCH)


def bitmap_in_lds(domain):
    return (domain + 31) // 32 + 1 <= LDS_WORDS


@pytest.fixture(scope="module")
def eng():
    from amira_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def csr(rows):
    offs = np.zeros(len(rows) + 1, np.int64)
    np.cumsum([len(r) for r in rows], out=offs[1:])
    seq = np.concatenate([np.asarray(r, np.int32) for r in rows]) if offs[-1] else np.zeros(0, np.int32)
    return seq.astype(np.int32), offs


def search(eng, which, seq, offs, tail, pats, domain, single=False):
    """one call against the reference; returns the reference's (offsets, hit_read, hit_pos)"""
    got = eng.match_patterns(which, pats)
    if single:
        want = match_reference_single(seq, offs, tail, [p[0] for p in pats], domain)
    else:
        want = match_reference(seq, offs, tail, pats, domain)
    for name, g, w in zip(("offsets", "hit_read", "hit_pos"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.shape, w.shape)
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, (which, name, bad[:8], g[bad[:8]], w[bad[:8]])
    return want


def hits_of(want, j):
    off, hr, hp = want
    return hr[off[j]:off[j + 1]], hp[off[j]:off[j + 1]]


def windows_of(rng, seq, offs, tail, n, longest):
    """n patterns cut out of the searched part of random rows"""
    lens = np.diff(offs) - tail
    rows = np.flatnonzero(lens >= 1)
    pats = []
    for _ in range(n):
        r = int(rows[rng.integers(0, rows.size)])
        m = int(rng.integers(1, min(longest, lens[r]) + 1))
        s = int(offs[r] + rng.integers(0, lens[r] - m + 1))
        pats.append(seq[s:s + m].tolist())
    return pats


def base_reads(seed):
    """40 reads of 150 genes that go round a loop of 60 genes more than twice, as lists of gene strings"""
    return list(P.synth_inputs(seed, 40, 150, 60, 0.05)[0].values())


def build_nodes(eng, gene_lists, k=K):
    """(node id per window as the device holds it, read offsets, number of nodes) of a build over gene_lists"""
    from amira_amd import tokenize
    vocab, toks, offs, _ = tokenize({f"r{i:05d}": g for i, g in enumerate(gene_lists)})
    eng.set_reads(toks, offs, vocab.two_v)
    eng.build(k)
    return eng.read_node_ids(), offs, eng.graph_sizes()[0]


def set_tokens(eng, rows, two_v):
    seq, offs = csr(rows)
    eng.set_reads(seq, offs, two_v)
    return seq, offs


# ------------------------------------------------------------------ long rows
def long_row_cases(side, eng, which, seq, offs, tail, domain, long_rows):
    """a call per pattern row[s : s + m] for s in {63, 64, 65, len - m} of every row of long_rows, m = 1 and 2; from the
    reference: is the hit beyond the wave's first look, has the row hits only there, is it the only row of its batch
    that is walked"""
    lens = np.diff(offs) - tail
    met_lengths = set()
    for r in long_rows:
        n = int(lens[r])
        row = seq[offs[r]:offs[r] + n]
        for m in (1, 2):
            for s in sorted({63, 64, 65, n - m}):
                if s < 0 or s + m > n:
                    continue
                pat = row[s:s + m].tolist()
                want = search(eng, which, seq, offs, tail, [pat], domain)
                hr, hp = want[1], want[2]
                assert ((hr == r) & (hp == s)).any()
                if (hp >= WAVE).any():
                    SEEN.add(f"{side}: hit beyond 63")
                mine = hp[hr == r]
                if mine.min() >= WAVE and pat[0] not in row[:WAVE]:    # nothing in the wave's first look starts it
                    SEEN.add(f"{side}: row with hits only beyond 63")
                    met_lengths.add(n)
                    b = r - r % MATCH_BATCH
                    others = [q for q in range(b, min(b + MATCH_BATCH, len(lens))) if q != r]
                    if len(others) == 3 and all(lens[q] <= WAVE and pat[0] not in seq[offs[q]:offs[q] + max(lens[q], 0)]
                                                for q in others):
                        SEEN.add(f"{side}: one long row in a batch of four")
    if met_lengths >= {n for n in LENGTHS if n > WAVE}:
        SEEN.add(f"{side}: every row length")


def test_long_rows_of_tokens(eng):
    rng = np.random.default_rng(1)
    fill, marker, two_v = 10, 100, 2000       # symbols below `fill` are everywhere; a marker occurs once
    rows, long_rows, pats = [], [], []
    for j, n in enumerate(LENGTHS * 2):
        row = rng.integers(0, fill, n)
        for s in sorted({63, 64, 65, n - 1, n - 2}):
            if 0 <= s < n:
                row[s] = marker
                marker += 1
        batch = [rng.integers(0, fill, int(x)) for x in rng.choice([0, 1, 20, 63, 64], 3)]
        batch.insert(j % MATCH_BATCH, row)
        long_rows.append(len(rows) + j % MATCH_BATCH)
        rows += batch
    rows += [rng.integers(0, fill, 150), rng.integers(0, fill, 129)]   # and a last batch of two long rows
    seq, offs = set_tokens(eng, rows, two_v)
    assert sorted(set(np.diff(offs)[long_rows].tolist())) == LENGTHS
    long_row_cases("tokens", eng, 0, seq, offs, 0, two_v, long_rows)
    # all markers in one call, then windows cut out anywhere: hits at every position of every row
    markers = [[int(x)] for x in np.unique(seq[seq >= 100])] + [[int(seq[i]), int(seq[i + 1])] for i in np.flatnonzero(seq[:-1] >= 100)]
    want = search(eng, 0, seq, offs, 0, markers, two_v)
    assert (want[2] >= WAVE).sum() > 40
    want = search(eng, 0, seq, offs, 0, windows_of(rng, seq, offs, 0, 200, 6) + markers, two_v)
    assert (want[2] >= WAVE).sum() > 500 and (want[2] >= 2 * WAVE).sum() > 20


def test_long_rows_of_nodes(eng):
    base = base_reads(11)
    lists, long_rows = [], []
    for j, n in enumerate(LENGTHS * 4):
        batch = [base[(j + 13 * (i + 1)) % 40][:w + K - 1] for i, w in enumerate((64, 20, 1))]
        batch.insert(j % MATCH_BATCH, (base[j % 40] + base[j % 40])[:n + K - 1])   # (150 windows: the read and k - 1 more)
        long_rows.append(len(lists) + j % MATCH_BATCH)
        lists += batch
    ids, offs, n_nodes = build_nodes(eng, lists)
    tail = K - 1
    assert sorted(set((np.diff(offs) - tail)[long_rows].tolist())) == LENGTHS
    long_row_cases("nodes", eng, 1, ids, offs, tail, n_nodes, long_rows)
    rng = np.random.default_rng(2)
    want = search(eng, 1, ids, offs, tail, windows_of(rng, ids, offs, tail, 300, 6), n_nodes)
    assert (want[2] >= WAVE).sum() > 100


# ------------------------------------------------------------------ row ends and the tail
def end_patterns(side, seq, offs, tail, rows):
    """whole rows, patterns that end on a row's last symbol, patterns longer than every row"""
    lens = np.diff(offs) - tail
    pats = []
    for r in rows:
        row = seq[offs[r]:offs[r] + lens[r]].tolist()
        pats += [row, row[-1:], row[-3:], row[1:], row + row[:1], row + [0] * 60]
    return pats, int(lens.max())


def note_ends(side, want, pats, offs, tail, longest):
    lens = np.diff(offs) - tail
    for j, p in enumerate(pats):
        hr, hp = hits_of(want, j)
        if ((hp == 0) & (lens[hr] == len(p))).any():
            SEEN.add(f"{side}: pattern is a whole row")
        if ((hp + len(p) == lens[hr]) & (hp > 0)).any():
            SEEN.add(f"{side}: pattern ends on the last symbol")
        if len(p) > longest:
            assert hr.size == 0
            SEEN.add("pattern longer than every row")


def test_row_ends_of_tokens(eng):
    from amira_amd import tokenize
    vocab, toks, offs, _ = tokenize({f"r{i:05d}": g for i, g in enumerate(
        [[], base_reads(3)[0][:1]] + base_reads(3) + [base_reads(3)[1][:2], []])})
    eng.set_reads(toks, offs, vocab.two_v)
    pats, longest = end_patterns("tokens", toks, offs, 0, [1, 2, 3, 17, 41, 42])
    want = search(eng, 0, toks, offs, 0, pats, vocab.two_v)
    note_ends("tokens", want, pats, offs, 0, longest)
    assert (np.diff(offs) == 0).sum() == 2
    SEEN.add("empty row")


def test_row_ends_and_the_tail_of_nodes(eng):
    base = base_reads(3)
    lists = [[], base[0][:K - 1], base[1][:1]] + base + [base[2][:K], base[3][:K + 1], []]
    ids, offs, n_nodes = build_nodes(eng, lists)
    tail = K - 1
    lens = np.diff(offs) - tail
    assert (lens < 0).sum() == 3 and (lens == 0).sum() == 1 and (lens == 1).sum() == 1
    SEEN.add("row shorter than k")
    pats, longest = end_patterns("nodes", ids, offs, tail, [3, 4, 20, 42, 43, 44])
    want = search(eng, 1, ids, offs, tail, pats, n_nodes)
    note_ends("nodes", want, pats, offs, tail, longest)
    # a real end of a row, extended by what the device holds in the last k - 1 places: the array holds the pattern there,
    # the row does not
    pats, places = [], []
    for r in (3, 4, 20, 42, 43, 44):
        n = int(lens[r])
        for back, beyond in ((2, 1), (1, 1), (1, tail), (3, 2)):
            if back <= n:
                s = int(offs[r]) + n - back
                pats.append(ids[s:s + back + beyond].tolist())
                places.append((r, n - back))
    want = search(eng, 1, ids, offs, tail, pats, n_nodes)
    for j, (r, s) in enumerate(places):
        p = np.asarray(pats[j])
        assert np.array_equal(ids[offs[r] + s:offs[r] + s + len(p)], p) and p[0] >= 0
        hr, hp = hits_of(want, j)
        assert not ((hr == r) & (hp == s)).any()
    SEEN.add("match only by running into the tail")
    # the values of the last places themselves start nothing
    search(eng, 1, ids, offs, tail, [[int(ids[offs[4] - 1])], [int(ids[offs[4] - 1])] * 2, [-1], [-2]], n_nodes)


# ------------------------------------------------------------------ read counts: batches of four, the grid stride
def test_no_reads(eng):
    eng.set_reads(np.zeros(0, np.int32), np.zeros(1, np.int64), 100)
    off, hr, hp = eng.match_patterns(0, [[1], [2, 3], []])
    assert off.tolist() == [0, 0, 0, 0] and hr.size == 0 and hp.size == 0
    assert launch(0) == (0, 0, 0)
    SEEN.add("no reads")


N_READS = [1, 2, 3, 5, 65535, 65536, 65537, 65536 + 4 * MAX_BLOCKS * MATCH_BATCH + 3]


@pytest.mark.parametrize("n_reads", N_READS)
def test_read_counts(eng, n_reads):
    rng = np.random.default_rng(n_reads)
    two_v = 4096
    lens = rng.integers(2, 5, n_reads)
    offs = np.zeros(n_reads + 1, np.int64)
    np.cumsum(lens, out=offs[1:])
    seq = rng.integers(10, 1010, int(offs[-1])).astype(np.int32)
    # a symbol of its own at the end of the first rows, the last rows and the rows either side of 65 536
    marked = sorted({r for r in list(range(4)) + list(range(n_reads - 5, n_reads)) + list(range(65530, 65543))
                     if 0 <= r < n_reads})
    pats = []
    for j, r in enumerate(marked):
        seq[offs[r + 1] - 1] = 2000 + j
        pats += [[2000 + j], seq[offs[r + 1] - 2:offs[r + 1]].tolist()]
    eng.set_reads(seq, offs, two_v)
    pats += windows_of(rng, seq, offs, 0, 40, 3)
    want = search(eng, 0, seq, offs, 0, pats, two_v)
    hr = want[1]
    for j, r in enumerate(marked):
        assert hits_of(want, 2 * j)[0].tolist() == [r] and hits_of(want, 2 * j + 1)[0].tolist() == [r]
    # the regime, from the launch formulas
    blocks, waves, batches = launch(n_reads)
    rounds = -(-batches // waves)
    assert rounds == (1 if n_reads <= 65536 else 2 if n_reads <= 2 * 65536 else 3)
    SEEN.add({1: "one batch a wave", 2: "second batch of a wave", 3: "third batch of a wave"}[rounds])
    if n_reads % MATCH_BATCH:
        SEEN.add(f"last batch of {n_reads % MATCH_BATCH}")
        if (hr >= n_reads - n_reads % MATCH_BATCH).any() and (hr == n_reads - 1).any():
            SEEN.add("hit in the last row of a partial batch")
    if (hr == 65535).any() and (hr == 65536).any():
        SEEN.add("hits either side of read 65536")
    if n_reads > 65536:
        assert blocks == MAX_BLOCKS and (hr >= waves * MATCH_BATCH).any()        # hits of rows of a later round


# ------------------------------------------------------------------ the first-symbol bitmap
@pytest.mark.parametrize("two_v", [393184, 393186, 393218, 800000])
def test_bitmap_placement(eng, two_v):
    """393 184: the last domain whose bitmap (one spare word included) is staged in LDS; 393 186: the first one tested
    in global memory; 393 218: the first one with symbols in a word beyond the LDS_WORDS that could be staged"""
    rng = np.random.default_rng(two_v)
    d = two_v
    last_full = 32 * (d // 32) - 32            # first bit of the last word that lies wholly inside the domain
    special = [0, 1, 31, 32, 33, d - 1, d - 2, last_full, last_full + 5, last_full + 31, 32 * (LDS_WORDS - 1) - 1,
               32 * (LDS_WORDS - 1), d // 2]
    special = [s for s in special if 0 <= s < d]
    rows = [rng.integers(0, d, int(n)) for n in rng.integers(1, 40, 60)]
    rows += [np.array(special), np.array(special[::-1] * 3), np.array([d - 1]), np.array([d - 1, 0, d - 1])]
    seq, offs = set_tokens(eng, rows, two_v)
    pats = [[s] for s in special] + [[s, t] for s in special for t in special[:3]]
    pats += [[d], [d, 0], [-1], [-5, 0], [d + 31], [2 ** 31 - 1]]          # outside the domain: no hits
    pats += windows_of(rng, seq, offs, 0, 60, 3)
    want = search(eng, 0, seq, offs, 0, pats, d)
    n_sp = len(special)
    assert all(hits_of(want, j)[0].size >= 3 for j in range(n_sp))
    assert want[0][n_sp + 3 * n_sp + 6] == want[0][n_sp + 3 * n_sp]
    if bitmap_in_lds(d):
        assert not bitmap_in_lds(d + 2)
        SEEN.add("bitmap in LDS, last domain")
    else:
        SEEN.add("bitmap in global memory")
    assert hits_of(want, special.index(d - 1))[0].size >= 3 and hits_of(want, special.index(last_full + 31))[0].size >= 3
    SEEN.update({"first symbol in the last bit", "first symbol in the last full word"})


# ------------------------------------------------------------------ buckets
def test_a_bucket_of_2000_and_repeated_patterns(eng):
    rng = np.random.default_rng(7)
    a, two_v = 77, 200
    rows = [rng.integers(0, 40, 400) for _ in range(8)]
    starts = np.arange(50) * 7
    rows[0][starts] = a                       # one long path with the symbol at 50 places
    for r in rows[1:]:
        r[rng.integers(0, 360, 6)] = a
    rows[3][100:140] = rows[0][7:47]          # and a second copy of 40 of its symbols
    seq, offs = set_tokens(eng, rows, two_v)
    # every window of 1 to 40 symbols of the path that begins with the symbol, in the order of _sublist_windows
    pats = [rows[0][s:s + m].tolist() for m in range(1, 41) for s in starts]
    assert len(pats) == 2000 and all(p[0] == a for p in pats)
    SEEN.add("bucket of 2000")
    pats += [pats[1999], pats[57], pats[1999], pats[57], pats[0]]
    want = search(eng, 0, seq, offs, 0, pats, two_v)
    for j in (1999, 57):
        first = [x.tolist() for x in hits_of(want, j)]
        assert first[0] and all([x.tolist() for x in hits_of(want, i)] == first
                                for i in range(2000, 2004) if pats[i] == pats[j])
    assert hits_of(want, 1999)[0].size >= 1 and hits_of(want, 0)[0].size >= 50 + 6
    SEEN.add("pattern given three times")


def test_overlapping_hits_in_rows_of_one_symbol(eng):
    a, two_v = 5, 64
    rows = [np.full(n, a) for n in (1, 2, 3, 64, 65, 130, 200, 1000)] + [np.array([a, a, 6, a, a, a])]
    seq, offs = set_tokens(eng, rows, two_v)
    pats = [[a, a], [a], [a, a, a], [a] * 64, [a] * 65, [a] * 200, [a] * 1001, [a, 6], [a, a]]
    want = search(eng, 0, seq, offs, 0, pats, two_v)
    hr, hp = hits_of(want, 0)
    assert hr.size == sum(len(r) - 1 for r in rows[:-1]) + 3
    assert np.diff(hp[hr == 7]).tolist() == [1] * 998          # every position but the last: each hit overlaps the next
    SEEN.add("overlapping hits")
    assert (hr == 7).sum() > 2 * WAVE                          # a lane of the wave holds more than one hit
    SEEN.add("more hits than lanes")


def test_65535_one_symbol_patterns(eng):
    from amira_amd import _ffi
    rng = np.random.default_rng(9)
    two_v = 50
    rows = [rng.integers(0, two_v, n % 12) for n in range(55)]
    seq, offs = set_tokens(eng, rows, two_v)
    assert seq.size == 285
    syms = rng.integers(0, two_v, (1 << PAT_BITS) - 1)
    pats = [[int(s)] for s in syms]
    want = search(eng, 0, seq, offs, 0, pats, two_v, single=True)
    assert np.bincount(syms).min() >= 1000 and want[0][-1] > 300000
    SEEN.add("1000 patterns a bucket")
    with pytest.raises(_ffi.AmgError) as ei:
        eng.match_patterns(0, pats + [[1]])
    assert ei.value.code == E_ARG
    search(eng, 0, seq, offs, 0, pats[:100], two_v)            # the refusal leaves the context usable


# ------------------------------------------------------------------ one-node patterns: the product's search 1
def test_every_live_node_as_a_pattern(eng):
    ids, offs, n_nodes = build_nodes(eng, base_reads(21))
    tail = K - 1
    assert 0 < n_nodes < (1 << PAT_BITS)
    pats = [[i] for i in range(n_nodes)]
    want = search(eng, 1, ids, offs, tail, pats, n_nodes, single=True)
    assert (np.diff(want[0]) >= 1).all() and want[0][-1] == 40 * (150 - tail)
    assert (np.diff(want[0]) >= 3).sum() > 10                  # a read meets a node of the loop more than twice
    SEEN.add("every live node")
    eng.filter(3, 1)
    alive = np.flatnonzero(eng.nodes()["alive"])
    ids = eng.read_node_ids()
    assert 0 < alive.size < n_nodes and (ids == -2).any()
    want = search(eng, 1, ids, offs, tail, [[int(i)] for i in alive], n_nodes, single=True)
    assert (np.diff(want[0]) >= 3).all()
    # and the removed ones: their windows are masked, they have no hits
    dead = np.setdiff1d(np.arange(n_nodes), alive)
    assert search(eng, 1, ids, offs, tail, [[int(i)] for i in dead], n_nodes, single=True)[0][-1] == 0
    SEEN.add("every live node after a filter")


# ------------------------------------------------------------------ the two-call protocol
class Raw:
    """amg_match_patterns through the C ABI, the two calls apart"""

    def __init__(self, eng, which, pats):
        self.eng, self.which, self.n = eng, which, len(pats)
        self.offs = np.zeros(self.n + 1, np.int64)
        np.cumsum([len(p) for p in pats], out=self.offs[1:])
        self.flat = np.array([x for p in pats for x in p], np.int32)
        self.total = 0

    def call(self, second, n_pat=None):
        from amira_amd import _ffi
        n = self.n if n_pat is None else n_pat
        hit_off = np.full(self.n + 1, -1, np.int64)
        hr, hp = np.full(self.total + 1, -1, np.int32), np.full(self.total + 1, -1, np.int32)
        rc = _ffi.lib.amg_match_patterns(self.eng._h, self.which, _ffi.ptr(self.flat), _ffi.ptr(self.offs), n,
                                         _ffi.ptr(hit_off), _ffi.ptr(hr) if second else None,
                                         _ffi.ptr(hp) if second else None)
        if rc == 0 and not second:
            self.total = int(hit_off[-1])
        return rc, hit_off, hr[:-1], hp[:-1]


def with_positions(eng, toks, offs, two_v):
    eng.set_reads(toks, offs, two_v)
    at = np.concatenate([np.arange(n) for n in np.diff(offs)]) * 1000
    eng.set_positions(at, at + 899, np.diff(offs) * 1000 + 100)


def test_two_call_protocol():
    from amira_amd import Engine, tokenize
    vocab, toks, offs, _ = tokenize({f"r{i:05d}": g for i, g in enumerate(base_reads(31))})
    pats = [toks[5:8].tolist(), toks[200:201].tolist(), [], toks[150:152].tolist()]
    eng, other = Engine(0), Engine(0)
    try:
        eng.set_reads(toks, offs, vocab.two_v)
        raw = Raw(eng, 0, pats)
        raw.total = 64
        assert raw.call(True)[0] == E_STATE                     # no first call
        rc, off1, _, _ = raw.call(False)
        assert rc == 0 and raw.total > 0
        want = match_reference(toks, offs, 0, pats, vocab.two_v)
        a, b = raw.call(True), raw.call(True)                   # the cached result, twice
        for x in (a, b):
            assert x[0] == 0 and np.array_equal(x[1], want[0]) and np.array_equal(x[2], want[1]) and np.array_equal(x[3], want[2])
        assert raw.call(True, n_pat=raw.n - 1)[0] == E_STATE    # another n_pat
        assert raw.call(True)[0] == 0                           # (which does not spoil the cache)

        def primed(which=0, build=False, positions=False):
            if positions:
                with_positions(eng, toks, offs, vocab.two_v)
            else:
                eng.set_reads(toks, offs, vocab.two_v)
            if build:
                eng.build(K)
            p = pats if which == 0 else [[0], [1, 2], [3]]
            r = Raw(eng, which, p)
            assert r.call(False)[0] == 0 and r.call(True)[0] == 0
            return r

        r = primed()
        eng.set_reads(toks, offs, vocab.two_v)
        assert r.call(True)[0] == E_STATE
        r = primed()
        eng.build(K)
        assert r.call(True)[0] == E_STATE
        for which in (0, 1):   # removals clear the cache whichever array was searched
            r = primed(which, build=True)
            eng.remove_nodes([0])
            assert r.call(True)[0] == E_STATE
            # amg_remove_edges -> live_lists_after_edge_deaths clears it as well, although no node id changes
            r = primed(which, build=True)
            eng.remove_edges([0])
            assert r.call(True)[0] == E_STATE
            r = primed(which, build=True)
            eng.filter(3, 1)
            assert r.call(True)[0] == E_STATE
        # an empty removal list returns before anything is touched: the cache stays
        r = primed(1, build=True)
        eng.remove_nodes([])
        eng.remove_edges([])
        assert r.call(True)[0] == 0
        # adopt_corrected on the context itself, set_reads_from_corrected on another one
        with_positions(eng, toks, offs, vocab.two_v)
        eng.build(K)
        eng.filter(3, 1)
        r = Raw(eng, 0, pats)
        assert r.call(False)[0] == 0
        eng.correct_reads()
        other.set_reads(toks, offs, vocab.two_v)
        ro = Raw(other, 0, pats)
        assert ro.call(False)[0] == 0 and ro.call(True)[0] == 0
        other.set_reads_from_corrected(eng)
        assert ro.call(True)[0] == E_STATE
        eng.adopt_corrected()
        assert r.call(True)[0] == E_STATE
    finally:
        eng.close()
        other.close()


# ------------------------------------------------------------------ the position field of the packed hits
def test_a_row_of_2_to_the_20(eng):
    rng = np.random.default_rng(20)
    n, two_v = 1 << POS_BITS, 1000
    seq = rng.integers(0, 100, n).astype(np.int32)
    seq[n - 1] = 500
    offs = np.array([0, n], np.int64)
    eng.set_reads(seq, offs, two_v)
    pats = [[500], seq[n - 2:].tolist(), seq[n - 40:].tolist(), [7], [7, 8], seq[:3].tolist()]
    want = search(eng, 0, seq, offs, 0, pats, two_v)
    assert hits_of(want, 0)[1].tolist() == [n - 1] and hits_of(want, 1)[1].tolist() == [n - 2]
    assert hits_of(want, 3)[1].size > 5000
    SEEN.add("hit at the last position of 2^20")
    # the same symbols as two rows: no position is anywhere near the limit, the read field is used
    offs2 = np.array([0, 8, n], np.int64)
    eng.set_reads(seq, offs2, two_v)
    search(eng, 0, seq, offs2, 0, pats, two_v)


@pytest.mark.parametrize("where", ["host", "device"])
def test_a_longer_row_is_refused(eng, where):
    """a position of 2^20 or more has no place in a packed hit ((pattern << 48) | (read << 20) | position): the call
    refuses the read set — before this check it returned AMG_OK, with the hit of the last position filed under read 1
    of a set of one read"""
    from amira_amd import _ffi
    n, two_v = (1 << POS_BITS) + 8, 1000
    seq = np.random.default_rng(21).integers(0, 100, n).astype(np.int32)
    seq[n - 1] = 500
    rows = [(np.array([0, n], np.int64), [[500], [7]]), (np.array([0, 3, 3, n, n], np.int64), [[500]]),
            (np.array([0, 3, 5, n], np.int64), [[9999]])]           # the long row anywhere, hits or none
    keep = []
    for offs, pats in rows:
        if where == "host":
            eng.set_reads(seq, offs, two_v)
        else:
            import torch
            keep = [torch.from_numpy(seq).cuda(), torch.from_numpy(offs).cuda()]
            torch.cuda.synchronize()
            eng.set_reads_device(keep[0].data_ptr(), keep[1].data_ptr(), len(offs) - 1, two_v, borrow=True)
        raw = Raw(eng, 0, pats)
        rc = raw.call(False)[0]
        assert rc == E_ARG, (rc, offs)
        assert str(1 << POS_BITS) in _ffi.lib.amg_last_error().decode()
        raw.total = 4
        assert raw.call(True)[0] == E_STATE                          # and hands out no hits afterwards
    # one symbol fewer in that row: served
    offs = np.array([0, 7, 8, n], np.int64)
    eng.set_reads(seq, offs, two_v)
    want = search(eng, 0, seq, offs, 0, [[500], [7]], two_v)
    assert hits_of(want, 0)[1].tolist() == [(1 << POS_BITS) - 1]
    del keep


# ------------------------------------------------------------------ the host wrapper's chunks of 60 000 patterns
def test_match_gene_lists_in_two_chunks():
    from amira_amd import GeneMerGraph
    reads, _, _ = P.synth_inputs(3, 30, 30, 60, 0.05)
    g = GeneMerGraph(reads, 3)
    try:
        vocab, toks, offs = g._vocab, np.asarray(g._tokens_val), np.asarray(g._read_off)
        rng = np.random.default_rng(4)
        usable = [vocab.decode(p) for p in windows_of(rng, toks, offs, 0, 60001, 3)]
        unusable = {0: ["+no_such_gene"], 1: [], 59999: [], 60000: ["-no_such_gene", usable[0][0]], 60001: [usable[0][0], "+no_such_gene"]}
        lists, it = [], iter(usable)
        for i in range(60001 + len(unusable) + 2):
            lists.append(unusable[i] if i in unusable else next(it, None))
        lists[-2:] = [[], ["+no_such_gene"]]
        usable = [x for i, x in enumerate(lists[:-2]) if i not in unusable]
        assert len(usable) == 60001 and None not in lists      # the last usable list is alone in the second call
        SEEN.add("two chunks of the host wrapper")
        got = g._match_gene_lists(lists)
        assert len(got) == len(lists)
        memo = {}
        for i, (genes, (hr, hp)) in enumerate(zip(lists, got)):
            if i in unusable or i >= len(lists) - 2:
                assert hr.size == 0 and hp.size == 0, i
                continue
            key = tuple(genes)
            if key not in memo:
                w = match_reference(toks, offs, 0, [[vocab.token(x) for x in genes]], vocab.two_v)
                memo[key] = (w[1], w[2])
                assert w[1].size >= 1
            assert np.array_equal(hr, memo[key][0]) and np.array_equal(hp, memo[key][1]), (i, genes)
    finally:
        g.close()


def test_every_regime_was_seen():
    assert SEEN == REGIMES, (sorted(REGIMES - SEEN), sorted(SEEN - REGIMES))
