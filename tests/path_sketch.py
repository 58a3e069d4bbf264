"""Constructed read sets for amg_path_sketch_overlaps (amira_amd/csrc/amg_sketch.hip: k_bs_mark, k_bs_fill, k_bs_segs,
k_bs_hash, k_bs_unique, k_bs_pstart, k_bs_common) and the numbers the reference gives on each, for
tests/test_path_sketch_cpu.py (the cases against the reference alone) and tests/test_gpu_path_sketch.py.

`expected` restates construct_graph.py:2148-2194 and :1747-1786 (as oracle/amira_oracle/bubbles.py has them) on arrays and
hashes with the oracle's MinHash class.  A case is a `Case`: reads as tokens, gene positions, sequences, paths as lists of
node ids, pairs of paths — and `claims`, the properties the case was built to have, which the CPU test holds against the
reference alone.  The sketch call returns counts, not hashes: small WITNESS paths, whose overlap with the path under
test must be their own size, pin which hashes are in a sketch.

A read of exactly k genes has one window, hence one node and one segment: `Case.one(seq, a, e)` makes such a read of
genes nobody else has whose segment is the Python slice seq[a : e + 1].

Node ids: the engine numbers gene-mers in the order the reads first show them (tests/derive_cases.py build_orders,
tests/test_gpu_build.py); `host_tok_node` restates that so that cases can be built and judged without a device.  The GPU
test checks it against Engine.read_node_ids() and hands the engine's own array to `expected`."""
import functools

import numpy as np

from amira_oracle.minhash import MinHash

SEAMS = (1024, 2048, 3072)   # multiples of BS_CHUNK: k_bs_hash takes a segment through LDS 1024 start positions at a time
_RC = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def revcomp(s):
    return s.encode().translate(_RC)[::-1].decode()


def bases(rng, n):
    return np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(n))].tobytes().decode()


# ------------------------------------------------------------------ the reference
@functools.lru_cache(maxsize=None)
def sketch(seg, ksize, scaled):
    """the hashes sourmash keeps of one segment (computed once per distinct text: the tests share them)"""
    mh = MinHash(n=0, ksize=ksize, scaled=scaled)
    mh.add_sequence(seg, force=True)
    return frozenset(mh.hashes)


def segments(read_off, gs, ge, k, tok_node, sequences, row_to_seq, listed=None):
    """(node, text) of every window that sits on a node (of `listed`, when given), in window order"""
    out = []
    for r in range(len(read_off) - 1):
        row = r if row_to_seq is None else int(row_to_seq[r])
        for w in range(int(read_off[r]), int(read_off[r + 1]) - k + 1):
            n = int(tok_node[w])
            if n < 0 or (listed is not None and n not in listed):
                continue
            out.append((n, sequences[row][int(gs[w]):int(ge[w + k - 1]) + 1]))
    return out


def path_sketches(read_off, gs, ge, k, tok_node, sequences, row_to_seq, ksize, scaled, paths):
    node_set = {}
    for n, seg in segments(read_off, gs, ge, k, tok_node, sequences, row_to_seq, {int(x) for p in paths for x in p}):
        node_set.setdefault(n, set()).update(sketch(seg, ksize, scaled))
    return [set().union(*[node_set.get(int(n), set()) for n in p]) for p in paths]


def expected(read_tokens, read_off, gs, ge, k, tok_node, sequences, row_to_seq, ksize, scaled, paths, pairs):
    """(sizes, common) as np.int64 arrays: len(sketch) per path, len(sketch[a] & sketch[b]) per pair"""
    assert len(read_tokens) == int(read_off[-1]) == len(gs) == len(ge) == len(tok_node)
    sk = path_sketches(read_off, gs, ge, k, tok_node, sequences, row_to_seq, ksize, scaled, paths)
    return (np.array([len(s) for s in sk], np.int64).reshape(-1),
            np.array([len(sk[a] & sk[b]) for a, b in pairs], np.int64).reshape(-1))


def kept_windows(seg, ksize, scaled):
    """k-mer windows of a segment that pass the cut, every occurrence counted"""
    return sum(len(sketch(seg[i:i + ksize], ksize, scaled)) for i in range(len(seg) - ksize + 1))


def pair_count(case, tok_node):
    """the (path, hash) pairs the call makes before it sorts them: hashes of a segment x paths listing its node"""
    listings = {}
    for p in case.paths:
        for n in p:
            listings[int(n)] = listings.get(int(n), 0) + 1
    return sum(kept_windows(seg, case.ksize, case.scaled) * listings[n]
               for n, seg in segments(case.off, case.gs, case.ge, case.k, tok_node, case.sequences, case.row_to_seq, set(listings)))


def sorted_pairs(case, tok_node):
    """the paths of the (path, hash) pairs in the order the two sorts leave them in, every occurrence kept"""
    per_path = [[] for _ in case.paths]
    segs = {}
    for n, seg in segments(case.off, case.gs, case.ge, case.k, tok_node, case.sequences, case.row_to_seq):
        segs.setdefault(n, []).append(seg)
    for p, nodes in enumerate(case.paths):
        for n in nodes:
            for seg in segs.get(int(n), []):
                for i in range(len(seg) - case.ksize + 1):
                    per_path[p].extend(sketch(seg[i:i + case.ksize], case.ksize, case.scaled))
    return [(p, h) for p, hs in enumerate(per_path) for h in sorted(hs)]


# ------------------------------------------------------------------ node ids without a device
def host_tok_node(tokens, off, k, two_v):
    """node id per window (-1 on the last k - 1 genes of a read): gene-mers numbered as the reads first show them, a
    gene-mer and its reverse complement (the reversed list of flipped tokens) one node"""
    ids, out = {}, np.full(len(tokens), -1, np.int32)
    for r in range(len(off) - 1):
        for w in range(int(off[r]), int(off[r + 1]) - k + 1):
            t = tuple(int(x) for x in tokens[w:w + k])
            rc = tuple(two_v - 1 - x for x in reversed(t))
            assert t != rc, "palindromic gene-mer"
            out[w] = ids.setdefault(min(t, rc), len(ids))
    return out


def host_filter(tok_node, min_node_cov):
    """filter_graph(min_node_cov, 1): the windows of nodes seen fewer times become -2"""
    live = tok_node[tok_node >= 0]
    cov = np.bincount(live, minlength=int(live.max()) + 1 if len(live) else 0)
    out = tok_node.copy()
    out[(tok_node >= 0) & (cov[np.maximum(tok_node, 0)] < min_node_cov)] = -2
    return out


# ------------------------------------------------------------------ a case
class Case:
    def __init__(self, name, k, ksize, scaled, seed):
        self.name, self.k, self.ksize, self.scaled = name, int(k), int(ksize), int(scaled)
        self.rng = np.random.default_rng(seed)
        self._genes, self._n_genes = [], 0
        self.off, self.gs, self.ge, self.sequences = [0], [], [], []
        self.row_to_seq = None
        self.filter = None        # min_node_cov of a filter(min_node_cov, 1) between the build and the call
        self._wpaths = []         # paths as lists of window indices until finish()
        self.pairs = []
        # what the case was built to show, judged by the reference alone in the CPU test:
        #   ("common_is_size", q, p)   common[q] == sizes[p] > 0
        #   ("size", p, n)             sizes[p] == n
        #   ("seam", p, c)             path p is one segment with a k-mer starting at every offset in (c - ksize, c]
        #   ("text", p, text)          path p is one segment and the slice of it is exactly `text`
        #   ("smaller", p, q)          sizes[p] < sizes[q]
        self.claims = []

    # -- reads
    def fresh(self, n):
        self._n_genes += n
        return [(g, 1) for g in range(self._n_genes - n, self._n_genes)]

    def read(self, seq, genes, spans):
        """a read of (gene, strand) pairs at (start, end) spans on `seq`; returns the index of its first window"""
        assert len(genes) == len(spans)
        w0 = self.off[-1]
        self._genes.extend(genes)
        self.gs.extend(int(s) for s, _ in spans)
        self.ge.extend(int(e) for _, e in spans)
        self.off.append(w0 + len(genes))
        self.sequences.append(seq)
        return w0

    def one(self, seq, a, e, genes=None):
        """a read of k genes: one window whose segment is seq[a : e + 1]"""
        return self.read(seq, genes or self.fresh(self.k), [(a, e)] * self.k)

    def whole(self, text, genes=None):
        """a read whose one segment is all of `text`"""
        return self.one(text, 0, len(text) - 1, genes)

    # -- paths and pairs
    def path(self, windows):
        self._wpaths.append(list(windows))
        return len(self._wpaths) - 1

    def pair(self, a, b):
        self.pairs.append((a, b))
        return len(self.pairs) - 1

    def witness(self, p, text):
        """a path of one segment `text` whose hashes must all be among path p's"""
        w = self.path([self.whole(text)])
        self.claims.append(("common_is_size", self.pair(w, p), w))
        self.pair(p, w)
        return w

    def finish(self, shuffle_rows=False, extra_rows=0, unsequenced=()):
        V = max(self._n_genes, 1)
        self.two_v = 2 * V
        self.tokens = np.array([V + g if s > 0 else V - 1 - g for g, s in self._genes], np.int32)
        self.off = np.array(self.off, np.int64)
        self.gs, self.ge = np.array(self.gs, np.int64), np.array(self.ge, np.int64)
        built = host_tok_node(self.tokens, self.off, self.k, self.two_v)
        self.n_nodes = int(built.max()) + 1 if len(built) else 0
        self.tok_node = built if self.filter is None else host_filter(built, self.filter)
        self.paths = [[int(built[w]) for w in p] for p in self._wpaths]
        if shuffle_rows or extra_rows or unsequenced:
            n = len(self.sequences)
            rows = [r for r in range(n) if r not in set(unsequenced)]
            seqs = [self.sequences[r] for r in rows] + [bases(self.rng, 50 + 7 * i) for i in range(extra_rows)]
            order = self.rng.permutation(len(seqs)) if shuffle_rows else np.arange(len(seqs))
            self.row_to_seq = np.full(n, -1, np.int32)
            place = {int(src): dst for dst, src in enumerate(order)}
            for i, r in enumerate(rows):
                self.row_to_seq[r] = place[i]
            self.sequences = [seqs[int(src)] for src in order]
        return self

    # -- what the call takes
    def path_arrays(self, paths=None):
        paths = self.paths if paths is None else paths
        path_off = np.zeros(len(paths) + 1, np.int64)
        np.cumsum([len(p) for p in paths], out=path_off[1:])
        return path_off, np.array([n for p in paths for n in p], np.int32)

    def expected(self, tok_node=None):
        return expected(self.tokens, self.off, self.gs, self.ge, self.k, self.tok_node if tok_node is None else tok_node,
                        self.sequences, self.row_to_seq, self.ksize, self.scaled, self.paths, self.pairs)


# ------------------------------------------------------------------ a. seams of k_bs_hash's chunks
def seam_lengths(ksize):
    raw = [ksize - 1, ksize, ksize + 1, 1023, 1024, 1025, 1024 + ksize - 2, 1024 + ksize - 1, 1024 + ksize, 2047, 2048,
           2049, 2048 + ksize - 1, 3077]
    return list(dict.fromkeys(raw))


def seams(k, ksize, scaled, lengths=None):
    c = Case("seams k=%d ksize=%d scaled=%d" % (k, ksize, scaled), k, ksize, scaled, 1000 * k + 10 * ksize + scaled)
    for L in lengths or seam_lengths(ksize):
        for _ in range(200):   # (scaled > 1: a segment whose witnesses all keep a hash; the first one at scaled 1)
            S = bases(c.rng, L)
            cuts = [(s, S[max(s - (ksize - 1) - 3, 0):s + (ksize - 1) + 3]) for s in SEAMS if L > s]
            if all(len(w) < ksize or sketch(w, ksize, scaled) for _, w in cuts):
                break
        else:
            raise AssertionError("no segment with non-empty witnesses")
        a = int(c.rng.integers(0, 70))   # (the segment starts anywhere in its read)
        p = c.path([c.one(bases(c.rng, a) + S + bases(c.rng, 9), a, a + L - 1)])
        c.claims.append(("text", p, S))
        for s, w in cuts:
            if L >= s + ksize:
                c.claims.append(("seam", p, s))
            if len(w) >= ksize:
                c.witness(p, w)
    return c.finish()


SEAM_CASES = [(3, ks, 1, None) for ks in (1, 8, 9, 16, 17, 24, 25, 32)] + \
             [(k, 11, scaled, (1024 + 11, 2048 + 11 - 1)) for k in (3, 5) for scaled in (1, 2, 3, 10)]


# ------------------------------------------------------------------ b. the Python slice
def slices(ksize=4):
    c = Case("slices", 3, ksize, 1, 21)
    n = 200
    S = bases(c.rng, n)
    far = 1 << 40
    for what, a, e, text in [("b == len", 50, n - 1, S[50:]), ("b == len + 1", 50, n, S[50:]),
                             ("b far beyond len", 50, n + 10 ** 6, S[50:]), ("a == len - ksize", n - ksize, n + 3, S[-ksize:]),
                             ("a == len - 1", n - 1, n + 5, S[-1:]), ("a == len", n, n + 50, ""), ("a > len", n + 7, n + 50, ""),
                             ("shorter than ksize", 10, 10 + ksize - 2, S[10:10 + ksize - 1]), ("a == b", 30, 29, ""),
                             ("a > b", 60, 20, ""), ("a = 2^40", far, far + 100, ""), ("b = 2^40", 120, far, S[120:]),
                             ("a == 0, b == len", 0, n - 1, S)]:
        p = c.path([c.one(S, a, e)])
        c.claims.append(("text", p, text))
        w = c.path([c.whole(text)])
        c.pair(p, w)
        c.claims.append(("size", p, len(sketch(text, ksize, 1))))
        if len(text) >= ksize:
            c.claims.append(("common_is_size", c.pair(w, p), p))
    return c.finish()


# ------------------------------------------------------------------ c. what a base may be
def letters():
    ksize = 11
    c = Case("letters", 3, ksize, 1, 31)
    U = bases(c.rng, 1500)
    up = c.path([c.whole(U)])
    for twin in (U.lower(), revcomp(U), revcomp(U).lower(), "".join(x.lower() if i % 3 else x for i, x in enumerate(U))):
        p = c.path([c.whole(twin)])
        c.claims.append(("common_is_size", c.pair(p, up), up))
        c.claims.append(("common_is_size", c.pair(up, p), p))
    clean = bases(c.rng, 2100)
    cp = c.path([c.whole(clean)])
    wit = c.witness(cp, clean[1023 - (ksize - 1) - 3:1024 + (ksize - 1) + 3])
    for at, ch in [((1023,), "N"), ((1024,), "n"), ((1023, 1024), "RY"), ((0, 5, 1013, 1034, 2047, 2048, 2099), "NU-*xyN")]:
        t = list(clean)
        for i, x in zip(at, ch):
            t[i] = x
        p = c.path([c.whole("".join(t))])
        c.claims.append(("common_is_size", c.pair(p, cp), p))   # nothing but hashes of the clean text ...
        c.claims.append(("smaller", p, cp))                      # ... and not all of them
        c.pair(p, wit)
        c.pair(wit, p)
    homo_a, homo_t, two = (c.path([c.whole(x)]) for x in ("A" * 2500, "t" * 2500, "AC" * 1250))
    c.claims += [("size", homo_a, 1), ("size", homo_t, 1), ("size", two, 2)]
    c.claims.append(("common_is_size", c.pair(homo_a, homo_t), homo_a))
    c.pair(two, homo_a)
    c.claims.append(("size", c.path([c.whole("N" * 1100 + "ACGTTGCAAGT" + "N" * 1100)]), 1))
    return c.finish()


# ------------------------------------------------------------------ d. which path lists which node
LISTED_BY = (1, 2, 63, 64, 65, 130)


def membership():
    c = Case("membership", 3, 11, 1, 41)
    shared = c.whole(bases(c.rng, 40))
    empty_first = c.path([])
    first_of = []
    for n in LISTED_BY:
        x = c.whole(bases(c.rng, 290))
        first_of.append(len(c._wpaths))
        for j in range(n):
            c.path([x, shared] if j == n - 1 and n > 1 else [x])
        if n == 64:
            empty_mid = c.path([])
    x = c.whole(bases(c.rng, 300))
    once, twice, thrice = c.path([x]), c.path([x, x]), c.path([x, shared, x])
    empty_last = c.path([])
    c.claims.append(("common_is_size", c.pair(once, twice), twice))
    c.claims.append(("common_is_size", c.pair(twice, once), once))
    c.claims.append(("common_is_size", c.pair(once, thrice), once))
    c.claims.append(("common_is_size", c.pair(once, once), once))
    c.claims.append(("common_is_size", c.pair(twice, twice), once))
    for e in (empty_first, empty_mid, empty_last):
        c.claims.append(("size", e, 0))
        c.pair(once, e)
        c.pair(e, once)
        c.pair(e, e)
    c.pair(empty_first, empty_last)
    for f, n in zip(first_of, LISTED_BY):
        c.claims.append(("common_is_size", c.pair(f, f + n - 1), f))   # the first and the last path listing the node
        c.pair(f + n - 1, f)
        c.pair(f, once)
    return c.finish()


def membership_filtered():
    """filter_graph(2, 1) between the build and the call: nodes B and D lose their only window"""
    c = Case("membership after a filter", 3, 11, 1, 43)
    c.filter = 2
    ga, gb, gc = c.fresh(3), c.fresh(3), c.fresh(4)
    A = [c.whole(bases(c.rng, 120), ga) for _ in range(3)][0]
    B = c.whole(bases(c.rng, 130), gb)
    S = bases(c.rng, 400)
    C = c.read(S, gc, [(0, 99), (100, 199), (200, 299), (300, 399)])
    D = C + 1
    for _ in range(2):
        c.read(bases(c.rng, 300), gc[:3], [(0, 99), (100, 199), (200, 299)])
    pa, pb, pbd, pab, pcd, pd, pc = (c.path(x) for x in ([A], [B], [B, D], [A, B], [C, D], [D], [C]))
    c.claims += [("size", pb, 0), ("size", pbd, 0), ("size", pd, 0)]
    c.claims.append(("common_is_size", c.pair(pa, pab), pa))
    c.claims.append(("common_is_size", c.pair(pcd, pc), pc))
    c.pair(pb, pa)
    c.pair(pbd, pd)
    return c.finish()


# ------------------------------------------------------------------ e. windows that share bases, reads that share nodes
def sharing():
    c = Case("sharing", 3, 11, 1, 51)
    spans = lambda n, at=0: [(at + 100 * i, at + 100 * i + 79) for i in range(n)]   # noqa: E731
    # a tandem read a b c a b c: node (a b c) twice on one read
    a, b, cc = c.fresh(3)
    T = bases(c.rng, 620)
    t0 = c.read(T, [a, b, cc, a, b, cc], spans(6, 11))
    tandem = c.path([t0])
    c.witness(tandem, T[11:11 + 280])
    c.witness(tandem, T[311:311 + 280])
    c.path([t0, t0 + 1, t0 + 2])
    # the same genes on the other strand with the reverse complement of the bases
    g = c.fresh(5)
    F = bases(c.rng, 500)
    f0 = c.read(F, g, spans(5))
    r0 = c.read(revcomp(F), [(x, -s) for x, s in reversed(g)], [(500 - 1 - e, 500 - 1 - s) for s, e in reversed(spans(5))])
    both = c.path([f0, f0 + 1, f0 + 2])
    alone = c.path([c.whole(F[0:280]), c.whole(F[100:380]), c.whole(F[200:480])])
    c.claims.append(("common_is_size", c.pair(both, alone), both))
    c.claims.append(("common_is_size", c.pair(alone, both), alone))
    c.reverse_first_window = r0
    # one node on 40 reads, its segment at 40 different offsets modulo 64
    g = c.fresh(3)
    core = bases(c.rng, 150)
    for i in range(40):
        at = 64 * int(c.rng.integers(0, 5)) + i
        seg = bases(c.rng, 60 + i) + core + bases(c.rng, 90)
        w = c.one(bases(c.rng, at) + seg + bases(c.rng, 13), at, at + len(seg) - 1, g)
    many = c.path([w])
    c.witness(many, core)
    c.pair(many, tandem)
    # reads no path lists: they have no sequence at all
    none = [len(c.sequences), len(c.sequences) + 1]
    c.whole(bases(c.rng, 90))
    c.whole(bases(c.rng, 90))
    return c.finish(shuffle_rows=True, extra_rows=3, unsequenced=none)


# ------------------------------------------------------------------ f. waves of k_bs_unique
def runs():
    ksize = 11
    c = Case("runs", 3, ksize, 1, 61)
    big_text = [bases(c.rng, 3010)]
    big_text.append(big_text[0][1500:] + bases(c.rng, 1500))
    big_text += [bases(c.rng, 3010), bases(c.rng, 2990)]
    c.big, c.small, texts = [], [], []
    for i in range(400):
        if i % 100 == 50:
            c.big.append(c.path([c.whole(big_text[len(c.big)])]))
        text = bases(c.rng, ksize + i % 5)
        if i in (201, 211):       # twins: the same bases as the path before, on a node of their own
            text = texts[-1]
        if i == 210:
            text = bases(c.rng, ksize)
        texts.append(text)
        w = c.whole(text)
        c.small.append(c.path([w] * 6))   # (listed six times: six equal pairs per hash)
        c.claims.append(("size", c.small[-1], i % 5 + 1 if i not in (201, 211) else len(texts[-1]) - ksize + 1))
    for x, y in zip(c.small[:-1], c.small[1:]):
        c.pair(x, y)
    for i in (201, 211):
        c.claims.append(("common_is_size", c.pair(c.small[i], c.small[i - 1]), c.small[i]))
    c.pair(c.big[0], c.big[1])
    for x in c.big:
        c.pair(x, x)
        c.pair(x, c.small[0])
        c.pair(c.small[-1], x)
    c.pair(c.big[1], c.big[0])
    c.pair(c.big[2], c.big[3])
    return c.finish()


def wave_kinds(paths_in_order):
    """of the aligned runs of 64 sorted pairs (one wave of k_bs_unique each): how many lie inside one path, how many span
    three or more"""
    inside = spanning = 0
    for i in range(0, len(paths_in_order), 64):
        n = len(set(paths_in_order[i:i + 64]))
        inside += n == 1
        spanning += n >= 3
    return inside, spanning


CLASSES = {"slices": slices, "letters": letters, "membership": membership, "membership_filtered": membership_filtered,
           "sharing": sharing, "runs": runs}


def case_id(name):
    return name if isinstance(name, str) else "k%d-ksize%d-scaled%d" % name[:3]


@functools.lru_cache(maxsize=None)
def case(name):
    """a case by class name or by its SEAM_CASES tuple, built once"""
    return CLASSES[name]() if isinstance(name, str) else seams(*name)
