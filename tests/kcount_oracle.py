"""Host oracle of the device k-mer counts (amg_kcount.hip): canonical k-mers of nucleotide sequences in numpy, and the
same in ten lines of plain Python for the numpy version to be held against (tests/test_depth_cpu.py).

Definition (jellyfish count -m k -C, restated): every window of k bases of every sequence, either case; a window with
a character outside ACGT is skipped; no window spans two sequences; a k-mer and its reverse complement are one key.
Codes here are A 0, C 1, G 2, T 3 (complement 3 - code), the key is the smaller of the two packed strands — not the
device's packing: which strand stands for a pair is observable through neither."""
from collections import Counter

import numpy as np

_CODE = np.full(256, 4, np.uint8)
for _i, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _CODE[ord(_c.lower())] = _i

HISTO_LAST = 10001


def window_keys(seq, k):
    """(keys uint64[max(len - k + 1, 0)], valid bool[...]): the canonical key of the window at every start"""
    raw = np.frombuffer(seq.encode() if isinstance(seq, str) else bytes(seq), dtype=np.uint8)
    n = len(raw) - k + 1
    if n <= 0:
        return np.zeros(0, np.uint64), np.zeros(0, bool)
    code = _CODE[raw]
    bad = np.concatenate(([0], np.cumsum(code == 4)))
    valid = (bad[k:] - bad[:-k]) == 0
    c = (code & 3).astype(np.uint64)
    fwd = np.zeros(n, np.uint64)
    rev = np.zeros(n, np.uint64)
    for j in range(k):   # the rolling pack: k shifts over all windows at once
        fwd = (fwd << np.uint64(2)) | c[j: j + n]
        rev |= (np.uint64(3) - c[j: j + n]) << np.uint64(2 * j)
    return np.minimum(fwd, rev), valid


class Table:
    """the counts of every canonical k-mer of `seqs`"""

    def __init__(self, seqs, k):
        self.k = k
        parts = [key[valid] for key, valid in (window_keys(s, k) for s in seqs)]
        allk = np.concatenate(parts) if parts else np.zeros(0, np.uint64)
        self.keys, self.counts = np.unique(allk, return_counts=True)
        self.counts = self.counts.astype(np.int64)
        self.windows, self.distinct = int(len(allk)), int(len(self.keys))

    def lookup(self, seq, min_count=0):
        """int64 per BASE of seq: the count of the k-mer that starts there (0: absent or below min_count), -1: no
        valid window starts there"""
        key, valid = window_keys(seq, self.k)
        out = np.full(len(seq), -1, np.int64)
        if len(key) == 0 or len(self.keys) == 0:
            out[: len(key)][valid] = 0
            return out
        at = np.minimum(np.searchsorted(self.keys, key), len(self.keys) - 1)
        cnt = np.where(self.keys[at] == key, self.counts[at], 0)
        cnt = np.where(cnt >= max(min_count, 1), cnt, 0)
        out[: len(key)] = np.where(valid, cnt, -1)
        return out

    def histo(self, min_count=0):
        """{times counted: distinct keys}, everything beyond 10 000 in bin 10 001 (jellyfish histo)"""
        kept = self.counts[self.counts >= max(min_count, 1)]
        v, n = np.unique(np.minimum(kept, HISTO_LAST), return_counts=True)
        return {int(a): int(b) for a, b in zip(v, n)}

    def set_counts(self, seqs, min_count=0):
        """the sorted counts >= max(min_count, 1) of every valid window of seqs, one per occurrence"""
        got = [self.lookup(s, min_count) for s in seqs]
        allc = np.concatenate(got) if got else np.zeros(0, np.int64)
        return np.sort(allc[allc > 0])


def counter_counts(seqs, k):
    """the same counts, slowly: {canonical k-mer as text: occurrences}"""
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    out = Counter()
    for s in seqs:
        s = s.upper()
        for i in range(len(s) - k + 1):
            w = s[i: i + k]
            if set(w) <= set("ACGT"):
                out[min(w, "".join(comp[c] for c in reversed(w)))] += 1
    return out


def counter_lookup(counter, seq, k):
    """Table.lookup with counter_counts' result"""
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    s = seq.upper()
    out = [-1] * len(s)
    for i in range(len(s) - k + 1):
        w = s[i: i + k]
        if set(w) <= set("ACGT"):
            out[i] = counter[min(w, "".join(comp[c] for c in reversed(w)))]
    return np.array(out, np.int64)


def random_sequences(rng, n, lo, hi):
    """tests/test_gpu_minhash.py's alphabet and weights"""
    alphabet = np.frombuffer(b"ACGTacgtNRY", dtype=np.uint8)
    probs = np.array([0.23, 0.23, 0.23, 0.23, 0.015, 0.015, 0.015, 0.015, 0.01, 0.005, 0.005])
    return [bytes(rng.choice(alphabet, size=int(rng.integers(lo, hi)), p=probs / probs.sum())).decode()
            for _ in range(n)]


def revcomp(seq):
    return seq.translate(str.maketrans("ACGTacgt", "TGCAtgca"))[::-1]


def synthetic_reads(seed=11, genome=6000, n_reads=240, length=1000, err=0.04):
    """reads of a random circular genome with substitutions, half of them reverse-complemented:
    {read id: {"sequence": ...}} (the end-to-end case of the copy-number tests)"""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 4, genome)
    reads = {}
    for i in range(n_reads):
        start = int(rng.integers(0, genome))
        r = g[(start + np.arange(length)) % genome].copy()
        hit = rng.random(length) < err
        r[hit] = (r[hit] + rng.integers(1, 4, int(hit.sum()))) % 4
        s = "".join("ACGT"[x] for x in r)
        reads[f"read_{i}"] = {"sequence": revcomp(s) if i % 2 else s}
    return reads
