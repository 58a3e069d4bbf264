"""A plain numpy reference of the batched sub-list search (amg_match_patterns, amg_match.hip): all occurrences of
every pattern in every row of a CSR array, in the shape Engine.match_patterns returns them.

A row is seq[offs[r] : offs[r + 1] - tail] (tail: the last k - 1 places of a read hold no window for node ids); a
match lies inside one row.  A pattern that is empty, or whose first symbol is outside [0, domain), has no hits — the
library buckets patterns by their first symbol over the symbol domain.  Hits are ordered by pattern, then row, then
position, which is the order of the flat index.

match_reference       any patterns: the places of the first symbol, narrowed by comparing the array shifted by
                      1, 2, ... against the pattern's further symbols, masked by the rows' ends
match_reference_single  one-symbol patterns by the ten thousand: one stable argsort of the searched symbols, grouped
match_naive           the list comprehension of the older tests, for small cases (test_match_oracle_cpu.py pins the two
                      forms above to it)"""
import numpy as np


def _rows(seq, offs, tail):
    """per flat index: its row, and the flat index at which the searched part of that row ends"""
    seq = np.ascontiguousarray(seq, np.int64)
    offs = np.ascontiguousarray(offs, np.int64)
    lens = np.diff(offs)
    row = np.repeat(np.arange(len(lens), dtype=np.int64), lens)
    end = (offs[1:] - tail)[row]
    return seq, offs, row, end


def _pack(per_pattern, offs, row):
    counts = np.array([len(x) for x in per_pattern], np.int64)
    hit_off = np.zeros(len(per_pattern) + 1, np.int64)
    np.cumsum(counts, out=hit_off[1:])
    flat = np.concatenate(per_pattern) if per_pattern and hit_off[-1] else np.zeros(0, np.int64)
    hit_read = row[flat]
    return hit_off, hit_read.astype(np.int32), (flat - offs[hit_read]).astype(np.int32)


def match_reference(seq, offs, tail, patterns, domain=None):
    """(offsets[n_pat + 1], hit_read, hit_pos); domain None: every non-negative first symbol is usable"""
    seq, offs, row, end = _rows(seq, offs, tail)
    n = len(seq)
    at = np.arange(n, dtype=np.int64)
    per = []
    for p in patterns:
        m = len(p)
        if m == 0 or p[0] < 0 or (domain is not None and p[0] >= domain) or m > n:
            per.append(np.zeros(0, np.int64))
            continue
        idx = np.flatnonzero((seq == p[0]) & (at + m <= end))
        for j in range(1, m):
            if idx.size == 0:
                break
            idx = idx[seq[idx + j] == p[j]]
        per.append(idx)
    return _pack(per, offs, row)


def match_reference_single(seq, offs, tail, symbols, domain=None):
    """the same for the patterns [s] for s in symbols"""
    seq, offs, row, end = _rows(seq, offs, tail)
    sym = np.ascontiguousarray(symbols, np.int64).reshape(-1)
    valid = np.flatnonzero(np.arange(len(seq), dtype=np.int64) < end)
    order = valid[np.argsort(seq[valid], kind="stable")]   # places by symbol, ascending within a symbol
    sorted_sym = seq[order]
    lo = np.searchsorted(sorted_sym, sym, "left")
    hi = np.searchsorted(sorted_sym, sym, "right")
    usable = sym >= 0 if domain is None else (sym >= 0) & (sym < domain)
    cnt = np.where(usable, hi - lo, 0)
    hit_off = np.zeros(len(sym) + 1, np.int64)
    np.cumsum(cnt, out=hit_off[1:])
    total = int(hit_off[-1])
    flat = order[np.repeat(lo, cnt) + np.arange(total, dtype=np.int64) - np.repeat(hit_off[:-1], cnt)]
    hit_read = row[flat]
    return hit_off, hit_read.astype(np.int32), (flat - offs[hit_read]).astype(np.int32)


def match_naive(seq, offs, tail, patterns, domain=None):
    rows = [list(map(int, seq[offs[r]:max(offs[r + 1] - tail, offs[r])])) for r in range(len(offs) - 1)]
    hit_off, hr, hp = [0], [], []
    for p in patterns:
        p = list(map(int, p))
        if p and p[0] >= 0 and (domain is None or p[0] < domain):
            hits = [(r, i) for r, row in enumerate(rows) for i in range(len(row) - len(p) + 1) if row[i:i + len(p)] == p]
            hr += [h[0] for h in hits]
            hp += [h[1] for h in hits]
        hit_off.append(len(hr))
    return np.array(hit_off, np.int64), np.array(hr, np.int32), np.array(hp, np.int32)


def same(a, b):
    return all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b) == 3
