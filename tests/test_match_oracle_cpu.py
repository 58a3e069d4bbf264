"""The numpy reference of the sub-list search (match_oracle.py) against the naive list comprehension of
test_match_patterns_against_brute_force, on a few hundred small random cases — empty rows, rows shorter than the tail,
duplicated and self-overlapping patterns, unusable first symbols — and its two forms against each other on
one-symbol pattern sets.  No GPU."""
import numpy as np
import pytest

from match_oracle import match_naive, match_reference, match_reference_single, same


def random_case(rng):
    n_rows = int(rng.integers(0, 9))
    vocab = int(rng.choice([1, 2, 3, 8]))
    tail = int(rng.choice([0, 0, 1, 2, 4]))
    lens = rng.integers(0, 14, n_rows)
    lens[rng.random(n_rows) < 0.2] = 0                       # empty rows
    short = rng.random(n_rows) < 0.2
    lens[short] = rng.integers(0, tail + 1, int(short.sum()))   # rows no longer than the tail
    offs = np.zeros(n_rows + 1, np.int64)
    np.cumsum(lens, out=offs[1:])
    seq = rng.integers(0, vocab, int(offs[-1])).astype(np.int32)
    if rng.random() < 0.3 and seq.size:
        seq[rng.random(seq.size) < 0.1] = -1                 # places without a symbol, as in the node ids of short reads
    domain = None if rng.random() < 0.5 else vocab
    pats = []
    for _ in range(int(rng.integers(0, 12))):
        kind = rng.random()
        if kind < 0.5 and seq.size:                          # a slice of the array: may cross rows, may lie in a tail
            s = int(rng.integers(0, seq.size))
            pats.append(seq[s:s + int(rng.integers(1, 7))].tolist())
        elif kind < 0.7:                                     # self-overlapping
            a = int(rng.integers(0, vocab))
            pats.append([a] * int(rng.integers(1, 5)))
        elif kind < 0.8:
            pats.append([])
        elif kind < 0.9:                                     # first symbol outside the domain
            pats.append([int(rng.choice([-1, vocab, vocab + 5]))] + rng.integers(0, vocab, 2).tolist())
        else:
            pats.append(rng.integers(0, vocab, int(rng.integers(1, 5))).tolist())
    if pats and rng.random() < 0.5:                          # duplicated patterns
        pats += [list(pats[0]), list(pats[-1]), list(pats[0])]
    return seq, offs, tail, pats, domain


@pytest.mark.parametrize("block", range(8))
def test_reference_equals_the_naive_search(block):
    rng = np.random.default_rng(1000 + block)
    hits = 0
    for _ in range(50):
        seq, offs, tail, pats, domain = random_case(rng)
        want = match_naive(seq, offs, tail, pats, domain)
        got = match_reference(seq, offs, tail, pats, domain)
        assert same(got, want), (seq, offs, tail, pats, domain, got, want)
        hits += int(want[0][-1])
        # the one-symbol form on the one-symbol patterns of the case and on every symbol around the vocabulary
        syms = [p[0] for p in pats if len(p) == 1] + list(range(-2, 10))
        single = match_reference_single(seq, offs, tail, syms, domain)
        assert same(single, match_naive(seq, offs, tail, [[s] for s in syms], domain))
        assert same(single, match_reference(seq, offs, tail, [[s] for s in syms], domain))
    assert hits > 100


def test_known_answers():
    seq = np.array([5, 5, 5, 5, 7, 5, 5, 1, 2], np.int32)
    offs = np.array([0, 4, 4, 7, 9], np.int64)
    off, hr, hp = match_reference(seq, offs, 0, [[5, 5], [5, 5, 5, 5], [5, 7], [7, 5, 5], [5, 5], [], [9], [1, 2, 3]])
    assert off.tolist() == [0, 4, 5, 5, 6, 10, 10, 10, 10]
    assert list(zip(hr.tolist(), hp.tolist())) == [(0, 0), (0, 1), (0, 2), (2, 1), (0, 0), (2, 0),
                                                  (0, 0), (0, 1), (0, 2), (2, 1)]
    # the last `tail` places of a row are not searched, and a row shorter than the tail has none
    off, hr, hp = match_reference(seq, offs, 2, [[5], [5, 5], [7], [1]])
    assert off.tolist() == [0, 2, 3, 4, 4]
    assert list(zip(hr.tolist(), hp.tolist())) == [(0, 0), (0, 1), (0, 0), (2, 0)]
    # the domain
    assert match_reference(seq, offs, 0, [[7], [5]], domain=7)[0].tolist() == [0, 0, 4 + 2]
    assert match_reference_single(seq, offs, 0, [7, 5, -1], domain=7)[0].tolist() == [0, 0, 6, 6]


def test_one_symbol_sets_of_ten_thousands():
    rng = np.random.default_rng(5)
    lens = rng.integers(0, 9, 60)
    offs = np.zeros(61, np.int64)
    np.cumsum(lens, out=offs[1:])
    seq = rng.integers(0, 50, int(offs[-1])).astype(np.int32)
    syms = rng.integers(-1, 52, 65535)
    a = match_reference_single(seq, offs, 2, syms, 50)
    b = match_reference(seq, offs, 2, [[int(s)] for s in syms], 50)
    assert same(a, b) and a[0][-1] > 50000
