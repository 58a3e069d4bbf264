"""GPU: a node's canonical tuple, first-seen position and direction (k_x_assign_nodes_ranked,
amg_build_x_claims.hip: the tuple is the window at the first-seen position of the node, read from the reads) against the
sequential C oracle, for every key scheme of the exact-key build, and through build_filtered.

The read sets are substrings of a random genome with a few substitutions, either strand, 3 ... 70 genes long, a few
thousand of them so that the token array spans many 1 024-token tiles, plus an empty read, reads of one and two genes
(shorter than every k here), and a LAST read of random genes: the only occurrence of its last window's node is the last
k tokens of the token array (first-seen position + k == number of tokens)."""
import functools

import numpy as np
import pytest

import token_oracle

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def read_set(V, seed, n_reads=3000):
    """(tokens, read offsets, 2V).  No two neighbouring tokens are each other's complement, so no window of any size is
    its own reverse complement (the build refuses those, as the reference does)."""
    rng = np.random.default_rng(seed)
    flip = 2 * V - 1

    def no_hairpin(t):
        for i in range(1, len(t)):
            while t[i] == flip - t[i - 1]:
                t[i] = rng.integers(0, 2 * V)
        return t

    genome = no_hairpin(rng.integers(0, 2 * V, 1500))
    reads = []
    for _ in range(n_reads):
        n = int(rng.integers(3, 71))
        a = int(rng.integers(0, len(genome) - n))
        r = genome[a:a + n].copy()
        err = rng.random(n) < 0.03
        r[err] = rng.integers(0, 2 * V, int(err.sum()))
        r = no_hairpin(r)
        reads.append(r if rng.random() < 0.5 else flip - r[::-1])
    for j in range(12):  # reads shorter than k for every k of this file, and an empty one
        reads.insert(int(rng.integers(0, len(reads))), rng.integers(0, 2 * V, j % 3))
    reads.append(no_hairpin(rng.integers(0, 2 * V, 12)))  # the last read: genes of its own
    toks = np.concatenate(reads).astype(np.int32)
    offs = np.zeros(len(reads) + 1, np.int64)
    np.cumsum([len(r) for r in reads], out=offs[1:])
    return toks, offs, 2 * V


@functools.lru_cache(maxsize=None)
def oracle(V, seed, k, filt=None):
    """the oracle's nodes (with the first-seen position of each: the first window of its id), once per read set and k"""
    toks, offs, two_v = read_set(V, seed)
    o = token_oracle.Sweep(toks, offs, two_v)
    try:
        o.build(k)
        tn, _ = o.read_nodes()
        pos = np.flatnonzero(tn >= 0)
        ids, at = np.unique(tn[pos], return_index=True)
        assert np.array_equal(ids, np.arange(o.counts()["n_nodes"]))
        first_token = pos[at].astype(np.int64)
        if filt:
            o.filter(*filt)
        n = o.nodes()
        n["first_token"] = first_token
        return n
    finally:
        o.close()


def check_conditions(V, seed, k):
    """what the read set must contain for the case to test anything (asserted on the oracle alone)"""
    toks, offs, _ = read_set(V, seed)
    want = oracle(V, seed, k)
    T = len(toks)
    lens = np.diff(offs)
    assert T > 50 * 1024 and (lens < k).sum() >= 8                     # many tiles; reads shorter than k
    last = np.flatnonzero(want["first_token"] + k == T)                  # the last window of the last read ...
    assert len(last) == 1 and want["coverage"][last[0]] == 1 and lens[-1] >= k   # ... is its node's only occurrence
    assert (want["first_dir"] == -1).sum() > 100 and (want["first_dir"] == 1).sum() > 100  # nodes first seen reversed
    assert (want["coverage"] >= 3).sum() > 100                           # something survives filter(3, 1)


def run(V, seed, k, expect_keys):
    from amira_amd import Engine
    toks, offs, two_v = read_set(V, seed)
    check_conditions(V, seed, k)
    eng = Engine(0)   # (made here: the switches of a case are read from the environment)
    try:
        eng.set_reads(toks, offs, two_v)
        eng.build(k)
        assert eng.counts()["exact_keys"] == expect_keys
        got, want = eng.nodes(), oracle(V, seed, k)
        for key in ("first_token", "first_dir", "tokens", "coverage"):
            assert np.array_equal(got[key], want[key]), ("build", key)
        # the same through the fused build + filter: only the survivors exist, in the same order
        eng.build_filtered(k, 3, 1)
        got, want = eng.nodes(), oracle(V, seed, k, (3, 1))
        g_live, w_live = got["alive"] != 0, want["alive"] != 0
        assert 0 < w_live.sum() < len(w_live)
        for key in ("first_token", "first_dir", "tokens", "coverage"):
            assert np.array_equal(got[key][g_live], want[key][w_live]), ("build_filtered", key)
    finally:
        eng.close()


# one- and two-word 16-bit keys (k = 3, 5), k = 7 (tight bits: 7 x 10), the run-time-k kernel (k = 4, 6), k = 9 at 10 bits
@pytest.mark.parametrize("V,k", [(40, 3), (300, 3), (40, 5), (300, 5), (300, 7), (120, 4), (300, 6), (300, 9)])
def test_exact_key_schemes(V, k):
    run(V, 7, k, 1)


def test_fingerprint_keys_control():
    """k = 9 over 600 gene names: 9 x 11 bits do not fit the slot, the key is a fingerprint and the tuple has always come
    from the reads (300 names and fewer give 10 bits a gene, 90 in all: an exact key, the case above)"""
    run(600, 7, 9, 2)


@pytest.mark.parametrize("env", [{"AMG_X_TIGHT_BITS": "1"}, {"AMG_NODE_BUCKETS": "0"},
                                 {"AMG_CLAIM_SHARDS": "1", "AMG_X_HEAD_TILES": "2"}],
                         ids=lambda e: "+".join(e))
def test_switches(env, monkeypatch):
    """tight bits, hashed slots only, claim ids with holes behind a head launch"""
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    run(300, 7, 5, 1)
