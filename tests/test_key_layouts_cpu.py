"""What tests/test_gpu_key_layouts.py relies on, from the sequential C oracle alone: every read set of tests/key_layouts.py
builds at every k in 2 .. 16 and holds, at each, repeated and single nodes, short and long reads, the vocabulary's edge
tokens, and — from k = 11 — a token with bit 15 (bit 16 on the 32-bit vocabulary) set at a tuple position that a packed
node record keeps in its words 6 and 7."""
import numpy as np
import pytest

import key_layouts as KL


@pytest.mark.parametrize("k", KL.KS)
@pytest.mark.parametrize("name", list(KL.VOCABS))
def test_read_set_exercises_the_layout(name, k):
    toks, offs, two_v = KL.read_set(name)
    pinned = KL.VOCABS[name][1]
    flip = two_v - 1
    assert toks.min() >= 0 and toks.max() < two_v
    g = KL.oracle(name, k)          # (raises on a palindromic gene-mer)
    cov = g["coverage"]
    assert int((cov >= 3).sum()) >= 100 and int((cov == 1).sum()) >= 100
    n_reads = len(offs) - 1
    assert 0 < g["n_short"] < n_reads
    assert g["n_short"] == int((np.diff(offs) < k).sum())
    for t in pinned:
        assert np.isin(g["tokens"], (t, flip - t)).any(), t
    if k >= 11:
        far = g["tokens"][:, 10:]
        assert (far >= (65536 if name == "wide" else 32768 if name == "edge16" else 300)).any()
    for world in (2, 3):
        b = KL.shard_bounds(n_reads, world)
        assert all(offs[b[r + 1]] > offs[b[r]] for r in range(world))


def test_read_sets_have_the_sketched_shape():
    for name in KL.VOCABS:
        toks, offs, two_v = KL.read_set(name)
        n = np.diff(offs)
        assert len(n) == KL.N_READS and 9000 < len(toks) < 11500
        assert n.min() >= 1 and n.max() <= 45
        assert np.all(n[np.arange(len(n)) % 9 != 8] >= 20)
        # no token next to its own complement inside a read
        inner = ~np.isin(np.arange(1, len(toks)), offs)
        assert not np.any((toks[:-1] + toks[1:] == two_v - 1) & inner)


def test_layout_rule_switches_where_the_widths_say():
    """key_layouts.layout against the figures worked out by hand: 16 bits per token up to k = 5, then 10 / 16 / 17 bits;
    94 key bits"""
    first_fp = {"small": 10, "edge16": 6, "wide": 6}
    for name, (two_v, _, _) in KL.VOCABS.items():
        for k in KL.KS:
            single = KL.layout(k, two_v, False, False)
            assert single["exact_keys"] == (1 if k < first_fp[name] else 2), (name, k)
            assert KL.layout(k, two_v, True, False)["exact_keys"] == 0
            merged = KL.layout(k, two_v, False, True)
            assert merged["exact_keys"] == (1 if k < first_fp[name] else 0), (name, k)
            assert (merged["held"] == "32-bit tokens") == (name == "wide")
            if merged["exact_keys"] == 0:
                assert (merged["slots"] == "fp, packed") == (name != "wide" and k <= 14)
    assert KL.layout(3, 600, False, True)["slots"] == "exact, one word"
    assert KL.layout(4, 600, False, True)["slots"] == "exact, two words"
    assert KL.layout(6, 600, False, True)["slots"] == "exact, one word"      # 60 bits at 10 bits per gene
    assert KL.layout(7, 600, False, True)["slots"] == "exact, two words"
    assert KL.layout(5, 65538, False, True)["slots"] == "exact, two words"   # 85 bits at 17 bits per gene
