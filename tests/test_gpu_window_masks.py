"""The live-window masks that a removal's read walk leaves (k_mask_reads, amg_filter.hip) and the correction's
classification takes (k_corr_classify, amg_correct.hip) instead of loading a flagged read's windows again — in every
order of calls in which the masks are current, absent, or older than the reads, against the sequential C oracle
(token_oracle.Sweep) after every stage.

Reads over one genome of 150 of 300 gene names, each gene once, so that a window of correct genes is a node every read
over that place shares and a window with a wrong gene is a node of coverage 1 that filter(3, 1) removes.  Window counts:
0 (a read shorter than k), 1, 63, 64 — the last read whose mask holds every window — and 65, which the wave walks as
before; 17 to 40 otherwise.  Kinds of read: clean; wrong genes inside (None runs between live windows: re-threaded);
wrong genes at the two ends only (dead windows at the ends: a slice); random genes throughout (every window dead:
dropped); and four side branches of two nodes, four reads each, which outlive the filter and fall to tip clipping."""
import numpy as np
import pytest

import token_oracle
from helpers import compare_corrected, compare_engine_to_sweep, live_arrays

pytestmark = pytest.mark.gpu

V, GENOME = 300, 150
KINDS = ("clean", "inside", "ends", "random")


def window_counts(k):
    return [0, 1, 63, 64, 65, 17, 26, 40, 33, 64, 63, 65, 21]


def make_reads(seed, k, n_reads=360):
    """(tokens, read_offsets, two_v, gene_start, gene_end, read_len), kinds[n_reads], windows[n_reads]"""
    rng = np.random.default_rng(seed)
    genes = rng.permutation(V)[:GENOME]
    genome = np.where(rng.random(GENOME) < 0.5, V + genes, V - 1 - genes)
    wc = window_counts(k)
    toks, offs, kinds, wins = [], [0], [], []
    for r in range(n_reads):
        n = wc[r % len(wc)]
        L = n + k - 1 if n > 0 else int(rng.integers(1, k))      # (n = 0: one to k - 1 genes)
        kind = KINDS[(r // len(wc)) % 4] if n >= 1 else "clean"
        s0 = int(rng.integers(0, GENOME - L + 1))
        read = genome[s0:s0 + L].copy()
        wrong = lambda m: rng.integers(0, 2 * V, m)
        if kind == "inside" and L > 2 * k + 2:
            at = rng.permutation(np.arange(k, L - k))[:max(1, L // 25)]
            read[at] = wrong(len(at))
        elif kind == "ends":
            read[0] = wrong(1)[0]
            read[-1] = wrong(1)[0]
        elif kind == "random":
            read = wrong(L)
        if rng.random() < 0.5:
            read = (2 * V - 1 - read)[::-1]
        toks.append(read)
        offs.append(offs[-1] + L)
        kinds.append(kind)
        wins.append(n)
    for tip in range(4):    # side branches of two nodes that survive the filter (four reads each) and fall to tip clipping
        s0 = int(rng.integers(0, GENOME - 20))
        read = np.concatenate([genome[s0:s0 + 18 + tip], rng.integers(0, 2 * V, 2)])
        for copy in range(4):
            toks.append(read if copy % 2 else (2 * V - 1 - read)[::-1])
            offs.append(offs[-1] + len(read))
            kinds.append("tip")
            wins.append(len(read) - k + 1)
    tokens = np.concatenate(toks).astype(np.int32)
    offs = np.asarray(offs, np.int64)
    within = np.arange(len(tokens)) - np.repeat(offs[:-1], np.diff(offs))
    gs = 100 + 1000 * within.astype(np.int64)
    ge = gs + 900
    rl = 1000 * np.diff(offs) + 300
    return (tokens, offs, 2 * V, gs, ge, rl), np.asarray(kinds), np.asarray(wins)


@pytest.fixture(scope="module")
def eng():
    from amira_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def begin(eng, data, k):
    tokens, offs, two_v, gs, ge, rl = data
    eng.set_reads(tokens, offs, two_v)
    eng.set_positions(gs, ge, rl)
    orc = token_oracle.Sweep(tokens, offs, two_v, gs, ge, rl)
    eng.build(k)
    orc.build(k)
    compare_engine_to_sweep(eng, orc, "build")
    return orc


def filter_both(eng, orc, what="filter"):
    eng.filter(3, 1)
    orc.filter(3, 1)
    compare_engine_to_sweep(eng, orc, what)


def clip_both(eng, orc, k, what="clip"):
    got = eng.remove_short_linear_paths(k)
    want = orc.remove_short_linear_paths(k)
    assert sorted(got.tolist()) == sorted(want.tolist()), what
    compare_engine_to_sweep(eng, orc, what)
    return len(want)


def adopt_and_build(eng, orc, k, what):
    eng.adopt_corrected()
    orc.adopt_corrected()
    eng.build(k)
    orc.build(k)
    compare_engine_to_sweep(eng, orc, what)


@pytest.mark.parametrize("k", [3, 5])
def test_the_read_set_has_every_kind_of_read(k):
    """what the other tests rely on, asked of the oracle alone: after filter(3, 1) there are flagged reads of 1, 63, 64
    and 65 windows, reads with no live window, reads whose dead windows are at the ends only, and reads with a None run
    between live windows"""
    data, kinds, wins = make_reads(41 + k, k)
    orc = token_oracle.Sweep(*data)
    orc.build(k)
    orc.filter(3, 1)
    tn, _ = orc.read_nodes()
    fix = orc.reads_to_correct() != 0
    offs = data[1]
    seen = {"all_dead": set(), "ends": set(), "gap": set()}
    for r in np.flatnonzero(fix):
        n = int(wins[r])
        w = tn[offs[r]:offs[r] + n] >= 0
        if not w.any():
            seen["all_dead"].add(n)
            continue
        first, last = int(np.argmax(w)), n - 1 - int(np.argmax(w[::-1]))
        seen["gap" if not w[first:last + 1].all() else "ends"].add(n)
    assert (wins == 0).any() and not fix[wins == 0].any()
    assert 1 in seen["all_dead"]
    assert {63, 64, 65} <= seen["all_dead"] and {63, 64, 65} <= seen["ends"] and {63, 64, 65} <= seen["gap"]
    assert (~fix & (wins > 0)).any()


@pytest.mark.parametrize("k", [3, 5])
def test_masks_current(eng, k):
    """build -> filter -> correct_reads: the classification takes every flagged read of at most 64 windows from the masks"""
    data, _, _ = make_reads(41 + k, k)
    orc = begin(eng, data, k)
    filter_both(eng, orc)
    compare_corrected(eng, orc, True, "correct")
    compare_corrected(eng, orc, True, "correct again, same graph, same masks")


@pytest.mark.parametrize("k", [3, 5])
def test_two_walks_before_one_classify(eng, k):
    """build -> filter -> remove_short_linear_paths -> correct_reads: the second walk rewrites the mask of every read,
    also of a read that the first removal flagged and the second left alone"""
    data, _, _ = make_reads(41 + k, k)
    orc = begin(eng, data, k)
    filter_both(eng, orc)
    fix1 = eng.reads_to_correct() != 0
    tn1, _ = eng.read_nodes()
    assert clip_both(eng, orc, k) > 0
    tn2, _ = eng.read_nodes()
    offs = data[1]
    changed = np.add.reduceat((tn1 != tn2).astype(np.int64), offs[:-1]) > 0
    assert changed.any() and (fix1 & ~changed).any()
    compare_corrected(eng, orc, True, "correct")


@pytest.mark.parametrize("k", [3, 5])
def test_flags_without_masks(eng, k):
    """build_filtered -> correct_reads: the filtered build flags its dead reads itself, no walk has made masks — the
    classification loads the windows (node ids number the survivors only: the live graphs are compared)"""
    data, _, _ = make_reads(41 + k, k)
    tokens, offs, two_v, gs, ge, rl = data
    # (masks of the same reads from a plain filter first: they must not be taken for those of the filtered build)
    orc = begin(eng, data, k)
    filter_both(eng, orc)
    eng.build_filtered(k, 3, 1)
    a, b = live_arrays(eng, with_adj=False), live_arrays(orc, with_adj=False)
    for key in a:
        assert np.array_equal(a[key], b[key]), key
    compare_corrected(eng, orc, True, "correct")


@pytest.mark.parametrize("no_derive", [False, True])
@pytest.mark.parametrize("k", [3, 5])
def test_the_sweep_in_its_own_order(eng, monkeypatch, k, no_derive):
    """build -> filter -> correct -> adopt -> build -> clip -> correct -> adopt -> build: every correction after a walk,
    every build (the derived one, or with AMG_NO_DERIVE=1 the one from the reads) voids the masks"""
    if no_derive:
        monkeypatch.setenv("AMG_NO_DERIVE", "1")
    data, _, _ = make_reads(41 + k, k)
    orc = begin(eng, data, k)
    filter_both(eng, orc)
    compare_corrected(eng, orc, True, "correct 1")
    adopt_and_build(eng, orc, k, "build 2")
    clip_both(eng, orc, k)
    compare_corrected(eng, orc, True, "correct 2")
    adopt_and_build(eng, orc, k, "build 3")
    if no_derive:
        assert eng.counts()["derived"] == 0
    # and on: the third graph is one to work on like any other
    filter_both(eng, orc, "filter 3")
    compare_corrected(eng, orc, True, "correct 3")


@pytest.mark.parametrize("fresh", [True, False])
def test_stale_mask_words_of_a_larger_read_set(eng, fresh):
    """a read set of 360 reads is masked, then one of 90 reads runs on buffers that still hold the larger set's words
    (the same engine, or a second engine that takes the first one's buffers over): with flags and no masks, and with
    masks of its own"""
    from amira_amd import Engine
    k = 5
    big, _, _ = make_reads(46, k)
    small, _, _ = make_reads(47, k, n_reads=90)
    first = Engine(0) if fresh else eng
    try:
        orc = begin(first, big, k)
        filter_both(first, orc)
        compare_corrected(first, orc, True, "large set")
    finally:
        if fresh:
            first.close()
    second = Engine(0) if fresh else eng
    try:
        tokens, offs, two_v, gs, ge, rl = small
        second.set_reads(tokens, offs, two_v)
        second.set_positions(gs, ge, rl)
        orc = token_oracle.Sweep(*small)
        orc.build(k)
        orc.filter(3, 1)
        second.build_filtered(k, 3, 1)
        compare_corrected(second, orc, True, "small set, flags of the filtered build")
        orc = begin(second, small, k)
        filter_both(second, orc)
        compare_corrected(second, orc, True, "small set, masks of its own")
    finally:
        if fresh:
            second.close()
