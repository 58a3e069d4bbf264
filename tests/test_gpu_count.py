"""GPU: the coverage counting sweeps (amg_count.hip: count_ids / k_count_ids) against numpy's bincount, one count per
call through amg_count_probe, in every regime the sweeps have: one to four id ranges of HOT ids and what lies beyond
them, the early finish once an eighth of the array is left, the first sweep that finishes from the previous count's
hint, the number of sweeps a build learnt, the listed ids of the first sweep and a list segment that runs over, the
marked-claim and the gathered form, the 16-byte and the scalar loads, the block clamp.  Everything is integer equality.
Every case that is meant for a regime asserts it from the state record the probe returns, and the last test of the
module asserts that the cases before it met every regime at least once (it needs the whole module to have run)."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HOT = 39936          # ids a sweep keeps in LDS (HOT_IDS)
MAX_SWEEPS = 4       # COUNT_MAX_SWEEPS
SEG = 256            # ids per list segment of a workgroup (COUNT_LIST_SEG)
MAX_BLOCKS = 256     # COUNT_MAX_BLOCKS
MADE, LAST = 0x40000000, 0x80000000   # AMG_MADE_FLAG, AMG_LAST_FLAG
NODES, EDGES = 0, 1
PLAIN, MARKED, GATHER = 0, 1, 2
FORGET, LEARN = 1, 2
KINDS = [NODES, EDGES]
N_IDS = [1, HOT - 1, HOT, HOT + 1, 2 * HOT, 2 * HOT + 1, 4 * HOT, 4 * HOT + 1, 10 * HOT]
DISTS = ["low", "uniform", "high", "boundary", "none"]

SEEN = set()  # regimes met by the cases of this module (test_every_regime_was_seen)
REGIMES = {"first sweep finished by hint", "later sweep finished by the eighth", "list walk", "list overrun",
           "finish at sweep index 3", "launches cut by learning", "block clamp"}


@pytest.fixture(scope="module")
def eng():
    from amira_amd import Engine
    e = Engine(0)
    yield e
    e.close()


class State:
    def __init__(self, w):
        self.words = w.copy()
        self.beyond = [int(x) for x in w[0:4]]
        self.done = [int(x) for x in w[4:8]]
        self.list_over, self.listed = int(w[8]), int(w[9])
        self.sweeps, self.blocks, self.learnt, self.guards = int(w[10]), int(w[11]), int(w[12]), int(w[13])

    @property
    def finisher(self):
        return self.done.index(1) if 1 in self.done else None

    @property
    def walked(self):  # the second launch walked the first sweep's segments (it does whenever they hold everything)
        return self.sweeps > 1 and self.listed == 1 and self.list_over == 0 and self.beyond[0] > 0

    def __repr__(self):
        return (f"State(beyond={self.beyond}, done={self.done}, list_over={self.list_over}, listed={self.listed}, "
                f"sweeps={self.sweeps}, blocks={self.blocks}, learnt={self.learnt})")


def probe(eng, kind, form, ids, n_ids, tab=None, mis=0, flags=FORGET):
    from amira_amd import _ffi
    ids = np.ascontiguousarray(ids, np.int32).copy()
    counts = np.zeros(n_ids + 1, np.uint32)
    state = np.zeros(16, np.int64)
    tab = None if tab is None else np.ascontiguousarray(tab, np.int32)
    _ffi.check(_ffi.lib.amg_count_probe(eng._h, kind, form, _ffi.ptr(ids) if ids.size else None, ids.size, n_ids,
                                        _ffi.ptr(tab) if tab is not None and tab.size else None,
                                        0 if tab is None else tab.size, mis, flags, _ffi.ptr(counts), _ffi.ptr(state)))
    return counts, ids, State(state)


def check(eng, kind, form, ids, n_ids, tab=None, mis=0, flags=FORGET):
    """one count; counts, the array afterwards and the guard words against numpy, then what holds of the state record
    in every regime; notes the regimes it met"""
    ids = np.ascontiguousarray(ids, np.int32)
    n = ids.size
    got, after, st = probe(eng, kind, form, ids, n_ids, tab, mis, flags)
    if form == PLAIN:
        counted = ids[ids >= 0].astype(np.int64)
        want = np.bincount(counted, minlength=n_ids)
        want_after, rest = ids, 0
    elif form == MARKED:
        raw = ids.view(np.uint32)
        present = ids != -1
        made = present & ((raw & np.uint32(MADE)) != 0)
        counted = (raw & np.uint32(~(MADE | LAST) & 0xffffffff))[present & ~made].astype(np.int64)
        want = 1 + np.bincount(counted, minlength=n_ids)
        want_after, rest = ids, 1
    else:
        want_after = np.where(ids >= 0, tab[np.maximum(ids, 0)], -1).astype(np.int32)
        counted = want_after[want_after >= 0].astype(np.int64)
        want = np.bincount(counted, minlength=n_ids)
        rest = 0
    what = (kind, form, n, n_ids, mis, flags, st)
    assert st.guards == 1, what
    bad = np.flatnonzero(got[:n_ids].astype(np.int64) != want[:n_ids])
    assert bad.size == 0, (what, bad[:8], got[bad[:8]], want[bad[:8]])
    assert got[n_ids] == rest, what
    assert np.array_equal(after, want_after), what
    # the launches
    ranges = min(-(-n_ids // HOT), MAX_SWEEPS)
    if n == 0:
        assert st.sweeps == 0 and st.blocks == 0, what
        return st
    assert 1 <= st.sweeps <= ranges, what
    want_blocks = -(-n // (2 * HOT))
    assert st.blocks == min(max(want_blocks, 1), MAX_BLOCKS), what
    # at most one sweep finishes, and a count that nobody finished had nothing left
    assert sum(st.done) <= 1 and all(d in (0, 1) for d in st.done) and not any(st.done[st.sweeps:]), what
    if st.finisher is None:
        assert st.sweeps > 1 and 0 in st.beyond[:st.sweeps - 1], what
    # what a sweep that went over the array found beyond its range
    for r in range(st.sweeps):
        ran = r == 0 or (not any(st.done[:r]) and st.beyond[r - 1] != 0 and not (r == 1 and st.walked))
        assert st.beyond[r] == (int((counted >= (r + 1) * HOT).sum()) if ran else 0), (what, r)
    if st.sweeps == 1:
        assert st.done[0] == 1 and st.listed == 0, what
    f = st.finisher
    if f == 0 and st.sweeps > 1:
        SEEN.add("first sweep finished by hint")
    if st.walked:
        assert f == 1 and st.beyond[1] == 0, what
        SEEN.add("list walk")
    if st.list_over:
        assert st.listed == 1, what
        SEEN.add("list overrun")
    if f is not None and 0 < f < st.sweeps - 1 and not st.walked:
        assert st.beyond[f - 1] * 8 <= n, what
        SEEN.add("later sweep finished by the eighth")
    if f == 3:
        SEEN.add("finish at sweep index 3")
    if st.sweeps < ranges:
        SEEN.add("launches cut by learning")
    if want_blocks > MAX_BLOCKS:
        SEEN.add("block clamp")
    return st


# ------------------------------------------------------------------ generators
def gen_ids(rng, dist, n, n_ids, scale=HOT / 4, none=0.03):
    if dist == "none" or n == 0:
        return np.full(n, -1, np.int32)
    if dist == "uniform":
        ids = rng.integers(0, n_ids, n)
    elif dist in ("low", "high"):
        ids = np.minimum(rng.geometric(1.0 / max(scale, 1.0), n) - 1, n_ids - 1)
        if dist == "high":
            ids = n_ids - 1 - ids
    else:  # the ids either side of every range boundary, and the last one
        edge = [r * HOT + d for r in range(1, MAX_SWEEPS + 1) for d in (-1, 0)] + [n_ids - 1]
        edge = np.array(sorted({e for e in edge if 0 <= e < n_ids}))
        ids = edge[rng.integers(0, edge.size, n)]
    ids = ids.astype(np.int32)
    if none:
        ids[rng.random(n) < none] = -1
    return ids


def mark(rng, ids):
    """plain ids -> claims as a table pass leaves them: exactly one occurrence of every id present carries MADE, about
    half of all occurrences LAST"""
    out = ids.astype(np.int64)
    at = np.flatnonzero(ids >= 0)
    at = at[rng.permutation(at.size)]
    _, first = np.unique(ids[at], return_index=True)
    out[at[first]] |= MADE
    last = (ids >= 0) & (rng.random(ids.size) < 0.5)
    out[last] |= LAST
    return (out & 0xffffffff).astype(np.uint32).view(np.int32)


def slots_for(rng, ids, n_ids):
    """plain ids -> (slots of a table, the table's id per slot): every id has a slot, the table has as many again that
    repeat ids"""
    base = np.concatenate([np.arange(n_ids), rng.integers(0, n_ids, n_ids + 7)]).astype(np.int32)
    perm = rng.permutation(base.size)
    tab = base[perm]
    inv = np.empty(base.size, np.int64)
    inv[perm] = np.arange(base.size)
    slots = np.where(ids >= 0, inv[np.maximum(ids, 0)], -1).astype(np.int32)
    return slots, tab


def in_form(rng, form, ids, n_ids):
    if form == MARKED:
        return mark(rng, ids), None
    if form == GATHER:
        return slots_for(rng, ids, n_ids)
    return ids, None


def with_beyond(rng, n, m, first=HOT, span=HOT, far=0):
    """n ids of the first range, m of them replaced by ids of [first, first + span), `far` of those by ids of the range
    after that; shuffled"""
    ids = rng.integers(0, HOT, n).astype(np.int32)
    ids[:m] = rng.integers(first, first + span, m)
    ids[:far] = rng.integers(first + span, first + 2 * span, far)
    return ids[rng.permutation(n)]


# ------------------------------------------------------------------ single calls, every one from forgotten hints
@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("n_ids", N_IDS)
def test_n_ids_by_distribution(eng, n_ids, dist):
    for kind in KINDS:
        rng = np.random.default_rng(n_ids * 10 + kind)
        n = 300_003
        st = check(eng, kind, PLAIN, gen_ids(rng, dist, n, n_ids), n_ids)
        assert st.sweeps == min(-(-n_ids // HOT), MAX_SWEEPS) and st.blocks == 4
        if n_ids <= HOT:
            assert st.done == [1, 0, 0, 0] and st.beyond == [0, 0, 0, 0]
        elif dist == "none":
            assert st.finisher is None and st.beyond == [0, 0, 0, 0]
        elif n_ids >= 4 * HOT and dist in ("uniform", "high", "boundary"):
            # more than an eighth is left after every range: all four sweeps count, the fourth finishes
            assert st.done == [0, 0, 0, 1] and st.list_over == 1
            assert (st.beyond[3] > 0) == (n_ids > 4 * HOT)
        elif dist == "low" and n_ids > HOT:
            # e^-4 of the ids beyond the first range: too many for the segments, few enough for the second launch
            assert st.list_over == 1 and st.finisher == 1


@pytest.mark.parametrize("dist", ["low", "uniform", "high"])
@pytest.mark.parametrize("n_ids", [HOT + 1, 4 * HOT + 1, 10 * HOT])
def test_four_million_ids(eng, n_ids, dist):
    for kind in KINDS:
        rng = np.random.default_rng(n_ids * 10 + kind + 5)
        st = check(eng, kind, PLAIN, gen_ids(rng, dist, 4_000_001, n_ids), n_ids)
        assert st.blocks == 51
        if n_ids > 4 * HOT and dist != "low":
            assert st.done == [0, 0, 0, 1]


def test_block_clamp(eng):
    n = MAX_BLOCKS * 2 * HOT + 5  # one workgroup more than COUNT_MAX_BLOCKS would be wanted
    rng = np.random.default_rng(21)
    st = check(eng, NODES, PLAIN, gen_ids(rng, "uniform", n, 4 * HOT + 1), 4 * HOT + 1)
    assert st.blocks == MAX_BLOCKS and st.done == [0, 0, 0, 1]
    assert "block clamp" in SEEN


@pytest.mark.parametrize("form", [PLAIN, MARKED])
@pytest.mark.parametrize("which", ["0", "HOT-1", "HOT", "last"])
def test_one_id_n_times(eng, which, form):
    """every thread of every workgroup on one counter, in LDS or in global memory, and a counter of n"""
    n, n_ids = 3_000_000, 5 * HOT + 3
    the_id = {"0": 0, "HOT-1": HOT - 1, "HOT": HOT, "last": n_ids - 1}[which]
    for kind in KINDS:
        rng = np.random.default_rng(kind)
        ids = np.full(n, the_id, np.int32)
        if form == MARKED:
            ids = mark(rng, ids)
        st = check(eng, kind, form, ids, n_ids)
        counted = n - (form == MARKED)
        assert st.beyond[0] == (counted if the_id >= HOT else 0)
        if the_id == n_ids - 1:
            assert st.done == [0, 0, 0, 1] and st.beyond == [counted] * 4
        elif the_id == HOT:
            assert st.beyond[1] == 0


@pytest.mark.parametrize("form", [PLAIN, MARKED, GATHER])
@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 4097])
def test_short_arrays(eng, n, form):
    n_ids = 3 * HOT - 5
    for kind in KINDS:
        rng = np.random.default_rng(n + 100 * kind)
        ids, tab = in_form(rng, form, gen_ids(rng, "uniform", n, n_ids, none=0.1), n_ids)
        st = check(eng, kind, form, ids, n_ids, tab)
        assert st.sweeps == (3 if n else 0) and st.blocks == (1 if n else 0)


@pytest.mark.parametrize("form", [PLAIN, MARKED, GATHER])
@pytest.mark.parametrize("tail", [0, 1, 2, 3])
@pytest.mark.parametrize("mis", [0, 1, 2, 3])
def test_misaligned_base_and_tail(eng, mis, tail, form):
    """the 16-byte loads with the n % 4 ids they leave, and the scalar path of a base that is not 16-byte aligned"""
    n_ids = 2 * HOT + 9
    for kind in KINDS:
        for n in (4096 + tail, 200_000 + tail):
            rng = np.random.default_rng(16 * mis + 4 * tail + kind)
            ids, tab = in_form(rng, form, gen_ids(rng, "uniform", n, n_ids), n_ids)
            st = check(eng, kind, form, ids, n_ids, tab, mis=mis)
            assert st.sweeps == 3


@pytest.mark.parametrize("dist", ["uniform", "low"])
@pytest.mark.parametrize("n_ids", [HOT, 2 * HOT, 5 * HOT + 7])
@pytest.mark.parametrize("form", [PLAIN, MARKED, GATHER])
def test_forms_by_ranges(eng, form, n_ids, dist):
    for kind in KINDS:
        rng = np.random.default_rng(n_ids + kind)
        ids, tab = in_form(rng, form, gen_ids(rng, dist, 300_003, n_ids), n_ids)
        st = check(eng, kind, form, ids, n_ids, tab)
        assert st.sweeps == {HOT: 1, 2 * HOT: 2}.get(n_ids, 4)
        if n_ids > 4 * HOT and dist == "uniform":
            assert st.done == [0, 0, 0, 1]


@pytest.mark.parametrize("lists", ["on", "off"])
@pytest.mark.parametrize("n_ids", [2 * HOT, 3 * HOT])
def test_the_eighth(eng, monkeypatch, n_ids, lists):
    """exactly n / 8 occurrences beyond the first range: the second sweep takes everything that is left; one more: it
    does not.  With two ranges the second sweep is the last one launched and finishes the count either way (the state
    cannot tell the two apart: counts and the finisher are what is asserted), so the decision is read off a count over
    three ranges, where the sweep that finishes is the second or the third."""
    if lists == "off":
        monkeypatch.setenv("AMG_COUNT_LIST_SEG", "0")
    n = 800_000
    far = 5 if n_ids > 2 * HOT else 0   # a few ids of the third range: the third sweep has something left to finish
    for kind in KINDS:
        for m, finisher in ((n // 8, 1), (n // 8 + 1, 2 if far else 1)):
            rng = np.random.default_rng(m + kind)
            st = check(eng, kind, PLAIN, with_beyond(rng, n, m, far=far), n_ids)
            assert st.blocks == 11 and st.sweeps == n_ids // HOT
            assert st.beyond[0] == m and st.list_over == 1 and not st.walked   # 11 segments cannot hold 100 000 ids
            assert st.finisher == finisher, (m, st)
            if far:
                assert st.beyond[1] == far
    assert "later sweep finished by the eighth" in SEEN


@pytest.mark.parametrize("seg", [None, 8])
@pytest.mark.parametrize("n_ids", [2 * HOT, 3 * HOT])
def test_segment_capacity(eng, monkeypatch, n_ids, seg):
    """one workgroup: its segment holds exactly what lies beyond the first range and the second launch walks it; one id
    more and the segment has run over: the second launch sweeps"""
    if seg is not None:
        monkeypatch.setenv("AMG_COUNT_LIST_SEG", str(seg))
    cap = SEG if seg is None else seg
    n = 2 * HOT
    for kind in KINDS:
        for m in (cap, cap + 1):
            rng = np.random.default_rng(m + kind)
            # spread over the second and (three ranges) the third range; more than an eighth of a short array when m is
            # set against n = 300, so that the walk, not the eighth, is what finishes
            ids = with_beyond(rng, n, m, span=n_ids - HOT)
            st = check(eng, kind, PLAIN, ids, n_ids)
            assert st.blocks == 1 and st.listed == 1 and st.beyond[0] == m
            assert st.list_over == (0 if m == cap else 1), (m, st)
            assert st.walked == (m == cap) and st.finisher == 1
            short = with_beyond(rng, 300, min(m, 300), span=n_ids - HOT)
            st = check(eng, kind, PLAIN, short, n_ids)
            assert st.list_over == (0 if m == cap else 1) and st.walked == (m == cap)
    assert {"list walk", "list overrun"} <= SEEN


# ------------------------------------------------------------------ sequences on one context
@pytest.mark.parametrize("learn_all", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_hint_that_no_longer_fits(eng, kind, learn_all):
    """a low-heavy count leaves "finish in the first sweep" and two learnt sweeps; the counts that follow have nearly
    everything beyond the first range, a tenth and ten times the ids"""
    n, n_ids = 400_000, 4 * HOT
    rng = np.random.default_rng(31 + kind)
    st = check(eng, kind, PLAIN, gen_ids(rng, "low", n, n_ids), n_ids, flags=FORGET | LEARN)
    assert st.sweeps == 4 and st.finisher == 1 and not st.walked and st.beyond[0] * 8 <= n and st.learnt == 2
    later = LEARN if learn_all else 0
    st = check(eng, kind, PLAIN, gen_ids(rng, "high", n, n_ids), n_ids, flags=later)
    assert st.sweeps == 2 and st.done == [1, 0, 0, 0] and st.beyond[0] > n * 9 // 10   # by the hint, against the data
    assert st.learnt == (1 if learn_all else 2)
    for m in (n // 10, n * 10):
        st = check(eng, kind, PLAIN, gen_ids(rng, "high", m, n_ids), n_ids, flags=later)
        assert st.sweeps == (1 if learn_all else 2) and st.done == [1, 0, 0, 0] and st.beyond[0] > m * 9 // 10
    assert {"first sweep finished by hint", "launches cut by learning"} <= SEEN
    # and the marked and the gathered form under the same stale hint
    for form in (MARKED, GATHER):
        ids, tab = in_form(rng, form, gen_ids(rng, "uniform", n + 1, n_ids), n_ids)
        st = check(eng, kind, form, ids, n_ids, tab, mis=form, flags=later)
        assert st.done == [1, 0, 0, 0]


@pytest.mark.parametrize("kind", KINDS)
def test_learnt_down_to_one_sweep(eng, kind):
    rng = np.random.default_rng(41 + kind)
    st = check(eng, kind, PLAIN, gen_ids(rng, "uniform", 100_000, HOT), HOT, flags=FORGET | LEARN)
    assert st.sweeps == 1 and st.learnt == 1
    n_ids = 10 * HOT
    st = check(eng, kind, PLAIN, gen_ids(rng, "uniform", 500_000, n_ids), n_ids, flags=0)
    assert st.sweeps == 1 and st.done == [1, 0, 0, 0] and st.beyond[0] > 400_000


def test_kinds_keep_their_own_hint_and_sweeps(eng):
    rng = np.random.default_rng(51)
    n, n_ids = 400_000, 4 * HOT
    st = check(eng, NODES, PLAIN, gen_ids(rng, "low", n, n_ids), n_ids, flags=FORGET | LEARN)
    assert st.finisher == 1 and st.learnt == 2
    # the edge classes know nothing of that: four sweeps, no early finish
    big = 10 * HOT
    st = check(eng, EDGES, PLAIN, gen_ids(rng, "uniform", 500_001, big), big, flags=0)
    assert st.sweeps == 4 and st.done == [0, 0, 0, 1]
    st = check(eng, NODES, PLAIN, gen_ids(rng, "high", n, n_ids), n_ids, flags=0)
    assert st.sweeps == 2 and st.done == [1, 0, 0, 0]
    # learning takes the done flags of both kinds, each from its own last count: the edge classes used four sweeps, the
    # nodes' last count finished in its first
    st = check(eng, EDGES, MARKED, mark(rng, gen_ids(rng, "uniform", 300_000, big)), big, flags=LEARN)
    assert st.sweeps == 4 and st.done == [0, 0, 0, 1] and st.learnt == 4
    st = check(eng, NODES, PLAIN, gen_ids(rng, "uniform", n, n_ids), n_ids, flags=LEARN)
    assert st.sweeps == 1 and st.done == [1, 0, 0, 0] and st.learnt == 1
    st = check(eng, EDGES, PLAIN, gen_ids(rng, "high", 500_001, big), big, flags=0)
    assert st.sweeps == 4 and st.done == [0, 0, 0, 1]
    # an edge-class count small enough for the lists, with the nodes' hint around: its own second launch walks
    st = check(eng, EDGES, PLAIN, with_beyond(rng, 2 * HOT, 100, span=big - HOT), big, flags=0)
    assert st.sweeps == 4 and st.walked


def test_forgetting_restores_a_new_context(eng):
    from amira_amd import Engine
    rng = np.random.default_rng(61)
    n, n_ids = 400_000, 4 * HOT
    high = gen_ids(rng, "high", n, n_ids)
    for kind in KINDS:
        st = check(eng, kind, PLAIN, gen_ids(rng, "low", n, n_ids), n_ids, flags=LEARN)
        assert st.learnt <= 2
    fresh = Engine(0)
    try:
        for kind in KINDS:
            # only the first of the two forgets: the second count runs on what the first one left, on both contexts
            a = check(eng, kind, PLAIN, high, n_ids, flags=FORGET if kind == NODES else 0)
            b = check(fresh, kind, PLAIN, high, n_ids, flags=0)
            assert a.sweeps == 4 and a.done == [0, 0, 0, 1]
            assert np.array_equal(a.words[:14], b.words[:14]), (a, b)
    finally:
        fresh.close()


def test_random_mix(eng):
    rng = np.random.default_rng(2024)
    for j in range(64):
        kind, form = int(rng.integers(0, 2)), int(rng.integers(0, 3))
        n = 0 if rng.random() < 0.05 else int(2_000_000 ** rng.random()) + int(rng.integers(0, 4))
        n_ids = int(rng.choice(N_IDS)) if rng.random() < 0.5 else int(rng.integers(1, 12 * HOT + 1))
        dist = DISTS[int(rng.integers(0, len(DISTS)))]
        scale = float(rng.choice([HOT / 8, HOT / 4, HOT / 2, HOT, 3 * HOT]))
        mis = int(rng.integers(0, 4))
        flags = (FORGET if rng.random() < 0.15 else 0) | (LEARN if rng.random() < 0.5 else 0)
        ids, tab = in_form(rng, form, gen_ids(rng, dist, n, n_ids, scale=scale), n_ids)
        check(eng, kind, form, ids, n_ids, tab, mis=mis, flags=flags)


def test_out_of_range_ids_are_refused(eng):
    """the probe does not hand the sweeps an id they would index a counter with out of bounds"""
    from amira_amd import _ffi
    for form, ids, tab in ((PLAIN, [0, 5], None), (MARKED, [5 | MADE], None), (GATHER, [0, 1], [0, 5]), (GATHER, [2], [0, 1])):
        with pytest.raises(_ffi.AmgError) as ei:
            probe(eng, NODES, form, np.array(ids, np.int32), 5, None if tab is None else np.array(tab, np.int32))
        assert ei.value.code == -2


def test_every_regime_was_seen():
    assert SEEN == REGIMES, sorted(REGIMES - SEEN)
