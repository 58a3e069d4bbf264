"""GPU: the position carry-over kernels (amg_correct_nw.hip: k_corr_nw_fast with its two shortcuts, its row-wise fill,
traceback and ballot-parallel position pass; k_corr_nw in LDS and in global scratch; k_nw_sizes, k_nw_place and the
host steps around them) on pairs of gene lists the tests choose, one batch per call through amg_nw_probe, against
the reference's needleman_wunsch + carry-over loop + replace_invalid_gene_positions (tests/carry_over.py, held equal
to the pinned oracle by tests/test_carry_over_cpu.py).

Everything is integer equality: the positions, the route every pair took against the route predicted for it from the
shortcut rules of test_nw_shortcut_cpu.py and the kernels' limits, the three totals of the shape fetch against what
the sizes imply, and the probe's guard words.  Every pair set runs with the shortcuts (flags 0), without them (2: every
pair of the fast kernel fills its matrix) and through the general kernel (1), and must give the same positions.
Original positions are random 64-bit values in no order, distinct within a pair, up to 2^62; read lengths are random
(the `edit` set runs without any).  The last test asserts that the module saw every route (it needs the whole module
to have run)."""
import random

import numpy as np
import pytest

import carry_over as co

pytestmark = pytest.mark.gpu

SEEN = set()   # routes the device reported in this module (test_every_route_was_seen)
FLAGS = [0, co.NO_SHORTCUT, co.NO_FAST]


@pytest.fixture(scope="module")
def eng():
    from amira_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def check(eng, ps, flags=0, keep=None):
    """one probe call on a PairSet: positions, routes, totals and guards against the reference; returns the routes"""
    pairs = ps.pairs
    xt = [g for x, _ in pairs for g in x]
    yt = [g for _, y in pairs for g in y]
    xo = np.cumsum([0] + [len(x) for x, _ in pairs])
    yo = np.cumsum([0] + [len(y) for _, y in pairs])
    ps_, pe_ = [s for pos in ps.pos for s, _ in pos], [e for pos in ps.pos for _, e in pos]
    gs, ge, route, state = eng.nw_probe((xt, xo), (yt, yo), (ps_, pe_), ps.read_len, keep, flags)
    live = [p for p in range(len(pairs)) if not (keep is not None and keep[p])]
    want_route = ps.routes(flags, keep)
    what = (ps.name, flags)
    assert state[3] == 1, what
    bad = [p for p in range(len(pairs)) if route[p] != want_route[p]]
    assert not bad, (what, bad[:5], [(int(route[p]), want_route[p]) + pairs[p] for p in bad[:2]])
    assert tuple(int(v) for v in state[:3]) == co.expected_totals(pairs, want_route), what
    want_s = np.array([v for p in live for v in ps.ref[p][0]], np.int64)
    want_e = np.array([v for p in live for v in ps.ref[p][1]], np.int64)
    assert gs.size == want_s.size
    if not (np.array_equal(gs, want_s) and np.array_equal(ge, want_e)):
        at = 0
        for p in live:   # the first pair that differs, in full
            n = len(pairs[p][0])
            got = (gs[at:at + n].tolist(), ge[at:at + n].tolist())
            assert got == (ps.ref[p][0], ps.ref[p][1]), (what, p, int(route[p]), pairs[p], ps.pos[p], ps.rl(p), got)
            at += n
    SEEN.update(int(r) for r in route)
    return [int(r) for r in route], state


def pair_set(name, pairs, seed=1, with_read_len=True):
    return co.PairSet(name, pairs, seed, with_read_len)


# ------------------------------------------------------------------ the generated sets
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("name", [s[0] for s in co.SETS])
def test_generated_set(eng, name, flags):
    ps = co.generated(name)
    assert (ps.read_len is None) == (name == co.NO_READ_LEN)
    routes, _ = check(eng, ps, flags)
    if name == "disjoint":   # every position repaired: the head from 0, the tail to the read length - 1
        for p, (x, _) in enumerate(ps.pairs):
            assert ps.ref[p][0] == [0] * len(x) and ps.ref[p][1] == [ps.read_len[p] - 1] * len(x)
    if name == "middle":
        for p in range(len(ps.pairs)):
            assert ps.ref[p][0][0] == 0 and ps.ref[p][1][-1] == ps.read_len[p] - 1


# ------------------------------------------------------------------ named edges
def shaped(rng, n, m):
    """pairs of one shape: uniform over two genes and over fifty, an edited copy, a tandem array, disjoint lists"""
    out = []
    for alpha in (2, 50):
        out.append(([rng.randrange(alpha) for _ in range(n)], [rng.randrange(alpha) for _ in range(m)]))
    y = rng.sample(range(5000), m)
    x = [y[min(i * m // n, m - 1)] for i in range(n)] if n > m else y[(m - n) // 2:(m - n) // 2 + n]
    for _ in range(1 + n // 16):
        x[rng.randrange(n)] = rng.choice(y)
    out.append((x, y))
    out.append(([7] * n, [7] * (m - 1) + [8]))
    out.append(([9000 + i for i in range(n)], y))
    return out


SHAPE_SETS = {}   # the named sets, made once and shared by the three runs of each
SHAPES = ([(1, 1), (1, 64), (128, 1), (128, 64)] +
          [(n, m) for n in (15, 16, 17, 63, 64, 65, 112, 113, 127) for m in (64, 7)] +
          [(1, 65), (128, 65), (128, 128), (128, 129), (129, 128), (1025, 3), (3, 1025)])


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shape(eng, shape, flags):
    n, m = shape
    ps = SHAPE_SETS.get(shape)
    if ps is None:
        ps = SHAPE_SETS[shape] = pair_set(f"{n}x{m}", shaped(random.Random(n * 2000 + m), n, m), seed=n + m)
    routes, state = check(eng, ps, flags)
    if not co.fast_ok(n, m) or flags & co.NO_FAST:
        assert set(routes) == {co.R_LDS if co.in_lds(n, m) else co.R_GLOBAL}
        assert state[2] == len(ps.pairs) and (state[0] > 0) == (not co.in_lds(n, m))
    elif flags & co.NO_SHORTCUT:
        assert set(routes) == {co.R_FILL}


def lane63_pairs():
    """64 against 64 with mismatches at places 0 and 63 (upto_b with b = 63, sufD at lane 63): where the rule takes
    the diagonal, and where a shifted alignment ties with it and the matrix must be filled"""
    y = list(range(100, 164))
    out = []
    for at in ((0, 63), (63,), (0,), (0, 31, 63), (0, 1, 62, 63), (62, 63), (0, 1, 2, 63)):
        x = list(y)
        for i in at:
            x[i] = 9000 + i
        out.append((x, y))
    out.append(([1] * 63 + [3], [2] + [1] * 63))            # x[i] == y[i+1] for every i < 63: ties, two mismatches
    out.append(([2] + [1] * 63, [1] * 63 + [3]))            # the mirror image
    out.append(([1] * 62 + [3, 4], [2] + [1] * 63))         # three mismatches, the last two at 62 and 63
    out.append(([2, 5] + [1] * 62, [1] * 62 + [6, 3]))
    t = [1, 1, 2, 2] * 16                                   # tandem pairs, shifted by one with the ends replaced
    out.append(([9] + t[2:] + [8], t))
    out.append((t[1:] + [8], t))
    return out


@pytest.mark.parametrize("flags", FLAGS)
def test_mismatches_at_the_first_and_last_lane(eng, flags):
    ps = SHAPE_SETS.setdefault("lane63", pair_set("lane63", lane63_pairs(), seed=63))
    routes, _ = check(eng, ps, flags)
    if flags == 0:
        assert routes[0] == co.R_EQUAL and routes[7] == co.R_FILL and routes[8] == co.R_FILL


def beyond_pairs():
    rng = random.Random(77)
    return shaped(rng, 128, 65)[:2] + shaped(rng, 128, 129)[:2]


@pytest.mark.parametrize("flags", FLAGS)
def test_keep_original_pairs_between_the_others(eng, flags):
    """plen 0 and no record for the fast kernel: nothing is written for them, the others' positions are placed by the
    scan past them"""
    src = co.generated("uniform")
    pairs = src.pairs[:150] + beyond_pairs() + co.generated("trimmed").pairs[:60] + [([], [1, 2, 3])]
    ps = SHAPE_SETS.setdefault("keep", pair_set("keep", pairs, seed=5))
    rng = random.Random(9)
    keep = [1 if (rng.random() < 0.4 or not x) else 0 for x, _ in pairs]
    keep[0], keep[1], keep[-2] = 1, 0, 1
    routes, state = check(eng, ps, flags, keep)
    assert routes.count(co.R_NONE) == sum(keep) and state[1] == sum(len(x) for (x, _), k in zip(pairs, keep) if not k)


def mixed_pairs():
    return (co.generated("equal").pairs[:40] + co.generated("trimmed").pairs[:40] + beyond_pairs() +
            co.generated("uniform").pairs[:40])


@pytest.mark.parametrize("flags", FLAGS)
def test_every_route_in_one_call(eng, flags):
    ps = SHAPE_SETS.setdefault("mixed", pair_set("mixed", mixed_pairs(), seed=6))
    keep = [1 if p % 7 == 3 else 0 for p in range(len(ps.pairs))]
    routes, _ = check(eng, ps, flags, keep)
    if flags == 0:
        assert set(routes) == {co.R_NONE, co.R_EQUAL, co.R_CERT, co.R_FILL, co.R_LDS, co.R_GLOBAL}


def test_originals_in_the_pool_of_produced_positions(eng):
    """flag 4: the originals lie in the pool the products go to, the products make the pool move, the kernels read the
    originals where they are afterwards; then a second call, and an ordinary sweep on the same engine"""
    import procedures as P
    from test_gpu_sweep import run_sweep
    ps = co.generated("tall")
    for flags in FLAGS:
        _, state = check(eng, ps, flags | co.POOLED)
        assert state[4] == 1
    check(eng, co.generated("trimmed"), co.POOLED)
    check(eng, co.generated("trimmed"), 0)
    reads, pos, fq = P.synth_inputs(7, 400, 30, 300, 0.03)
    run_sweep(eng, reads, pos, fq, 5)
    check(eng, co.generated("middle"), co.POOLED)


def test_probe_between_set_positions_and_correct(eng):
    """the probe borrows the context's position arrays and both pools: called after set_positions, before the
    correction, and again once the positions live in the pool of produced ones (after adopt_corrected), it leaves
    both corrections of a sweep as they are without it"""
    import procedures as P
    from amira_amd import tokenize
    from helpers import flat_positions
    reads, pos, fq = P.synth_inputs(17, 800, 40, 150, 0.05)
    vocab, toks, offs, read_ids = tokenize(reads)
    gs, ge = flat_positions(read_ids, reads, pos)
    rl = np.asarray([len(fq[r]["sequence"]) for r in read_ids], dtype=np.int64)

    def two_corrections(probe):
        eng.set_reads(toks, offs, vocab.two_v)
        eng.set_positions(gs + (1 << 33), ge + (1 << 33), rl + (1 << 33))
        probe()
        eng.build(5)
        eng.filter(3, 1)
        probe()
        n = eng.correct_reads()
        first = eng.corrected(*n, True)
        eng.adopt_corrected()
        probe()
        eng.build(5)
        eng.remove_short_linear_paths(5)
        probe()
        n = eng.correct_reads()
        return first, eng.corrected(*n, True)

    def probe():
        check(eng, co.generated("trimmed"), 0)
        check(eng, co.generated("tall"), co.POOLED)

    plain = two_corrections(lambda: None)
    probed = two_corrections(probe)
    assert plain[0]["changed"].any() and plain[1]["changed"].any()   # positions were carried over both times
    for a, b in zip(plain, probed):
        for key in a:
            assert np.array_equal(a[key], b[key]), key


def test_what_the_kernels_cannot_take_is_refused(eng):
    from amira_amd import _ffi
    one = ([5], [1])
    for xt, xo, yt, yo, keep in (([-1], [0, 1], [1], [0, 1], None),    # a negative corrected gene
                                 ([1], [0, 1], [-3], [0, 1], None),    # a negative original gene
                                 ([1], [0, 1], [], [0, 0], None),      # an empty y
                                 ([1], [0, 1], [], [0, 0], [1]),       # also on a pair that keeps its genes
                                 ([], [0, 0], [1], [0, 1], None)):     # an empty x on a pair that does not
        with pytest.raises(_ffi.AmgError) as ei:
            eng.nw_probe((xt, xo), (yt, yo), ([7] * len(yt), [8] * len(yt)), None, keep)
        assert ei.value.code == -2
    # lengths beyond what the records hold (refused before a gene is read)
    i32, i64, u8 = np.zeros(4, np.int32), np.zeros(4, np.int64), np.zeros(4, np.uint8)
    for big_x in (True, False):
        long_, short = np.array([0, (1 << 24) + 1], np.int64), np.array([0, 1], np.int64)
        rc = _ffi.lib.amg_nw_probe(eng._h, 1, _ffi.ptr(i32), _ffi.ptr(long_ if big_x else short), _ffi.ptr(i32),
                                   _ffi.ptr(short if big_x else long_), _ffi.ptr(i64), _ffi.ptr(i64), None, None, 0,
                                   _ffi.ptr(i64), _ffi.ptr(i64), _ffi.ptr(u8), _ffi.ptr(np.zeros(8, np.int64)))
        assert rc == -2
    check(eng, pair_set("one", [one]), 0)   # and the engine goes on


def test_every_route_was_seen():
    assert SEEN == {co.R_NONE, co.R_EQUAL, co.R_CERT, co.R_FILL, co.R_LDS, co.R_GLOBAL}, SEEN
