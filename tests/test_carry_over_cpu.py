"""The reference side of tests/test_gpu_carry_over.py, without a GPU: the row-wise restatement of the carry-over
(tests/carry_over.py) equals the pinned oracle's needleman_wunsch + process_read_correction loop +
replace_invalid_gene_positions on the generated pairs, and the generated pair sets hold what the GPU tests need of
them — by the reference and the predicted routes alone: enough pairs for every route of k_corr_nw_fast, every number
of mismatches the equal-length rule decides on, enough equal-length pairs on which it declines, alignments that end on
either side of an op word and that need the second and third 64-column chunk of the position pass."""
from collections import Counter

import carry_over as co


def all_sets():
    return [co.generated(name) for name, _, _, _ in co.SETS]


def test_restatement_equals_the_oracle():
    """every pair of the small sets, the first 450 of the large ones (oracle: about 0.5 us per matrix cell)"""
    checked = 0
    for ps in all_sets():
        for p, (x, y) in enumerate(ps.pairs[:450]):
            want = co.carry_over(x, y, ps.pos[p], ps.rl(p))
            assert ps.ref[p] == want, (ps.name, p, x, y)
            assert len(want[0]) == len(x) and None not in want[0] and None not in want[1]
            checked += 1
    assert checked >= 2000


def test_restatement_on_lists_beyond_the_fast_kernel():
    import random
    rng = random.Random(5)
    for n, m in ((1, 65), (128, 65), (129, 128), (3, 300), (300, 3)):
        for alpha in (2, 50):
            x = [rng.randrange(alpha) for _ in range(n)]
            y = [rng.randrange(alpha) for _ in range(m)]
            pos = co.positions_for(rng, m)
            assert co.carry_over_fast(x, y, pos, 77) == co.carry_over(x, y, pos, 77)


def test_restatement_on_the_named_edge_sets():
    """the pairs of the GPU tests' named cases (every shape, the first and last lane, the lists beyond the fast kernel,
    the mixed batch): what the device is compared with there is what the oracle's own functions give"""
    import random
    import test_gpu_carry_over as g
    sets = [g.pair_set(f"{n}x{m}", g.shaped(random.Random(n * 2000 + m), n, m), seed=n + m) for n, m in g.SHAPES]
    sets += [g.pair_set("lane63", g.lane63_pairs(), seed=63), g.pair_set("beyond", g.beyond_pairs(), seed=5),
             g.pair_set("mixed", g.mixed_pairs(), seed=6)]
    for ps in sets:
        for p, (x, y) in enumerate(ps.pairs):
            assert ps.ref[p] == co.carry_over(x, y, ps.pos[p], ps.rl(p)), (ps.name, p, x, y)


def test_generated_sets_hold_the_mix():
    routes, mism, declined, n_ops = Counter(), Counter(), 0, []
    for ps in all_sets():
        for (x, y), r, ref in zip(ps.pairs, ps.routes(0), ps.ref):
            assert co.fast_ok(len(x), len(y)), (ps.name, len(x), len(y))
            routes[r] += 1
            n_ops.append(len(ref[2]))
            if len(x) == len(y):
                m = sum(a != b for a, b in zip(x, y))
                if r == co.R_EQUAL:
                    mism[m] += 1
                elif m in (2, 3, 4):
                    declined += 1
    print(dict(routes), dict(mism), declined)
    for r in (co.R_EQUAL, co.R_CERT, co.R_FILL):
        assert routes[r] >= 200, routes
    for m in range(5):
        assert mism[m] >= 40, mism
    assert set(mism) <= set(range(5))
    assert declined >= 100
    for rest in (0, 1, 15):
        assert any(n % 16 == rest for n in n_ops), rest
    assert sum(n > 64 for n in n_ops) >= 50 and sum(n > 128 for n in n_ops) >= 50


def test_predicted_route_order_and_limits():
    # equal length first: a list against itself is the equal-length rule's, though the certificate would take it too
    y = list(range(10))
    assert co.certificate_positions(y, y) is not None and co.predicted_route(y, y) == co.R_EQUAL
    assert co.predicted_route(y[2:8], y) == co.R_CERT
    assert co.predicted_route(y[2:8], y, co.NO_SHORTCUT) == co.R_FILL
    assert co.predicted_route(y[2:8], y, co.NO_FAST) == co.R_LDS
    assert co.predicted_route(y, y, keep=True) == co.R_NONE
    assert co.predicted_route(y + y, y[:1]) == co.R_FILL   # N > M: no certificate
    one = [0]
    assert co.predicted_route(one * 128, one * 64, co.NO_SHORTCUT) == co.R_FILL
    assert co.predicted_route(one * 128, one * 65) == co.R_LDS
    assert co.predicted_route(one * 129, one * 64) == co.R_LDS
    assert co.predicted_route(one * 128, one * 128) == co.R_LDS
    assert co.predicted_route(one * 128, one * 129) == co.R_GLOBAL
    assert co.predicted_route(one * 1025, one * 3) == co.R_GLOBAL
    assert co.predicted_route(one * 3, one * 1025) == co.R_GLOBAL
