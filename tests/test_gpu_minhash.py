"""amg_minhash (HIP) against the restated sourmash MinHash of the oracle, and the reference-held
containments through the product's bubble-popping API."""
import numpy as np
import pytest

import procedures as P

pytestmark = pytest.mark.gpu


def _random_segments(rng, n, lo, hi):
    alphabet = np.frombuffer(b"ACGTacgtNRY", dtype=np.uint8)
    probs = np.array([0.23, 0.23, 0.23, 0.23, 0.015, 0.015, 0.015, 0.015, 0.01, 0.005, 0.005])
    segs = []
    for _ in range(n):
        L = int(rng.integers(lo, hi))
        segs.append(bytes(rng.choice(alphabet, size=L, p=probs / probs.sum())).decode())
    return segs


@pytest.mark.parametrize("ksize,scaled", [(11, 10), (9, 1), (21, 3), (4, 1), (32, 2),
                                          (1, 1), (8, 1), (16, 1), (17, 1), (24, 2), (25, 1), (31, 1)])   # (word boundaries of amg_bases.h)
def test_device_sketch_equals_oracle(ksize, scaled):
    from amira_amd import Engine
    from amira_oracle.minhash import MinHash
    rng = np.random.default_rng(ksize * 100 + scaled)
    segs = _random_segments(rng, 200, 0, 3000) + ["", "ACG", "N" * 50, "ACGT" * 700]
    sets = [int(x) for x in rng.integers(0, 17, len(segs))]
    eng = Engine(0)
    try:
        got = eng.minhash(segs, sets, ksize, scaled)
    finally:
        eng.close()
    want = {s: MinHash(n=0, ksize=ksize, scaled=scaled) for s in set(sets)}
    for seg, s in zip(segs, sets):
        want[s].add_sequence(seg, force=True)
    assert set(got) == set(want)
    for s in want:
        assert got[s] == set(want[s].hashes), s
    assert sum(len(v) for v in got.values()) > 0


def test_reference_held_containments_through_the_product():
    """tests/test_gene_mer_graph.py:5119-5155 through amira_amd.GeneMerGraph (device sketches)"""
    import dump as D
    from amira_amd import GeneMerGraph
    calls, pos = D.load_fixture("test_path_calls"), D.load_fixture("test_path_positions")
    g = GeneMerGraph(calls, 3, pos)
    fq = P.real_fastq()
    starts = g.identify_potential_bubble_starts()
    checked = 0
    for component in g.components():
        if component not in starts:
            continue
        unique = g.get_all_paths_between_junctions_in_component(starts[component], g.get_kmerSize() * 3, 1)
        filtered = sorted(g.filter_paths_between_bubble_starts(unique), key=lambda x: len(x[0]), reverse=True)
        sketches = g.get_minhashes_for_paths(filtered, fq, 1)
        m1 = g.get_minimizers_from_minhashes([n[0] for n in filtered[0][0]], sketches)
        m2 = g.get_minimizers_from_minhashes([n[0] for n in filtered[1][0]], sketches)
        assert len(m1 & m2) / len(m1) == 0.9105839416058394
        assert len(m1 & m2) / len(m2) == 0.9091323161011159
        checked += 1
    assert checked == 1


# ------------------------------------------------------------------ segment boundaries against the tiles of k_minhash
TILE = 1024    # BT_TILE (amg_bases.h): k-mer starts per workgroup


def _compare(segs, ksize, scaled=1):
    """every segment a sketch of its own, on the device and by the oracle; returns the number of hashes compared"""
    import path_sketch as PS
    from amira_amd import Engine
    eng = Engine(0)
    try:
        got = eng.minhash(segs, list(range(len(segs))), ksize, scaled)
    finally:
        eng.close()
    assert sorted(got) == list(range(len(segs)))
    for s, seg in enumerate(segs):
        assert got[s] == set(PS.sketch(seg, ksize, scaled)), (s, len(seg), ksize)
    return sum(len(v) for v in got.values())


def _cut(text, cuts):
    cuts = [0] + sorted(set(cuts)) + [len(text)]
    return [text[a:b] for a, b in zip(cuts, cuts[1:])]


@pytest.mark.parametrize("ksize", [1, 8, 11, 17, 32])
def test_segment_boundaries_on_the_edges_of_a_tile(ksize):
    """boundaries at stream offsets 1023, 1024, 1025, 2048 - ksize and 2048 - ksize + 1, and a segment whose last window
    ends on the last base of a tile (it ends at 2048); no window may run from one segment into the next"""
    import path_sketch as PS
    rng = np.random.default_rng(500 + ksize)
    text = PS.bases(rng, 3 * TILE + 77)
    segs = _cut(text, [1023, 1024, 1025, 2 * TILE - ksize, 2 * TILE - ksize + 1, 2 * TILE, 3 * TILE - 1])
    assert np.cumsum([len(s) for s in segs])[:-1].tolist() == sorted({1023, 1024, 1025, 2048 - ksize, 2049 - ksize, 2048, 3071})
    assert _compare(segs, ksize) > 0
    # the same bases as ONE segment have more windows than the pieces: those across the cuts
    assert len(PS.sketch(text, ksize, 1)) > len(set().union(*[PS.sketch(s, ksize, 1) for s in segs])) or ksize == 1


@pytest.mark.parametrize("scaled", [1, 2, 10, 2048, 2 ** 63])
def test_the_scaled_cut_is_the_oracles(scaled):
    """km_max_hash (amg_bases.h) through a sketch: the hashes kept are those at or below the oracle's max_hash"""
    import path_sketch as PS
    from amira_oracle.minhash import max_hash_for_scaled
    assert [max_hash_for_scaled(s) for s in (1, 2, 10, 2048, 2 ** 63)] == [2 ** 64 - 1, 2 ** 63, 1844674407370955264,
                                                                            2 ** 53, 2]
    kept = _compare([PS.bases(np.random.default_rng(550), 20000)], 11, scaled)
    if scaled == 1:
        assert kept > 19000
    elif scaled == 2 ** 63:
        assert kept == 0            # (a hash of 2 or less)
    else:
        assert 0 < kept < 2 * 20000 // scaled   # (1 / scaled of the windows, within a factor of two)


@pytest.mark.parametrize("ksize", [2, 3, 11])
def test_hundreds_of_tiny_segments_in_one_tile_before_a_long_one(ksize):
    import path_sketch as PS
    rng = np.random.default_rng(600 + ksize)
    segs = [PS.bases(rng, n) for n in rng.choice(4, 700, p=[0.3, 0.3, 0.2, 0.2])]
    assert sum(len(s) for s in segs) < TILE and {len(s) for s in segs} == {0, 1, 2, 3}
    segs.append(PS.bases(rng, 1500))
    assert _compare(segs, ksize) > 10


@pytest.mark.parametrize("ksize", [4, 11])
def test_runs_of_empty_segments_on_a_tile_edge_and_at_the_end(ksize):
    import path_sketch as PS
    rng = np.random.default_rng(700 + ksize)
    segs = [""] * 3 + [PS.bases(rng, TILE)] + [""] * 20 + [PS.bases(rng, 700)] + [""] * 70 + [PS.bases(rng, 324 + TILE)] + [""] * 5
    assert _compare(segs, ksize) > 300


@pytest.mark.parametrize("n", [TILE, TILE + 1])
@pytest.mark.parametrize("ksize", [1, 11, 32])
def test_a_stream_of_one_tile_and_of_one_base_more(n, ksize):
    import path_sketch as PS
    rng = np.random.default_rng(800 + n + ksize)
    text = PS.bases(rng, n)
    assert _compare([text], ksize) > 0
    assert _compare([text[:1000], text[1000:]], ksize) > 0


def test_capacity_smaller_than_the_result_and_null_outputs():
    """include/amg.h: out_set / out_hash may be NULL to get the count only; with a cap below the count the count is the
    same and nothing is written behind cap"""
    import ctypes as C
    from collections import Counter
    import path_sketch as PS
    from amira_amd import Engine, _ffi
    from amira_amd._ffi import check, ptr
    ksize, scaled = 11, 3
    rng = np.random.default_rng(900)
    segs = [PS.bases(rng, n) for n in (700, 0, 1024, 5, 1300)] + ["ACGTTGCAAGTC" * 40]   # (the last: hashes many times over)
    sets = np.array([0, 1, 2, 2, 0, 3], np.int32)
    offs = np.zeros(len(segs) + 1, np.int64)
    np.cumsum([len(s) for s in segs], out=offs[1:])
    stream = np.frombuffer("".join(segs).encode(), np.uint8)
    want = Counter((int(sets[i]), h) for i, seg in enumerate(segs) for j in range(len(seg) - ksize + 1)
                   for h in PS.sketch(seg[j:j + ksize], ksize, scaled))
    total = sum(want.values())
    assert total > len(want) > 500
    GUARD_S, GUARD_H = np.int32(-77), np.uint64(0xDEADBEEFDEADBEEF)
    eng = Engine(0)
    try:
        def run(cap, with_outputs=True):
            o_set, o_hash = np.full(cap + 8, GUARD_S, np.int32), np.full(cap + 8, GUARD_H, np.uint64)
            n = C.c_int64(-1)
            check(_ffi.lib.amg_minhash(eng._h, ptr(stream), ptr(offs), ptr(sets), len(segs), ksize, scaled,
                                       ptr(o_set) if with_outputs else None, ptr(o_hash) if with_outputs else None, cap,
                                       C.byref(n)))
            return n.value, o_set, o_hash
        assert run(0, False)[0] == total
        assert run(total, False)[0] == total           # (a cap without outputs is not a promise of room)
        for cap in (total, total - 1, 1, total + 5):
            n, o_set, o_hash = run(cap)
            assert n == total, cap
            m = min(cap, total)
            got = Counter(zip(o_set[:m].tolist(), o_hash[:m].tolist()))
            assert not got - want, (cap, "pairs that are not among the expected ones")
            assert cap < total or got == want
            assert (o_set[m:] == GUARD_S).all() and (o_hash[m:] == GUARD_H).all(), cap
    finally:
        eng.close()
