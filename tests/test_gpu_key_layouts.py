"""Single-engine and merged builds at every k in 2 .. 16 on three vocabulary sizes (tests/key_layouts.py), so that every
key scheme and record layout that (k, two_v) can select runs: one- and two-word exact keys in both packings, 94-bit
fingerprint keys, the 32-byte fingerprint path with packed node records (tuple positions 10 .. 13 in words 6 and 7,
tokens with bit 15 set) and with unpacked ones (k = 15, 16; more than 65 536 tokens), and the held node records of a
merge with 16-bit tokens (padded at odd k, full at even k) and with 32-bit tokens.  Everything is compared exactly with
the sequential C oracle; in a merged build on every rank, window ids as the rank's slice of the oracle's.

Every engine is rebuilt through K_ORDER (16, 3, 15, 2, ...): its tables, the held records and the per-claim arrays are
grow-only buffers that the previous, differently sized build filled.

What a test can see of the layout: amg_counts' exact_keys tells exact slots, 94-bit fingerprints in 16-byte slots and
the 32-byte path apart, on the shards of a merged build too.  Whether 32-byte node records were packed and which form
the held records took is not reported; the line a case prints per build states what key_layouts.layout derives from
(k, two_v)."""
import numpy as np
import pytest

import key_layouts as KL

pytestmark = pytest.mark.gpu

MODES = {"default": {}, "fp": {"AMG_KEY_MODE": "fp"}}
NODE_KEYS = ("tokens", "coverage", "first_dir")
EDGE_KEYS = (("src", "src"), ("tgt", "tgt"), ("sdir", "sdir"), ("tdir", "tdir"), ("coverage", "ecov"))


def assert_graph(eng, want, what):
    """node tuples, coverages, first directions and the five directed-edge arrays equal the oracle's"""
    nodes, edges = eng.nodes(), eng.edges()
    for key in NODE_KEYS:
        assert np.array_equal(nodes[key], want[key]), (what, key)
    for a, b in EDGE_KEYS:
        assert np.array_equal(edges[a], want[b]), (what, a)


def assert_windows(eng, want, offs, lo, hi, k, what):
    """the engine holds reads lo .. hi - 1 of the read set: its window -> node ids and directions are that slice of the
    oracle's, its window and short-read counts those of its reads"""
    tok_node, tok_dir = eng.read_nodes()
    a, b = int(offs[lo]), int(offs[hi])
    assert np.array_equal(tok_node, want["tok_node"][a:b]), (what, "tok_node")
    assert np.array_equal(tok_dir, want["tok_dir"][a:b]), (what, "tok_dir")
    n = np.diff(offs[lo:hi + 1])
    c = eng.counts()
    assert c["n_windows"] == int(np.maximum(n - k + 1, 0).sum()), (what, "n_windows")
    assert c["n_short_reads"] == int((n < k).sum()), (what, "n_short_reads")
    return c


def make_ranks(name, world):
    from amira_amd import Engine
    toks, offs, two_v = KL.read_set(name)
    bounds = KL.shard_bounds(len(offs) - 1, world)
    engines = []
    try:
        for r in range(world):
            lo, hi = bounds[r], bounds[r + 1]
            e = Engine(0)
            engines.append(e)
            e.set_reads(toks[offs[lo]:offs[hi]], offs[lo:hi + 1] - offs[lo], two_v)
    except BaseException:
        for e in engines:
            e.close()
        raise
    return engines, bounds


def set_env(monkeypatch, env):
    for name in ("AMG_KEY_MODE", "AMG_COUNT_INLINE", "AMG_TEST_WEAK_FP", "AMG_TEST_DIST_WEAK_KEYS"):
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


# ------------------------------------------------------------------ a. single engine
SINGLE_ARMS = {"default": ({}, KL.K_ORDER), "fp": ({"AMG_KEY_MODE": "fp"}, KL.K_ORDER),
               "inline": ({"AMG_COUNT_INLINE": "1"}, (15, 5, 12))}


@pytest.mark.parametrize("arm", list(SINGLE_ARMS))
@pytest.mark.parametrize("name", list(KL.VOCABS))
def test_single_engine_at_every_k(name, arm, monkeypatch):
    """default: the scheme the tuple width selects (exact_keys 1 while k * bits <= 94, 2 beyond); AMG_KEY_MODE=fp: the
    32-byte path everywhere; AMG_COUNT_INLINE=1: the 32-byte path with the counts in the slot, read out before the slot
    is packed"""
    from amira_amd import Engine
    env, ks = SINGLE_ARMS[arm]
    set_env(monkeypatch, env)
    toks, offs, two_v = KL.read_set(name)
    eng = Engine(0)
    try:
        eng.set_reads(toks, offs, two_v)
        for k in ks:
            want = KL.oracle(name, k)
            lay = KL.layout(k, two_v, arm != "default", False)
            eng.build(k)
            what = (name, arm, k)
            assert_graph(eng, want, what)
            c = assert_windows(eng, want, offs, 0, len(offs) - 1, k, what)
            assert (c["n_windows"], c["n_short_reads"]) == (want["n_windows"], want["n_short"]), what
            print(f"layout single {name} k={k} {arm}: exact_keys {c['exact_keys']} ({lay['slots']}), "
                  f"{c['n_nodes']} nodes, {c['n_edges']} edges")
            assert c["exact_keys"] == lay["exact_keys"], what
    finally:
        eng.close()


# ------------------------------------------------------------------ b. merged build over emulated ranks
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", list(KL.VOCABS))
def test_merged_build_at_every_k(name, world, mode, monkeypatch):
    """the same ranks build k = 16, 3, 15, 2, ...: every rank ends with the oracle's graph, whatever record size the
    merge before it left in the held records, the node table and the per-claim arrays"""
    from amira_amd.dist import dist_build_loopback
    set_env(monkeypatch, MODES[mode])
    toks, offs, two_v = KL.read_set(name)
    engines, bounds = make_ranks(name, world)
    try:
        for k in KL.K_ORDER:
            want = KL.oracle(name, k)
            lay = KL.layout(k, two_v, mode == "fp", True)
            dist_build_loopback(engines, k)
            seen, windows, short = [], 0, 0
            for r, e in enumerate(engines):
                what = (name, world, mode, k, "rank", r)
                assert_graph(e, want, what)
                c = assert_windows(e, want, offs, bounds[r], bounds[r + 1], k, what)
                windows, short = windows + c["n_windows"], short + c["n_short_reads"]
                seen.append(c["exact_keys"])
            print(f"layout merged {name} k={k} world={world} {mode}: exact_keys {seen} ({lay['slots']}; held records "
                  f"{lay['held']}), {len(want['coverage'])} nodes, {len(want['src'])} edges")
            assert seen == [lay["exact_keys"]] * world, (name, world, mode, k)
            assert (windows, short) == (want["n_windows"], want["n_short"]), (name, world, mode, k)
    finally:
        for e in engines:
            e.close()


# ------------------------------------------------------------------ c. merged build with the fused filter
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("name", list(KL.VOCABS))
def test_merged_build_with_fused_filter(name, world, mode, monkeypatch):
    """filter_graph(2, 1) and (3, 1) fused into the merge: dropped nodes come back from their key's owner as such, and
    the slot's record — packed or not — must say so to the edge pass; against the oracle's build followed by filter"""
    from amira_amd.dist import dist_build_loopback
    from helpers import live_arrays
    set_env(monkeypatch, MODES[mode])
    toks, offs, two_v = KL.read_set(name)
    engines, bounds = make_ranks(name, world)
    try:
        for k in (15, 4, 12, 9):
            for thr in ((2, 1), (3, 1)):
                want = KL.filtered_oracle(name, k, thr)
                assert 0 < len(want["coverage"]) < len(KL.oracle(name, k)["coverage"])   # some dropped, some kept
                dist_build_loopback(engines, k, *thr)
                for r, e in enumerate(engines):
                    what = (name, world, mode, k, thr, "rank", r)
                    got = live_arrays(e)
                    lo, hi = bounds[r], bounds[r + 1]
                    for key in ("tokens", "coverage", "first_dir", "src", "tgt", "sdir", "tdir", "ecov", "adj_off", "adj"):
                        assert np.array_equal(got[key], want[key]), (what, key)
                    assert np.array_equal(got["tok_node"], want["tok_node"][offs[lo]:offs[hi]]), what
                    assert np.array_equal(got["tok_dir"], want["tok_dir"][offs[lo]:offs[hi]]), what
                    assert np.array_equal(got["to_correct"], want["to_correct"][lo:hi]), what
    finally:
        for e in engines:
            e.close()


# ------------------------------------------------------------------ d. collisions in both verify branches
COLLISION_POINTS = [("small", 12), ("small", 15), ("wide", 5)]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name,k", COLLISION_POINTS)
def test_weak_fingerprints_are_caught(name, k, mode, monkeypatch):
    """AMG_TEST_WEAK_FP=1: the first attempt's fingerprints are cut to 12 bits, gene-mers share them, the verification
    must notice and the repeated build must be right.  With AMG_KEY_MODE=fp the 32-byte path verifies against the packed
    record (small, k = 12: positions 10 and 11 in word 6) or against node_tokens (k = 15; wide).  By default a tuple
    that does not fit (small, k = 12 and 15) is verified against its claim's first window instead, and one that would
    fit (wide, k = 5) is sent down the 32-byte path by the hook."""
    from amira_amd import Engine
    set_env(monkeypatch, dict(MODES[mode], AMG_TEST_WEAK_FP="1"))
    toks, offs, two_v = KL.read_set(name)
    want = KL.oracle(name, k)
    eng = Engine(0)
    try:
        eng.set_reads(toks, offs, two_v)
        eng.build(k)
        c = assert_windows(eng, want, offs, 0, len(offs) - 1, k, (name, k, mode))
        assert_graph(eng, want, (name, k, mode))
        print(f"weak fingerprints {name} k={k} {mode}: build_retries {c['build_retries']} exact_keys {c['exact_keys']}")
        assert c["build_retries"] >= 1
        fits = mode == "default" and KL.tuple_fits(k, two_v)
        assert c["exact_keys"] == (0 if mode == "fp" or fits else 2)
    finally:
        eng.close()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name,k", COLLISION_POINTS)
def test_weak_merge_keys_repeat_the_build(name, k, mode, monkeypatch):
    """AMG_TEST_DIST_WEAK_KEYS=1, two ranks: on fingerprint shards the first attempt's local fingerprints are weak and
    the edge pass's verify — packed at (small, 12), unpacked at (small, 15) and on wide — reports it; on exact shards
    (wide, k = 5 by default) the merge keys are cut to 10 bits and a key's holder reports the foreign tuple.  Every rank
    repeats the build and ends with the oracle's graph."""
    from amira_amd.dist import dist_build_loopback
    set_env(monkeypatch, dict(MODES[mode], AMG_TEST_DIST_WEAK_KEYS="1"))
    toks, offs, two_v = KL.read_set(name)
    want = KL.oracle(name, k)
    engines, bounds = make_ranks(name, 2)
    try:
        for e in engines:
            e.dist_stats(reset=True)
        dist_build_loopback(engines, k)
        repeats = [e.dist_stats(reset=False)["repeated_builds"] for e in engines]
        print(f"weak merge keys {name} k={k} {mode}: repeated_builds {repeats}")
        assert all(x >= 1 for x in repeats), repeats
        for r, e in enumerate(engines):
            what = (name, k, mode, "rank", r)
            assert_graph(e, want, what)
            assert_windows(e, want, offs, bounds[r], bounds[r + 1], k, what)
    finally:
        for e in engines:
            e.close()


# ------------------------------------------------------------------ e. tiny vocabularies on the 32-byte path
@pytest.mark.parametrize("inline", [None, "1"])
def test_tiny_vocabularies_on_the_fingerprint_path(inline, monkeypatch):
    """V = 2, 3, 6, 12 and 40 with planted period-2 reads (self-loops, edge classes of both signs between one pair of
    nodes, single nodes across read ends) through stage_tile / k_node_upsert / k_edges of the 32-byte path, the counts
    from the counting sweep or from the slot"""
    import token_oracle
    from amira_amd import Engine
    set_env(monkeypatch, {"AMG_KEY_MODE": "fp"} if inline is None else {"AMG_KEY_MODE": "fp", "AMG_COUNT_INLINE": inline})
    eng = Engine(0)
    try:
        for seed, V, n_reads, k in KL.EDGE_CLASS_CASES:
            toks, offs = KL.edge_class_reads(seed, V, n_reads, k)
            want = token_oracle.build(toks, offs, k, 2 * V)
            eng.set_reads(toks, offs, 2 * V)
            eng.build(k)
            what = (seed, V, k, inline)
            assert (want["coverage"] == 1).sum() > 20, "the case has no single nodes"
            assert_graph(eng, want, what)
            c = assert_windows(eng, want, offs, 0, len(offs) - 1, k, what)
            assert c["exact_keys"] == 0, what
    finally:
        eng.close()
