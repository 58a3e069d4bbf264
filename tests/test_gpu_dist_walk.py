"""GPU: the read walks on a merged graph (amira_amd/csrc/amg_dist_walk.hip) — depth by read length (A), AMR trimming
(B), AMR reads per component (C) over the reads of W emulated ranks on ONE GPU — against the single-engine calls on the
unsharded build and against tests/read_walk_oracle.py.  Integer equality throughout; one process, no children.

The transports: amg_dist_walk_local (device copies between the ranks' engines), the host-driven begin / next / result
with the all-gathers made here in numpy, and amg_dist_walk over RCCL at world 1."""
import ctypes as C

import numpy as np
import pytest

import procedures as P
import read_walk_oracle as RW
from test_gpu_dist import assert_same_graph, graph_state, live_state, make_shards
from test_gpu_read_walk import CACHE_SLOTS, flags_for, genome_reads, lengths_asked, pack, some_flags

pytestmark = pytest.mark.gpu

E_ARG, E_STATE, E_DIST = -2, -3, -7
A, B, Cc = 1, 2, 3                      # AMG_WALK_DEPTH, _AMR_TRIM, _COMPONENT_READS
EXCHANGES = {A: 1, B: 2, Cc: 2}


@pytest.fixture(params=["exact", "fp"])
def key_mode(request, monkeypatch):
    """the main comparisons run twice: shards with exact-key local tables, and shards on the fingerprint path"""
    if request.param == "fp":
        monkeypatch.setenv("AMG_KEY_MODE", "fp")
    return request.param


# ------------------------------------------------------------------ read sets and the unsharded answer
def read_set(k):
    """about 80 reads over three genomes (several components): lengths on both sides of k, 64, 64 - k + 1 and 2k - 1,
    and one read of 1 100 genes (several chunks of the walker, all on one rank)"""
    rng = np.random.default_rng(40 + k)
    edge = [k - 1, k, k + 1, 63, 64, 65, 64 - k, 64 - k + 1, 64 - k + 2, 2 * k - 2, 2 * k - 1, 2 * k, 0, 1, 1100, 130]
    lengths = edge + rng.choice([2, k, k + 2, 2 * k - 1, 2 * k + 3, 30, 41, 66, 90], 64).tolist()
    order = rng.permutation(len(lengths))
    tokens, off, two_v = genome_reads(400 + k, [lengths[i] for i in order], period=300)
    return tokens, off, two_v


def positions(off):
    """gene positions and read lengths made up from the offsets: gene i of a read at [100 i, 100 i + 90]"""
    within = np.arange(off[-1], dtype=np.int64) - np.repeat(off[:-1], np.diff(off))
    return 100 * within, 100 * within + 90, 100 * np.diff(off) + 10


def unsharded(tokens, off, two_v, k, flags, after=None, rebuild=False):
    """what one engine holding all reads answers, and the oracle on its arrays; then B, and (rebuild) correct -> build"""
    from amira_amd import Engine
    e = Engine(0)
    try:
        e.set_reads(tokens, off, two_v)
        if rebuild:
            e.set_positions(*positions(off))
        e.build(k)
        if after is not None:
            after(e)
        nodes, tok_node = e.nodes(), e.read_node_ids()
        n_comp = e.counts()["n_components"]
        out = {"k": k, "flags": flags}
        out["A"] = e.depth_by_length(lengths_asked(k))
        want_pairs, want_alive = RW.depth_by_length(off, tok_node, nodes["alive"], k, lengths_asked(k))
        assert out["A"][0].tolist() == want_pairs and out["A"][1] == want_alive
        out["C"] = e.component_amr_reads(flags, 2 * k - 1)
        w_reads, w_long = RW.component_amr_reads(tokens, off, tok_node, nodes["alive"], nodes["component"], n_comp, k, flags,
                                                 2 * k - 1)
        assert out["C"][0].tolist() == w_reads.tolist() and out["C"][1].tolist() == w_long.tolist()
        out["B"] = e.remove_non_amr_nodes(flags)
        assert out["B"] == len(RW.non_amr_nodes(tokens, off, tok_node, nodes["alive"], k, flags))
        out["alive"], out["ealive"] = e.nodes()["alive"], e.edges()["alive"]
        out["counts"], out["tok_node"], out["to_correct"] = e.counts(), e.read_node_ids(), e.reads_to_correct()
        out["live"] = live_state(e)
        if rebuild:
            out["corrected"] = e.corrected(*e.correct_reads(), True)
            e.adopt_corrected()
            e.build(k)
            out["rebuilt"] = graph_state(e)
        return out
    finally:
        e.close()


_REF = {}


def reference(k):
    """computed once per k, shared and left unchanged"""
    if k not in _REF:
        tokens, off, two_v = read_set(k)
        flags = some_flags(tokens, two_v, k)[3]          # five genes of interest among those the reads hold
        _REF[k] = (tokens, off, two_v, unsharded(tokens, off, two_v, k, flags, rebuild=True))
    return _REF[k]


def shard_engines(tokens, off, two_v, bounds, world_hook=False):
    """rank r holds the reads bounds[r] .. bounds[r + 1]"""
    from amira_amd import Engine
    shards = [(tokens[off[lo]:off[hi]], off[lo:hi + 1] - off[lo], lo, hi) for lo, hi in zip(bounds[:-1], bounds[1:])]
    if bounds == even_bounds(len(off) - 1, len(bounds) - 1):      # (the even split is test_gpu_dist's)
        even = make_shards(tokens, off, len(bounds) - 1)
        assert [(s[2], s[3]) for s in even] == [(s[2], s[3]) for s in shards]
        shards = even
    engines = []
    for t, o, _, _ in shards:
        e = Engine(0)
        e.set_reads(t, o, two_v)
        engines.append(e)
    if world_hook:                                       # (AMG_DIST_ALWAYS_EXCHANGE is read when the world is set)
        for r, e in enumerate(engines):
            e.dist_init_external(r, len(engines))
    return engines


def even_bounds(n_reads, world):
    return [(r * n_reads) // world for r in range(world + 1)]


def close_all(engines):
    for e in engines:
        e.close()


def exchanges(engines):
    got = [e.dist_stats()["exchanges"] for e in engines]
    assert len(set(got)) == 1
    return got[0]


def check_walks(engines, bounds, off, want, on_wire=True, same_ids=True):
    """A, C, then B of the loop-back walks against the unsharded answer `want`; the state B leaves on every rank"""
    from amira_amd import dist
    k, flags = want["k"], want["flags"]
    for e in engines:
        e.dist_stats(reset=True)
    pairs, n_alive = dist.dist_depth_by_length_loopback(engines, lengths_asked(k))
    assert pairs.tolist() == want["A"][0].tolist() and n_alive == want["A"][1]
    if on_wire:
        assert exchanges(engines) == EXCHANGES[A]
    n_reads, n_long = dist.dist_component_amr_reads_loopback(engines, flags, 2 * k - 1)
    if same_ids:
        assert n_reads.tolist() == want["C"][0].tolist() and n_long.tolist() == want["C"][1].tolist()
    else:   # (a fused filter labels the components of the FILTERED graph: the same components under other ids)
        assert sorted(p for p in zip(n_reads.tolist(), n_long.tolist()) if p[0]) == \
            sorted(p for p in zip(want["C"][0].tolist(), want["C"][1].tolist()) if p[0])
    if on_wire and len(n_reads):
        assert exchanges(engines) == EXCHANGES[Cc]
    assert dist.dist_remove_non_amr_nodes_loopback(engines, flags) == want["B"]
    if on_wire and engines[0].graph_sizes()[0]:
        assert exchanges(engines) == EXCHANGES[B]
    for r, e in enumerate(engines):
        lo, hi = bounds[r], bounds[r + 1]
        if same_ids:
            assert np.array_equal(e.nodes()["alive"], want["alive"]), r
            assert np.array_equal(e.edges()["alive"], want["ealive"]), r
            c = e.counts()
            for key in ("n_nodes", "n_edges", "n_components", "n_live_nodes", "n_live_edges"):
                assert c[key] == want["counts"][key], (r, key)
            assert c["n_reads_to_correct"] == int(want["to_correct"][lo:hi].sum()), r
            assert np.array_equal(e.read_node_ids(), want["tok_node"][off[lo]:off[hi]]), r
        else:
            got = live_state(e)
            for key in ("tokens", "coverage", "first_dir", "src", "tgt", "sdir", "tdir", "ecov"):
                assert np.array_equal(got[key], want["live"][key]), (r, key)
            assert np.array_equal(got["tok_node"], want["live"]["tok_node"][off[lo]:off[hi]]), r
        assert np.array_equal(e.reads_to_correct(), want["to_correct"][lo:hi]), r
    assert dist.dist_remove_non_amr_nodes_loopback(engines, flags) == 0      # nothing is left to trim


# ------------------------------------------------------------------ 1. sharded == unsharded
@pytest.mark.parametrize("k", [3, 9])
@pytest.mark.parametrize("world", [1, 2, 3, 5])
def test_sharded_walks_equal_unsharded(world, k, key_mode, monkeypatch):
    from amira_amd.dist import dist_build_loopback
    if world == 1:
        monkeypatch.setenv("AMG_DIST_ALWAYS_EXCHANGE", "1")
    tokens, off, two_v, want = reference(k)
    bounds = even_bounds(len(off) - 1, world)
    engines = shard_engines(tokens, off, two_v, bounds, world_hook=world == 1)
    try:
        dist_build_loopback(engines, k)
        check_walks(engines, bounds, off, want)
    finally:
        close_all(engines)


@pytest.mark.parametrize("derive", [True, False])
def test_trim_correct_rebuild_equals_unsharded(derive, key_mode, monkeypatch):
    """trim across ranks -> every rank corrects its reads -> merged rebuild == unsharded trim -> correct -> build: the
    graph, and the corrected reads concatenated in rank order; with the rebuild derived from the trimmed graph where
    the ranks agree that it may be, and with AMG_NO_DERIVE=1"""
    from amira_amd.dist import dist_build_loopback, dist_remove_non_amr_nodes_loopback
    if not derive:
        monkeypatch.setenv("AMG_NO_DERIVE", "1")
    k, world = 3, 3
    tokens, off, two_v, want = reference(k)
    bounds = even_bounds(len(off) - 1, world)
    engines = shard_engines(tokens, off, two_v, bounds)
    gs, ge, rl = positions(off)
    try:
        for r, e in enumerate(engines):
            lo, hi = bounds[r], bounds[r + 1]
            e.set_positions(gs[off[lo]:off[hi]], ge[off[lo]:off[hi]], rl[lo:hi])
        dist_build_loopback(engines, k)
        assert dist_remove_non_amr_nodes_loopback(engines, want["flags"]) == want["B"]
        got = [e.corrected(*e.correct_reads(), True) for e in engines]
        for e in engines:
            e.adopt_corrected()
            e.dist_stats(reset=True)
        dist_build_loopback(engines, k)
        taken = [e.dist_stats()["derived_builds"] for e in engines]
        assert len(set(taken)) == 1 and (derive or taken[0] == 0)
        for e in engines:
            assert_same_graph(graph_state(e), want["rebuilt"])
        for key in ("tokens", "gene_start", "gene_end", "changed"):
            assert np.array_equal(np.concatenate([o[key] for o in got]), want["corrected"][key]), key
        lens = np.concatenate([np.diff(o["read_offsets"]) for o in got])
        assert np.array_equal(lens, np.diff(want["corrected"]["read_offsets"]))
        orig = np.concatenate([o["orig_read"] + bounds[r] for r, o in enumerate(got)])
        assert np.array_equal(orig, want["corrected"]["orig_read"])
    finally:
        close_all(engines)


# ------------------------------------------------------------------ 2. shapes where the fold can go wrong
def run_case(tokens, off, two_v, k, flags, bounds, after=None, thr=None):
    """loop-back walks on the shards `bounds` against the unsharded engine; after(e): removals made on every engine"""
    from amira_amd.dist import dist_build_loopback
    want = unsharded(tokens, off, two_v, k, flags, after=(lambda e: e.filter(*thr)) if thr else after)
    engines = shard_engines(tokens, off, two_v, bounds)
    try:
        dist_build_loopback(engines, k, *(thr or (1, 1)))
        if after is not None:
            for e in engines:
                after(e)
        check_walks(engines, bounds, off, want, on_wire=len(engines) > 1, same_ids=thr is None)
        return want, [e.nodes()["alive"] for e in engines], [e.read_node_ids() for e in engines]
    finally:
        close_all(engines)


def test_only_hit_read_on_another_rank(key_mode):
    """the one read with a gene of interest on rank 0, every other read of its nodes on rank 1: without the OR of the
    ranks' bitmaps rank 1 would kill them all"""
    k, V = 3, 200
    seq = V + np.arange(60, dtype=np.int32)
    rows = [seq[0:30]] + [seq[s:s + 18] for s in (3, 6, 9, 10)] + [seq[40:55], seq[42:60]]
    tokens, off = pack(rows)
    flags = flags_for(2 * V, [1])                       # gene 1: the second token of read 0 only
    want, alive, tok_node = run_case(tokens, off, 2 * V, k, flags, [0, 1, len(rows)])
    assert int(want["alive"].sum()) == 28 and want["B"] > 0          # read 0's 28 nodes stay, the far reads' go
    assert (tok_node[1][:16] >= 0).all()                # rank 1 keeps the windows it shares with rank 0's read


@pytest.mark.parametrize("D", [63, 64, 65, 100])
def test_node_counts_around_a_bitmap_word(D, key_mode):
    """D nodes: the keep bitmap has one word exactly filled, one bit short, one bit over; 100 is no multiple of 32.
    The gene of interest is the LAST gene of the last read: the last bit of the bitmap decides"""
    k, V = 3, 400
    seq = V + np.arange(D + k - 1, dtype=np.int32)
    h = D // 2
    rows = [seq[:h + k - 1], seq[h - 3:h + k + 2], seq[h:], seq[:7]]
    tokens, off = pack(rows)
    for gene in (D + k - 2, 0):
        flags = flags_for(2 * V, [gene])
        want, _, _ = run_case(tokens, off, 2 * V, k, flags, [0, 2, 4])
        assert len(want["alive"]) == D and int(want["alive"].sum()) + want["B"] == D and 0 < want["B"] < D


def test_rank_without_reads_and_rank_of_short_reads(key_mode):
    k = 3
    rng = np.random.default_rng(2)
    lengths = [1, 2, 2] + rng.choice([3, 5, 9, 20, 66], 40).tolist()
    tokens, off, two_v = genome_reads(77, lengths, ranks_per_genome=60, period=90)
    R = len(lengths)
    flags = some_flags(tokens, two_v, 5)[3]
    run_case(tokens, off, two_v, k, flags, [0, 0, 3, R // 2, R, R])   # ranks 0 and 4 hold nothing, rank 1 short reads only


def test_no_node_at_all(key_mode):
    """all reads shorter than k: D = 0, nothing to trim and no component — complete without a data exchange"""
    from amira_amd import dist
    k, V = 5, 50
    rows = [V + np.arange(n, dtype=np.int32) for n in (1, 2, 4, 3, 4, 0, 2)]
    tokens, off = pack(rows)
    engines = shard_engines(tokens, off, 2 * V, [0, 2, 5, 7])
    try:
        dist.dist_build_loopback(engines, k)
        for e in engines:
            e.dist_stats(reset=True)
        pairs, n_alive = dist.dist_depth_by_length_loopback(engines, [0, 3])
        assert pairs.tolist() == [0, 0] and n_alive == 0
        assert dist.dist_remove_non_amr_nodes_loopback(engines, np.ones(V, np.uint8)) == 0
        n_reads, n_long = dist.dist_component_amr_reads_loopback(engines, np.ones(V, np.uint8), 3)
        assert len(n_reads) == 0 and len(n_long) == 0
        assert [e.dist_stats()["exchanges"] for e in engines] == [3, 3, 3]     # the three header exchanges alone
    finally:
        close_all(engines)


def test_more_components_than_cache_slots_over_three_ranks():
    n, k = 3 * CACHE_SLOTS + 17, 3
    V = 5 * n
    rows = [V + 5 * r + np.arange(5, dtype=np.int32) for r in range(n)]
    rows += [rows[(j % 3) * CACHE_SLOTS + j // 3][:4] for j in range(96)]
    tokens, off = pack(rows)
    flags = np.ones(V, np.uint8)
    flags[5 * 7:5 * 8] = 0
    want, _, _ = run_case(tokens, off, 2 * V, k, flags, even_bounds(len(rows), 3))
    assert len(want["C"][0]) == n and want["C"][0][7] == 0 and int(want["C"][0].max()) == 2


def test_no_gene_of_interest():
    k = 3
    tokens, off, two_v, _ = reference(k)
    want, alive, _ = run_case(tokens, off, two_v, k, np.zeros(two_v // 2, np.uint8), even_bounds(len(off) - 1, 2))
    assert want["B"] > 0 and not alive[0].any() and not want["C"][0].any()


def test_after_a_fused_filter(key_mode):
    tokens, off, two_v = P_tokens()
    flags = some_flags(tokens, two_v, 1)[2]     # one gene of interest: the nodes no read through it reaches are trimmed
    want, _, _ = run_case(tokens, off, two_v, 5, flags, even_bounds(len(off) - 1, 3), thr=(3, 1))
    assert 0 < want["B"]


def test_after_tip_clipping(key_mode):
    tokens, off, two_v = P_tokens()
    flags = some_flags(tokens, two_v, 1)[2]     # one gene of interest: the nodes no read through it reaches are trimmed
    removed = []
    want, _, _ = run_case(tokens, off, two_v, 5, flags, even_bounds(len(off) - 1, 3),
                          after=lambda e: removed.append(len(e.remove_short_linear_paths(5))))
    assert removed[0] > 0 and len(set(removed)) == 1


_P = {}


def P_tokens():
    """noisy synthetic reads (low-coverage nodes for the filter, tips for the clip)"""
    if not _P:
        from amira_amd import tokenize
        reads, _, _ = P.synth_inputs(17, 300, 40, 150, 0.05)
        vocab, toks, offs, _ = tokenize(reads)
        _P["v"] = (toks, offs, vocab.two_v)
    return _P["v"]


# ------------------------------------------------------------------ 3. / 4. the host-driven transport
def all_gather_by_hand(engines, xs):
    """what a transport does with one exchange of every rank: device -> host, concatenate, host -> device"""
    assert all(x is not None and x.kind == 2 for x in xs)
    assert len({(x.elem_bytes, x.count) for x in xs}) == 1
    parts = [np.empty(int(x.count) * int(x.elem_bytes), np.uint8) for x in xs]
    for e, x, p in zip(engines, xs, parts):
        e.copy_d2h(x.send, p)
    everything = np.concatenate(parts)
    for e, x in zip(engines, xs):
        e.copy_h2d(x.recv, everything)


def drive(engines, which, flags=None, min_genes=None):
    """begin / next / result on every rank, the exchanges made here; returns the ranks' answers and the exchanges made"""
    for e in engines:
        e.dist_walk_begin(which, flags, min_genes)
    n = 0
    while True:
        xs = [e.dist_walk_next() for e in engines]
        if all(x is None for x in xs):
            return [e.dist_walk_result() for e in engines], n
        all_gather_by_hand(engines, xs)
        n += 1


def test_host_driven_transport():
    k, world = 3, 3
    tokens, off, two_v, want = reference(k)
    bounds = even_bounds(len(off) - 1, world)
    engines = shard_engines(tokens, off, two_v, bounds)
    try:
        for r, e in enumerate(engines):
            e.dist_init_external(r, world)
        from amira_amd.dist import dist_build_loopback
        dist_build_loopback(engines, k)
        wanted = {A: want["A"][0].tolist() + [want["A"][1]], Cc: want["C"][0].tolist() + want["C"][1].tolist(), B: [want["B"]]}
        for which, flags, mg in ((A, None, lengths_asked(k)), (Cc, want["flags"], [2 * k - 1]), (B, want["flags"], None)):
            for e in engines:
                e.dist_stats(reset=True)
            got, n = drive(engines, which, flags, mg)
            assert all(g.tolist() == wanted[which] for g in got), which
            assert n == EXCHANGES[which] and exchanges(engines) == EXCHANGES[which]
        for r, e in enumerate(engines):
            assert np.array_equal(e.nodes()["alive"], want["alive"])
            assert np.array_equal(e.read_node_ids(), want["tok_node"][off[bounds[r]]:off[bounds[r + 1]]])
    finally:
        close_all(engines)


def test_ranks_that_disagree_give_up_together():
    """another n on one rank, other gene flags, another walk: every rank's next call after the header exchange returns
    AMG_E_DIST, nobody asks for a second exchange, nothing was removed, and the next walk succeeds"""
    from amira_amd._ffi import AmgError
    from amira_amd.dist import dist_build_loopback
    k, world = 3, 3
    tokens, off, two_v, want = reference(k)
    flags = want["flags"]
    other = flags.copy()
    other[np.flatnonzero(flags == 0)[0]] = 1
    engines = shard_engines(tokens, off, two_v, even_bounds(len(off) - 1, world))
    try:
        dist_build_loopback(engines, k)
        before = [(e.nodes()["alive"], e.read_node_ids()) for e in engines]
        mg = lengths_asked(k)
        cases = [[(A, None, mg), (A, None, mg[:5]), (A, None, mg)],
                 [(B, flags, None), (B, other, None), (B, flags, None)],
                 [(Cc, flags, [5]), (Cc, other, [5]), (Cc, flags, [5])],
                 [(Cc, flags, [5]), (Cc, flags, [6]), (Cc, flags, [5])]]
        for case in cases:
            for e, (which, f, m) in zip(engines, case):
                e.dist_walk_begin(which, f, m)
            all_gather_by_hand(engines, [e.dist_walk_next() for e in engines])
            for e in engines:
                with pytest.raises(AmgError) as err:
                    e.dist_walk_next()
                assert err.value.code == E_DIST
        # A on one rank, C on the others: the first messages differ in size, which a transport notices itself; ranks
        # that were handed each other's headers all the same give up together
        for e, (which, f, m) in zip(engines, [(Cc, flags, [5]), (A, None, mg), (Cc, flags, [5])]):
            e.dist_walk_begin(which, f, m)
        xs = [e.dist_walk_next() for e in engines]
        assert [int(x.count) for x in xs] == [8, 24, 8]
        heads = []
        for e, x in zip(engines, xs):
            h = np.empty(8, np.int64)
            e.copy_d2h(x.send, h)
            heads.append(h)
        for e, x in zip(engines, xs):
            block = np.zeros((world, int(x.count)), np.int64)
            block[:, :8] = heads
            e.copy_h2d(x.recv, block)
        for e in engines:
            with pytest.raises(AmgError) as err:
                e.dist_walk_next()
            assert err.value.code == E_DIST
        for e, (alive, tok_node) in zip(engines, before):
            assert np.array_equal(e.nodes()["alive"], alive) and np.array_equal(e.read_node_ids(), tok_node)
        got, n = drive(engines, B, flags)
        assert [g.tolist() for g in got] == [[want["B"]]] * world and n == 2
    finally:
        close_all(engines)


# ------------------------------------------------------------------ 5. refusals
def test_refusals():
    from amira_amd import Engine, _ffi
    from amira_amd.dist import dist_build_loopback
    k = 3
    tokens, off, two_v = genome_reads(1, [10, 20, 30, 8, 8, 8])
    flags = np.ones(two_v // 2, np.uint8)
    plain = Engine(0)
    engines = shard_engines(tokens, off, two_v, [0, 3, 6])
    try:
        plain.set_reads(tokens, off, two_v)
        plain.build(k)
        for call in (lambda: plain.dist_walk_begin(A, None, [3]), lambda: Engine.dist_walk_local([plain], B, flags),
                     lambda: plain.dist_walk(Cc, flags, [5])):
            with pytest.raises(_ffi.AmgError) as err:
                call()
            assert err.value.code == E_STATE and "amg_" in str(err.value)     # it names the single-GPU call
        dist_build_loopback(engines, k)
        e = engines[0]
        for call in (lambda: e.depth_by_length([3]), lambda: e.remove_non_amr_nodes(flags),
                     lambda: e.component_amr_reads(flags, 5)):
            with pytest.raises(_ffi.AmgError) as err:
                call()
            assert err.value.code == E_STATE          # the single-GPU calls still refuse a shard's partial answer
        for mg in ([], list(range(17))):
            with pytest.raises(_ffi.AmgError) as err:
                Engine.dist_walk_local(engines, A, None, mg)
            assert err.value.code == E_ARG
        for which, f, m, n in ((A, None, None, 1), (B, None, None, 0), (Cc, flags, None, 1), (Cc, None, np.array([5], np.int32), 1),
                               (Cc, flags, np.array([5, 6], np.int32), 2), (7, flags, np.array([5], np.int32), 1)):
            assert _ffi.lib.amg_dist_walk_begin(e._h, which, _ffi.ptr(f), _ffi.ptr(m), n) == E_ARG
        with pytest.raises(_ffi.AmgError) as err:
            e.dist_walk_result()
        assert err.value.code == E_STATE              # nothing has been completed yet
        # a walk while a merge is begun, and a walk while a walk is under way
        e.dist_merge_begin(k)
        with pytest.raises(_ffi.AmgError) as err:
            e.dist_walk_begin(A, None, [3])
        assert err.value.code == E_STATE
        dist_build_loopback(engines, k)               # (begins anew on every rank)
        e.dist_walk_begin(A, None, [3])
        with pytest.raises(_ffi.AmgError) as err:
            e.dist_walk_begin(A, None, [3])
        assert err.value.code == E_STATE
        dist_build_loopback(engines, k)               # (a new build ends the walk nobody finished)
        # room too small for C: the size is reported, the room untouched
        n_comp = e.counts()["n_components"]
        assert n_comp >= 2
        handles = (C.c_void_p * 2)(*[x._h for x in engines])
        room, n_out = np.full(2 * n_comp, -7, np.int64), C.c_int64(-1)
        mg = np.array([5], np.int32)
        rc = _ffi.lib.amg_dist_walk_local(handles, 2, Cc, _ffi.ptr(flags), _ffi.ptr(mg), 1, _ffi.ptr(room), 2 * n_comp - 1,
                                          C.byref(n_out))
        assert rc == E_ARG and n_out.value == 2 * n_comp and (room == -7).all()
        rc = _ffi.lib.amg_dist_walk_local(handles, 2, Cc, _ffi.ptr(flags), _ffi.ptr(mg), 1, _ffi.ptr(room), 2 * n_comp,
                                          C.byref(n_out))
        assert rc == 0 and n_out.value == 2 * n_comp and (room >= 0).all()
        # the engines of another world, or out of rank order
        with pytest.raises(_ffi.AmgError) as err:
            Engine.dist_walk_local(engines[::-1], B, flags)
        assert err.value.code == E_ARG
        assert Engine.dist_walk_local(engines, B, flags).tolist() == [0]       # (every gene is of interest)
    finally:
        close_all(engines + [plain])


# ------------------------------------------------------------------ 6. RCCL
def test_walks_over_rccl_world1(monkeypatch):
    """amg_dist_walk: the exchanges as ncclAllGather on the engine's stream, through libamg's own communicator — at
    world 1 with every exchange forced through the transport, which is the only RCCL path a one-GPU box can run (two
    ranks over RCCL need two GPUs)"""
    from amira_amd import Engine, _ffi
    monkeypatch.setenv("AMG_DIST_ALWAYS_EXCHANGE", "1")
    k = 3
    tokens, off, two_v, want = reference(k)
    eng = Engine(0)
    try:
        eng.set_reads(tokens, off, two_v)
        eng.dist_init(Engine.dist_unique_id(), 0, 1)
        eng.dist_merge(k)
        eng.dist_stats(reset=True)
        got = eng.dist_walk(_ffi.WALK_DEPTH, None, lengths_asked(k))
        assert got.tolist() == want["A"][0].tolist() + [want["A"][1]] and eng.dist_stats()["exchanges"] == EXCHANGES[A]
        got = eng.dist_walk(_ffi.WALK_COMPONENT_READS, want["flags"], [2 * k - 1])
        assert got.tolist() == want["C"][0].tolist() + want["C"][1].tolist() and eng.dist_stats()["exchanges"] == EXCHANGES[Cc]
        got = eng.dist_walk(_ffi.WALK_AMR_TRIM, want["flags"])
        assert got.tolist() == [want["B"]] and eng.dist_stats()["exchanges"] == EXCHANGES[B]
        assert np.array_equal(eng.nodes()["alive"], want["alive"]) and np.array_equal(eng.read_node_ids(), want["tok_node"])
        assert np.array_equal(eng.reads_to_correct(), want["to_correct"])
        eng.dist_finalize()
    finally:
        eng.close()


# ------------------------------------------------------------------ 7. the drivers
GENES = [f"amr{j}" for j in range(4)]


def loopback_of(reads, world):
    """the engines of `world` emulated ranks holding the reads of a {read: genes} dict, and the flags of GENES"""
    from amira_amd import tokenize
    vocab, toks, offs, _ = tokenize(reads)
    flags = np.zeros(vocab.two_v // 2, np.uint8)
    for g in GENES:
        if vocab.rank.get(g) is not None:
            flags[vocab.rank[g]] = 1
    return shard_engines(toks, offs, vocab.two_v, even_bounds(len(offs) - 1, world)), flags


def test_driver_mean_node_coverages():
    import amira_amd
    from amira_amd import dist, graph_utils as gu
    reads, pos, _ = P.synth_inputs(3, 300, 30, 300, 0.03, n_amr=4)
    whole = {f"r{i}": ["+a", "+b", "+c", "+d"] for i in range(6)}       # means that are whole numbers: ints
    for rd, ps, k in ((reads, pos, 3), (reads, pos, 5), (whole, None, 3)):
        g = amira_amd.GeneMerGraph(dict(rd), k, dict(ps) if ps else None)
        want = gu.get_overall_mean_node_coverages(g)
        g.close()
        engines, _ = loopback_of(rd, 3)
        try:
            dist.dist_build_loopback(engines, k)
            got = dist.dist_mean_node_coverages_loopback(engines)
        finally:
            close_all(engines)
        assert got == want and {k_: type(v) for k_, v in got.items()} == {k_: type(v) for k_, v in want.items()}
    assert type(got[3]) is int and got[3] == 6


def ragged_reads(keep):
    """the long synthetic reads of test_drop_in_choose_kmer_size_beyond_k5, cut to ragged lengths"""
    reads, pos, _ = P.synth_inputs(41, 90, 44, 120, 0.002, n_amr=4)
    for i, r in enumerate(list(reads)):
        n = keep[i % len(keep)]
        reads[r], pos[r] = reads[r][:n], pos[r][:n]
    return reads, pos


@pytest.mark.parametrize("case", ["drop_in", "beyond_5", "beyond_7"])
def test_driver_choose_kmer_size(case):
    from amira_amd import dist, graph_utils as gu
    if case == "drop_in":
        reads, pos, _ = P.synth_inputs(3, 300, 30, 300, 0.03, n_amr=4)
    else:
        reads, pos = ragged_reads({"beyond_5": [40, 36, 30, 24, 18, 14, 13, 13, 13, 10],
                                   "beyond_7": [44, 40, 36, 33, 31, 30, 29, 29, 29, 12]}[case])
    want = gu.choose_kmer_size(25, reads, 1, pos, GENES)
    assert case == "drop_in" or want >= (7 if case == "beyond_5" else 9)
    engines, flags = loopback_of(reads, 3)
    try:
        assert dist.dist_choose_kmer_size_loopback(engines, 25, flags) == want
        assert want <= engines[0].graph_sizes()[2] <= want + 2       # left with the last graph tried
    finally:
        close_all(engines)


def test_driver_choose_kmer_size_at_low_coverage(monkeypatch):
    """a mean coverage below 20: the answer is 3 and no graph is built"""
    from amira_amd import dist, graph_utils as gu
    reads, pos, _ = P.synth_inputs(3, 300, 30, 300, 0.03, n_amr=4)
    engines, flags = loopback_of(reads, 2)
    try:
        built = []
        monkeypatch.setattr(dist, "dist_build_loopback", lambda *a, **kw: built.append(a))
        assert dist.dist_choose_kmer_size_loopback(engines, 19.5, flags) == 3 == gu.choose_kmer_size(19.5, reads, 1, pos, GENES)
        assert built == []
    finally:
        close_all(engines)
