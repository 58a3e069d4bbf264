"""GPU: amg_select_reads (amira_amd/csrc/amg_select.hip) — get_valid_reads_only and remove_junk_reads as selections of
whole reads that stay on the device as a corrected set in which nothing changed — and the two GeneMerGraph methods on
top of it.  Expected values come from tests/select_oracle.py on what amg_get_read_nodes / amg_get_reads_to_correct
return and from the pure-Python amira_oracle's graphs, never from the call under test.  Integer equality throughout."""
import os
import pickle

import numpy as np
import pytest

import select_oracle as S

pytestmark = pytest.mark.gpu

E_ARG, E_STATE = -2, -3
K = S.CASE_K


# ------------------------------------------------------------------ the named case, once
@pytest.fixture(scope="module")
def case():
    from amira_amd.tokens import tokenize
    reads, pos, fq = S.named_case()
    vocab, toks, offs, ids = tokenize(reads)
    gs = np.asarray([p[0] for r in ids for p in pos[r]], np.int64)
    ge = np.asarray([p[1] for r in ids for p in pos[r]], np.int64)
    rl = np.asarray([len(fq[r]["sequence"]) for r in ids], np.int64)
    return {"reads": reads, "pos": pos, "fq": fq, "vocab": vocab, "toks": toks, "offs": offs, "ids": ids, "gs": gs,
            "ge": ge, "rl": rl}


@pytest.fixture(scope="module")
def oracle_graph(case):
    """the oracle's graph of the case after filter_graph(3, 1): read only"""
    from amira_oracle import GeneMerGraph
    g = GeneMerGraph(dict(case["reads"]), K, {r: list(v) for r, v in case["pos"].items()})
    g.filter_graph(3, 1)
    return g


@pytest.fixture(scope="module")
def eng():
    from amira_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def load(e, c, n=None, pos="i64", k=K, thr=(3, 1)):
    """the first n reads of the case on the engine, built and filtered; returns (tokens, offsets, gene starts, ends)"""
    n = len(c["ids"]) if n is None else n
    offs = c["offs"][:n + 1]
    T = int(offs[-1])
    toks, gs, ge = c["toks"][:T], c["gs"][:T], c["ge"][:T]
    e.set_reads(toks, offs, c["vocab"].two_v)
    if pos == "i64":
        e.set_positions(gs, ge, c["rl"][:n])
    elif pos == "i32":
        e.set_positions(gs.astype(np.int32), ge.astype(np.int32), c["rl"][:n])
    e.build(k)
    e.filter(*thr)
    return toks, offs, (gs if pos else None), (ge if pos else None)


def check_selection(e, toks, offs, gs, ge, mode, invert, table, k=K, pos_off=None, pool0=True):
    """one call against select_oracle on the engine's own per-window ids and flags: verdicts, sizes, and the set read
    back through amg_get_corrected and (with positions) amg_get_corrected32"""
    tok_node, fix = e.read_node_ids(), e.reads_to_correct()
    want = S.select(toks, offs, k, tok_node, fix, mode, invert, table, gs, ge, pos_off)
    verdict, n_reads, n_tokens = e.select_reads(mode, invert, table)
    assert np.array_equal(verdict, want["verdict"])
    assert (n_reads, n_tokens) == (want["n_reads"], want["n_tokens"])
    out = e.corrected(n_reads, n_tokens, gs is not None)
    assert np.array_equal(out["read_offsets"], want["read_offsets"]) and np.array_equal(out["tokens"], want["tokens"])
    assert np.array_equal(out["orig_read"], want["rows"]) and not out["changed"].any()
    assert n_reads < 2 or (np.diff(out["orig_read"]) > 0).all()
    if gs is not None:
        assert np.array_equal(out["gene_start"], want["gene_start"]) and np.array_equal(out["gene_end"], want["gene_end"])
        out32 = e.corrected32(n_reads, n_tokens)
        for key in ("tokens", "read_offsets", "orig_read", "changed"):
            assert np.array_equal(out32[key], out[key]), key
        if pool0:   # the caller's own arrays: nothing new travels, every read says where its positions begin
            # (a read without a gene has no position in any array: amg_get_corrected32 may say either of it — one that
            # ends the read set begins where the caller's arrays end)
            some = np.diff(out["read_offsets"]) > 0
            assert (out32["pos_src"][some] >= 0).all() and len(out32["new_start"]) == 0
            assert np.array_equal(out32["pos_src"][some], want["pos_src"][some])
    return want


def tables(offs, k=K):
    longest = int(S.windows(offs, k).max()) if len(offs) > 1 else 0
    return {rate: S.allowed_table(rate, longest) for rate in S.CASE_RATES}


# ------------------------------------------------------------------ 1. verdicts and the set
@pytest.mark.parametrize("pos", ["i64", "i32", None])
def test_verdicts_and_the_set(eng, case, oracle_graph, pos):
    toks, offs, gs, ge = load(eng, case, pos=pos)
    # the engine's graph is the oracle's: the listed reads and the reads to correct are those the CPU test pins
    assert int(eng.reads_to_correct().sum()) == len(oracle_graph.get_reads_to_correct()) == 235
    sizes = {}
    for invert in (0, 1):
        check_selection(eng, toks, offs, gs, ge, S.VALID, invert, None)
        for rate, table in tables(offs).items():
            want = check_selection(eng, toks, offs, gs, ge, S.JUNK, invert, table)
            sizes[rate, invert] = want["n_reads"]
    assert {rate: (sizes[rate, 0], sizes[rate, 1]) for rate in S.CASE_RATES} == S.CASE_WANT


# ------------------------------------------------------------------ 2. wave and block boundaries
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_wave_and_block_boundaries(eng, case, n):
    toks, offs, gs, ge = load(eng, case, n=n)
    table = tables(offs)[0.8]
    for invert in (0, 1):
        check_selection(eng, toks, offs, gs, ge, S.VALID, invert, None)
        check_selection(eng, toks, offs, gs, ge, S.JUNK, invert, table)


# ------------------------------------------------------------------ 3. forced boundaries with crafted tables
def test_crafted_tables(eng, case):
    from amira_amd._ffi import AmgError
    toks, offs, gs, ge = load(eng, case)
    w = S.windows(offs, K)
    m = S.masked_windows(offs, K, eng.read_node_ids())
    longest = int(w.max())
    at_most = np.zeros(longest + 1, np.int64)
    np.maximum.at(at_most, w, m)
    listed = int((w > 0).sum())
    # allowed[w] = the most masked windows a read of w windows has: every listed read is kept
    want = check_selection(eng, toks, offs, gs, ge, S.JUNK, 0, at_most.tolist())
    assert want["n_reads"] == listed == 342
    # one less: exactly the reads at the maximum are rejected
    want = check_selection(eng, toks, offs, gs, ge, S.JUNK, 1, (at_most - 1).tolist())
    assert np.array_equal(want["rows"], np.flatnonzero((w > 0) & (m == at_most[w]))) and 0 < want["n_reads"] < listed
    # a table of -1 keeps none
    want = check_selection(eng, toks, offs, gs, ge, S.JUNK, 0, [-1] * (longest + 1))
    assert want["n_reads"] == 0 and int((want["verdict"] == S.REJECTED).sum()) == listed
    # n_allowed = longest windows + 1 is accepted (above), one smaller is refused and leaves no corrected set
    with pytest.raises(AmgError) as err:
        eng.select_reads(S.JUNK, False, at_most[:longest].tolist())
    assert err.value.code == E_ARG
    with pytest.raises(AmgError) as err:
        eng.corrected_index(0)
    assert err.value.code == E_STATE and "amg_select_reads" in str(err.value) and "amg_correct_reads" in str(err.value)
    # bad arguments: a mode out of range, JUNK without a table
    for args in ((2, False, at_most.tolist()), (-1, False, None), (S.JUNK, False, None), (S.JUNK, True, [])):
        with pytest.raises(AmgError) as err:
            eng.select_reads(*args)
        assert err.value.code == E_ARG
    check_selection(eng, toks, offs, gs, ge, S.VALID, 0, None)   # and the engine goes on


# ------------------------------------------------------------------ 4. extremes
def test_empty_and_full_sets(eng, case):
    toks, offs, gs, ge = load(eng, case)
    longest = int(S.windows(offs, K).max())
    none = check_selection(eng, toks, offs, gs, ge, S.JUNK, 0, [-1] * (longest + 1))
    full = check_selection(eng, toks, offs, gs, ge, S.JUNK, 0, [1 << 40] * (longest + 1))
    assert none["n_reads"] == 0 and none["n_tokens"] == 0 and full["n_reads"] == 342
    assert check_selection(eng, toks, offs, gs, ge, S.JUNK, 1, [1 << 40] * (longest + 1))["n_reads"] == 0
    # VALID on a graph nothing was removed from: every read, the short ones and the empty ones included
    load(eng, case, thr=(1, 1))
    assert not eng.reads_to_correct().any()
    every = check_selection(eng, toks, offs, gs, ge, S.VALID, 0, None)
    assert every["n_reads"] == len(offs) - 1 and every["n_tokens"] == int(offs[-1])
    assert check_selection(eng, toks, offs, gs, ge, S.VALID, 1, None)["n_reads"] == 0


def test_a_read_set_of_zero_reads(eng, case):
    toks, offs = np.zeros(0, np.int32), np.zeros(1, np.int64)
    eng.set_reads(toks, offs, case["vocab"].two_v)
    eng.build(K)
    for mode, table in ((S.VALID, None), (S.JUNK, [0])):
        for invert in (0, 1):
            want = check_selection(eng, toks, offs, None, None, mode, invert, table)
            assert want["n_reads"] == 0 and want["n_tokens"] == 0


def test_a_read_without_genes_survives_valid(case):
    from amira_amd import GeneMerGraph
    from amira_amd.io import TokenizedReads
    g = GeneMerGraph(TokenizedReads(case["vocab"], case["toks"], case["offs"], case["ids"]), K)
    g.filter_graph(3, 1)
    valid = g.get_valid_reads_only()
    assert isinstance(valid, TokenizedReads) and valid.device_source() is not None
    empty = [r for r in case["ids"] if len(case["reads"][r]) == 0]
    assert len(empty) > 0 and all(r in valid and valid[r] == [] for r in empty)
    g.close()


# ------------------------------------------------------------------ 5. pools
def _tokenized(c):
    from amira_amd.io import ReadLengths, TokenizedPositions, TokenizedReads
    return (TokenizedReads(c["vocab"], c["toks"], c["offs"], c["ids"]),
            TokenizedPositions(c["ids"], c["offs"], c["gs"], c["ge"]), ReadLengths(c["ids"], c["rl"]))


def _same_mappings(got_reads, got_pos, want_reads, want_pos):
    assert list(got_reads) == list(want_reads)
    for r in want_reads:
        assert got_reads[r] == list(want_reads[r]), r
        assert [tuple(p) for p in got_pos[r]] == [tuple(p) for p in want_pos[r]], r


def test_selection_after_a_correction(case):
    """reads whose positions lie in the pool of produced positions (re-threaded) and at an offset of the caller's
    arrays (trimmed) go through a second graph, its filter and remove_junk_reads like the oracle's dicts"""
    from amira_amd import GeneMerGraph
    from amira_oracle import GeneMerGraph as Oracle
    reads, pos = case["reads"], case["pos"]
    o1 = Oracle(dict(reads), K, {r: list(v) for r, v in pos.items()})
    o1.filter_graph(3, 1)
    r_o, p_o = o1.correct_reads(case["fq"])
    changed = [r for r in r_o if list(r_o[r]) != list(reads[r])]
    is_slice = lambda a, b: any(b[i:i + len(a)] == a for i in range(len(b) - len(a) + 1))
    trimmed = [r for r in changed if len(r_o[r]) < len(reads[r]) and is_slice(list(r_o[r]), list(reads[r]))]
    assert len(trimmed) > 0 and len(changed) > len(trimmed)   # at least one trimmed and one re-threaded read
    treads, tpos, tlen = _tokenized(case)
    g1 = GeneMerGraph(treads, K, tpos)
    g1.filter_graph(3, 1)
    r_t, p_t = g1.correct_reads(tlen)
    g2, o2 = GeneMerGraph(r_t, K, p_t), Oracle(dict(r_o), K, {r: list(v) for r, v in p_o.items()})
    assert r_t.device_source() is not None    # taken over on the device
    g2.filter_graph(3, 1)
    o2.filter_graph(3, 1)
    got, want = g2.remove_junk_reads(0.8), o2.remove_junk_reads(0.8)
    assert len(want[0]) > 0
    _same_mappings(got[0], got[1], want[0], want[1])
    _same_mappings(got[2], got[3], want[2], want[3])
    for g in (g1, g2):
        g.close()


def test_selection_on_adopted_reads(eng, case):
    """the same on ONE engine: after amg_adopt_corrected the reads' positions are offsets into two pools"""
    toks, offs, gs, ge = load(eng, case)
    n_reads, n_tokens = eng.correct_reads()
    first = eng.corrected(n_reads, n_tokens, True)
    assert first["changed"].any()
    eng.adopt_corrected()
    eng.build(K)
    eng.filter(3, 1)
    toks2, offs2 = first["tokens"], first["read_offsets"]
    for mode, table in ((S.VALID, None), (S.JUNK, tables(offs2)[0.8]), (S.JUNK, tables(offs2)[0.5])):
        for invert in (0, 1):
            check_selection(eng, toks2, offs2, first["gene_start"], first["gene_end"], mode, invert, table, pool0=False)


# ------------------------------------------------------------------ 6. hand-over
def graph_state(e):
    n, ed = e.nodes(), e.edges()
    tn, td = e.read_nodes()
    out = {"n_" + key: v for key, v in n.items()}
    out.update({"e_" + key: v for key, v in ed.items()})
    out.update(tok_node=tn, tok_dir=np.where(tn >= 0, td, 0))
    return out


def _same_graph(g, o):
    assert list(g.get_nodes()) == list(o.get_nodes())
    assert [(h, e.get_edge_coverage()) for h, e in g.get_edges().items()] == \
           [(h, e.get_edge_coverage()) for h, e in o.get_edges().items()]
    assert {r: list(v) for r, v in g.get_readNodes().items()} == {r: list(v) for r, v in o.get_readNodes().items()}


def test_the_kept_reads_go_to_the_next_graph_on_the_device(case, oracle_graph):
    from amira_amd import GeneMerGraph
    from amira_oracle import GeneMerGraph as Oracle
    treads, tpos, _ = _tokenized(case)
    g = GeneMerGraph(treads, K, tpos)
    g.filter_graph(3, 1)
    kept, kept_pos, rejected, rejected_pos = g.remove_junk_reads(0.8)
    want = oracle_graph.remove_junk_reads(0.8)
    assert kept.device_source() is not None and kept_pos.device_source() is kept.device_source()
    assert rejected.device_source() is None and list(rejected) == list(want[2])
    g2 = GeneMerGraph(kept, K, kept_pos)
    assert kept.device_source() is not None            # no gene and no position crossed PCIe for the rebuild
    assert g2._engine.counts()["derived"] == 0
    o2 = Oracle(dict(want[0]), K, {r: list(v) for r, v in want[1].items()})
    _same_graph(g2, o2)
    _same_mappings(kept, kept_pos, want[0], want[1])    # (fetched now)
    _same_mappings(rejected, rejected_pos, want[2], want[3])
    # ... and the valid reads
    valid = g.get_valid_reads_only()
    want_valid = oracle_graph.get_valid_reads_only()
    assert valid.device_source() is not None
    g3 = GeneMerGraph(valid, K)   # (the graph's short-read annotations then read the genes on the host)
    assert g3._engine.counts()["derived"] == 0
    _same_graph(g3, Oracle(dict(want_valid), K))
    assert list(valid) == list(want_valid) and all(valid[r] == list(want_valid[r]) for r in want_valid)
    for x in (g, g2, g3):
        x.close()


@pytest.mark.parametrize("mode,rate", [(S.JUNK, 0.8), (S.JUNK, 0.0), (S.VALID, None)])
def test_adopting_a_selection_is_never_a_derived_rebuild(eng, case, mode, rate):
    """rejected reads take live coverage away and kept ones bring their masked windows back: the graph of the set is
    not the live part of the graph at hand"""
    from amira_amd import Engine
    toks, offs, gs, ge = load(eng, case)
    table = None if rate is None else tables(offs)[rate]
    want = check_selection(eng, toks, offs, gs, ge, mode, 0, table)
    eng.adopt_corrected()
    eng.build(K)
    c = eng.counts()
    assert c["derived"] == 0
    assert (c["n_reads"], c["n_tokens"]) == (want["n_reads"], want["n_tokens"])
    fresh = Engine(0)
    try:
        fresh.set_reads(want["tokens"], want["read_offsets"], case["vocab"].two_v)
        fresh.build(K)
        a, b = graph_state(eng), graph_state(fresh)
        assert a.keys() == b.keys()
        for key in a:
            assert np.array_equal(a[key], b[key]), key
    finally:
        fresh.close()
    # the adopted reads kept their positions: a selection of everything hands them back
    out = eng.corrected(*eng.select_reads(S.JUNK, False, [1 << 40] * (len(tables(offs)[0.8])))[1:], True)
    short = S.windows(want["read_offsets"], K) == 0
    listed = np.repeat(~short, np.diff(want["read_offsets"]))
    assert np.array_equal(out["gene_start"], want["gene_start"][listed])
    assert np.array_equal(out["gene_end"], want["gene_end"][listed])


# ------------------------------------------------------------------ 7. sweep
def test_cleaning_sweep_on_the_kept_reads(case):
    """read lengths and source rows were carried: a ReadLengths of the ORIGINAL reads serves the sweep of the kept ones"""
    from amira_amd import GeneMerGraph
    from amira_amd import graph_utils as gu
    treads, tpos, tlen = _tokenized(case)
    g = GeneMerGraph(treads, K, tpos)
    g.filter_graph(3, 1)
    kept, kept_pos, _, _ = g.remove_junk_reads(0.8)
    assert kept.source_ids is treads.read_ids and np.array_equal(np.asarray(treads.read_ids, object)[kept.source_rows],
                                                                 np.asarray(kept.read_ids, object))
    gd = GeneMerGraph(dict(case["reads"]), K, {r: list(v) for r, v in case["pos"].items()})
    gd.filter_graph(3, 1)
    kept_d, kept_pos_d, _, _ = gd.remove_junk_reads(0.8)
    g_t, r_t, p_t = gu.cleaning_sweep(kept, kept_pos, K, tlen, 3)
    g_d, r_d, p_d = gu.cleaning_sweep(kept_d, kept_pos_d, K, case["fq"], 3)
    _same_mappings(r_t, p_t, r_d, p_d)
    _same_graph(g_t, g_d)
    for x in (g, gd, g_t, g_d):
        x.close()


# ------------------------------------------------------------------ 8. order of events
def test_earlier_mappings_keep_answering(case, oracle_graph):
    from amira_amd import GeneMerGraph
    treads, tpos, _ = _tokenized(case)
    g = GeneMerGraph(treads, K, tpos)
    g.filter_graph(3, 1)
    want_junk, want_valid = oracle_graph.remove_junk_reads(0.8), oracle_graph.get_valid_reads_only()
    kept, kept_pos, _, _ = g.remove_junk_reads(0.8)
    assert kept.device_source() is not None
    log = list(g._pass_log)
    valid = g.get_valid_reads_only()             # overwrites the engine's corrected set: the kept reads come to the host
    assert kept.device_source() is None and valid.device_source() is not None
    _same_mappings(kept, kept_pos, want_junk[0], want_junk[1])
    g.filter_graph(4, 1)                          # a pass that changes the graph settles the lease as well
    assert valid.device_source() is None
    assert list(valid) == list(want_valid) and all(valid[r] == list(want_valid[r]) for r in want_valid)
    _same_mappings(kept, kept_pos, want_junk[0], want_junk[1])
    assert g._pass_log == log + [("filter", (4, 1))]   # a selection is not logged: it does not change the graph
    g.close()


def test_kept_mappings_round_trip_through_pickle(case, oracle_graph):
    from amira_amd import GeneMerGraph
    treads, tpos, _ = _tokenized(case)
    g = GeneMerGraph(treads, K, tpos)
    g.filter_graph(3, 1)
    kept, kept_pos, _, _ = g.remove_junk_reads(0.75)
    want = oracle_graph.remove_junk_reads(0.75)
    kept2, kept_pos2 = pickle.loads(pickle.dumps((kept, kept_pos)))
    _same_mappings(kept2, kept_pos2, want[0], want[1])
    _same_mappings(kept, kept_pos, want[0], want[1])
    g.close()


# ------------------------------------------------------------------ 9. fingerprint keys
def test_gene_mer_size_eleven(eng, case):
    toks, offs, gs, ge = load(eng, case, k=11, thr=(2, 1))
    assert eng.counts()["k"] == 11
    m = S.masked_windows(offs, 11, eng.read_node_ids())
    assert m.sum() > 0
    table = S.allowed_table(0.8, int(S.windows(offs, 11).max()))
    for invert in (0, 1):
        check_selection(eng, toks, offs, gs, ge, S.VALID, invert, None, k=11)
        want = check_selection(eng, toks, offs, gs, ge, S.JUNK, invert, table, k=11)
        assert want["n_reads"] > 0


# ------------------------------------------------------------------ 10. merged graph
def test_every_rank_of_a_merged_graph_selects_its_own_reads(eng, case):
    from amira_amd import Engine
    from amira_amd.dist import dist_build_loopback
    toks, offs, gs, ge = load(eng, case)
    table = tables(offs)[0.8]
    single = {(mode, invert): eng.select_reads(mode, invert, t)[0]
              for mode, t in ((S.VALID, None), (S.JUNK, table)) for invert in (0, 1)}
    R = len(offs) - 1
    bounds = [0, R // 2 + 3, R]
    ranks = []
    try:
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            e = Engine(0)
            e.set_reads(toks[offs[lo]:offs[hi]], offs[lo:hi + 1] - offs[lo], case["vocab"].two_v)
            e.set_positions(gs[offs[lo]:offs[hi]], ge[offs[lo]:offs[hi]], case["rl"][lo:hi])
            ranks.append(e)
        dist_build_loopback(ranks, K)
        for e in ranks:
            e.filter(3, 1)
        for (lo, hi), e in zip(zip(bounds[:-1], bounds[1:]), ranks):
            t, o = toks[offs[lo]:offs[hi]], offs[lo:hi + 1] - offs[lo]
            for (mode, invert), v in single.items():
                want = check_selection(e, t, o, gs[offs[lo]:offs[hi]], ge[offs[lo]:offs[hi]], mode, invert,
                                       table if mode == S.JUNK else None)
                assert np.array_equal(want["verdict"], v[lo:hi]), (mode, invert, lo)
    finally:
        for e in ranks:
            e.close()


# ------------------------------------------------------------------ 11. ABI
def test_the_symbol_is_exported():
    import ctypes
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = ctypes.CDLL(os.path.join(root, "amira_amd", "libamg.so"))
    assert hasattr(lib, "amg_select_reads")
    from amira_amd import _ffi
    assert "amg_select_reads" in _ffi.SYMBOLS
    assert (_ffi.SELECT_VALID, _ffi.SELECT_JUNK) == (S.VALID, S.JUNK)
    assert (_ffi.SEL_REJECTED, _ffi.SEL_KEPT, _ffi.SEL_UNLISTED) == (S.REJECTED, S.KEPT, S.UNLISTED)
