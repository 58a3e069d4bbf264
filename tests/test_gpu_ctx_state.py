"""What a context holds after each event that changes it (amg_state.h: one transition per event), through the ABI on the
smallest graphs that have the features: the constructed read sets of tests/derive_cases.py at k = 3, with positions.

  a  the corrected set is dropped by every removing call that has passed its argument checks (also one that removes
     nothing) and by every call that replaces reads or positions; an empty removal list keeps it
  b  new reads leave no graph
  c  the derived rebuild is offered once, to a build at the same k of the reads the adoption left
  d  reads handed to a second context, and amg_build_multi over contexts that held something

What tests/test_gpu_derive.py (verdicts per case class, another k, AMG_NO_DERIVE), tests/test_gpu_match.py (the cached
search result under the same events) and tests/test_gpu_select.py (a refused selection leaves no set) assert is not
repeated here.  No oracle graph is made: every expectation is a return code, a flag of amg_counts or the state of a twin
engine that went the plain way."""
import numpy as np
import pytest

import derive_cases as DC
from test_gpu_derive import graph_state, same_state

pytestmark = pytest.mark.gpu

E_STATE = -3


@pytest.fixture(scope="module")
def engines():
    from amira_amd import Engine
    es = [Engine(0) for _ in range(4)]
    yield es
    for e in es:
        e.close()


@pytest.fixture(scope="module")
def eng(engines):
    return engines[0]


_INPUTS = {}


def inputs(name):
    """(k, procedure, vocabulary, tokens, offsets, starts, ends, read lengths) of a case, made once and not changed"""
    if name not in _INPUTS:
        reads, k, procedure, _, _ = DC.case(name)
        vocab, toks, offs, _, gs, ge, rl, _, _ = DC.inputs(reads)
        _INPUTS[name] = (k, procedure, vocab, toks, offs, gs, ge, rl)
    return _INPUTS[name]


def load(e, name, positions=True, lengths=True):
    k, _, vocab, toks, offs, gs, ge, rl = inputs(name)
    e.set_reads(toks, offs, vocab.two_v)
    if positions:
        e.set_positions(gs, ge, rl if lengths else None)
    return k


def corrected(e, name="both_ends_cut", **kw):
    """build, the case's removals, correct: returns (k, (reads, genes) of the corrected set)"""
    k = load(e, name, **kw)
    e.build(k)
    for step in inputs(name)[1]:
        {"filter": e.filter, "clip": e.remove_short_linear_paths}[step[0]](*step[1:])
    return k, e.correct_reads()


def set_code(e, n):
    """0 while the corrected set of n = (reads, genes) can be fetched, else the code amg_get_corrected answers"""
    from amira_amd._ffi import AmgError
    try:
        e.corrected_index(n[0])
    except AmgError as err:
        return err.code
    return 0


# ------------------------------------------------------------------ a. who drops the corrected set
def clip_nothing(e, k):
    for _ in range(8):                      # (a clip can make new tips: until one finds none)
        if e.remove_short_linear_paths(k, want_ids=False) == 0:
            break
    n = e.correct_reads()
    assert set_code(e, n) == 0
    assert e.remove_short_linear_paths(k, want_ids=False) == 0
    return n


REMOVALS = {"filter": lambda e, k: e.filter(2, 1),
            "remove_nodes": lambda e, k: e.remove_nodes([0]),
            "remove_edges": lambda e, k: e.remove_edges([0]),
            "clip_that_removes_nothing": None,
            "low_components": lambda e, k: e.remove_low_coverage_components(1),
            "read_walk_trim": lambda e, k: e.remove_non_amr_nodes(
                np.ones(inputs("both_ends_cut")[2].two_v // 2, np.uint8))}       # (every gene is of interest)


@pytest.mark.parametrize("what", sorted(REMOVALS))
def test_a_removal_drops_the_corrected_set(eng, what):
    k, n = corrected(eng)
    assert set_code(eng, n) == 0
    if what == "clip_that_removes_nothing":
        n = clip_nothing(eng, k)
    else:
        REMOVALS[what](eng, k)
    assert set_code(eng, n) == E_STATE


def test_an_empty_removal_list_keeps_the_corrected_set(eng):
    _, n = corrected(eng)
    eng.remove_nodes([])
    eng.remove_edges([])
    assert set_code(eng, n) == 0


@pytest.mark.parametrize("what", ["set_reads", "set_positions", "set_positions32"])
def test_new_inputs_drop_the_corrected_set(eng, what):
    _, n = corrected(eng)
    _, _, vocab, toks, offs, gs, ge, rl = inputs("both_ends_cut")
    if what == "set_reads":
        eng.set_reads(toks, offs, vocab.two_v)
    elif what == "set_positions":
        eng.set_positions(gs, ge, rl)
    else:
        eng.set_positions(gs.astype(np.int32), ge.astype(np.int32), rl)
    assert set_code(eng, n) == E_STATE


# ------------------------------------------------------------------ b. new reads leave no graph
def test_new_reads_leave_no_graph(eng):
    from amira_amd._ffi import AmgError
    k = load(eng, "identity")
    eng.build(k)
    assert eng.graph_sizes()[2] == k
    load(eng, "identity", positions=False)
    with pytest.raises(AmgError) as err:
        eng.graph_sizes()
    assert err.value.code == E_STATE
    assert eng.counts()["n_nodes"] == 0


# ------------------------------------------------------------------ c. the derived rebuild is offered once
def adopted(e, name="both_ends_cut", before=None):
    """build, the case's removals, correct, adopt: returns (k, tokens, offsets of the reads the context now holds)"""
    k = load(e, name)
    e.build(k)
    if before:
        before(e)
    for step in inputs(name)[1]:
        {"filter": e.filter, "clip": e.remove_short_linear_paths}[step[0]](*step[1:])
    n = e.correct_reads()
    out = e.corrected(*n, False)
    e.adopt_corrected()
    assert e.sizes() == n
    return k, out["tokens"], out["read_offsets"]


@pytest.mark.parametrize("how", ["same_k", "other_k", "no_derive", "edge_removed_before", "set_reads_in_between"])
def test_who_gets_the_derived_rebuild(engines, monkeypatch, how):
    eng, twin = engines[0], engines[1]
    if how == "no_derive":
        monkeypatch.setenv("AMG_NO_DERIVE", "1")
    k, toks, offs = adopted(eng, before=(lambda e: e.remove_edges([0])) if how == "edge_removed_before" else None)
    two_v = inputs("both_ends_cut")[2].two_v
    k2 = k + 2 if how == "other_k" else k
    if how == "set_reads_in_between":
        # the very arrays the adoption left, handed in from outside: the engine cannot know that they are
        eng.set_reads(toks, offs, two_v)
    eng.build(k2)
    c = eng.counts()
    assert c["derived"] == (1 if how == "same_k" else 0) and c["k"] == k2
    # whichever way: the graph of the adopted reads, as a twin builds it from the reads alone
    twin.set_reads(toks, offs, two_v)
    twin.build(k2)
    assert twin.counts()["derived"] == 0
    same_state(graph_state(eng), graph_state(twin), how)
    eng.build(k2)                             # the offer is used up
    assert eng.counts()["derived"] == 0
    same_state(graph_state(eng), graph_state(twin), how)


# ------------------------------------------------------------------ d. reads handed on; several graphs at once
@pytest.mark.parametrize("positions,lengths", [(True, True), (True, False), (False, False)])
def test_reads_from_another_contexts_correction(engines, positions, lengths):
    from amira_amd import _ffi
    src, dst, twin = engines[0], engines[1], engines[2]
    k = load(dst, "identity")
    dst.build(k)
    dst.filter(1, 1)
    n_dst = dst.correct_reads()             # dst holds a graph and a corrected set of its own
    _, n = corrected(src, positions=positions, lengths=lengths)
    want = src.corrected(*n, positions)
    dst.set_reads_from_corrected(src)
    assert dst.sizes() == n
    assert dst.counts()["n_nodes"] == 0     # not built
    with pytest.raises(_ffi.AmgError) as err:
        dst.graph_sizes()
    assert err.value.code == E_STATE
    assert set_code(dst, n_dst) == E_STATE
    assert set_code(src, n) == 0            # the source keeps its set
    again = src.corrected(*n, positions)
    for key in want:
        assert (want[key] is None and again[key] is None) or np.array_equal(want[key], again[key]), key
    # positions are in dst exactly when they were in src: a correction of the untouched graph hands them back
    dst.build(k)
    nr, nt = dst.correct_reads()            # (nothing was removed: every read, as it is)
    assert (nr, nt) == n
    gs, ge = np.empty(max(nt, 1), np.int32), np.empty(max(nt, 1), np.int32)
    rc = _ffi.lib.amg_get_corrected_positions32(dst._h, _ffi.ptr(gs), _ffi.ptr(ge))
    if positions:
        assert rc == 0 and np.array_equal(gs[:nt], want["gene_start"]) and np.array_equal(ge[:nt], want["gene_end"])
    else:
        assert rc == E_STATE
    # read lengths have no getter: with them or without, dst corrects as a twin that was given the same arrays by hand
    twin.set_reads(want["tokens"], want["read_offsets"], inputs("both_ends_cut")[2].two_v)
    if positions:
        rl = inputs("both_ends_cut")[7][want["orig_read"]]
        twin.set_positions(want["gene_start"], want["gene_end"], rl if lengths else None)
    twin.build(k)
    for e in (dst, twin):
        e.filter(2, 1)
    a, b = dst.corrected(*dst.correct_reads(), positions), twin.corrected(*twin.correct_reads(), positions)
    for key in a:
        assert (a[key] is None and b[key] is None) or np.array_equal(a[key], b[key]), key


def test_build_multi_over_contexts_that_held_something(engines):
    from amira_amd import Engine
    first, second, third, single = engines
    _, n_old = corrected(second, "identity")                # a graph and a corrected set of other reads
    assert set_code(second, n_old) == 0
    k = load(first, "both_ends_cut", positions=False)
    ks = [k, k + 2, k + 4]
    Engine.build_multi([first, second, third], ks)
    load(single, "both_ends_cut", positions=False)
    for e, kk in zip((first, second, third), ks):
        single.build(kk)
        same_state(graph_state(e), graph_state(single), kk)
        ca, cb = e.counts(), single.counts()
        for key in ("k", "n_nodes", "n_edges", "n_windows", "n_short_reads", "n_components", "derived"):
            assert ca[key] == cb[key], (kk, key)
    assert set_code(second, n_old) == E_STATE
    # (the borrowed arrays go back before the module's engines are used again)
    for e in (second, third):
        load(e, "identity", positions=False)
