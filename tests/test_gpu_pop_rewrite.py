"""amg_pop_rewrite (amira_amd/csrc/amg_pop.hip; Engine.pop_rewrite) — the reads of all correction operations of one
correct_bubble_paths call rewritten in one device call — against the pinned oracle's own methods (tests/pop_rewrite.py):
every array of every case for exact equality.  k = 3 and an alphabet of six genes (twelve gene strings) unless a case
says otherwise, so that ties are common.  The last test runs the whole step with and without the call."""
import ctypes as C
import json
import lzma
import os
import random

import numpy as np
import pytest

import pop_rewrite as H
import procedures as P

pytestmark = pytest.mark.gpu

a, b, c, d, e, f = ("+g%d" % i for i in range(6))
A, B, Cc, D, E, F = ("-g%d" % i for i in range(6))


@pytest.fixture(scope="module")
def engine():
    from amira_amd import Engine
    eng = Engine(0)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def vocab():
    from amira_amd.tokens import Vocabulary
    return Vocabulary(H.NAMES)


def check(engine, vocab, k, operations, reads, read_op=None, interest=None):
    """the device's answer equals the oracle's; returns the oracle's (with its info)"""
    read_op = [0] * len(reads) if read_op is None else read_op
    want = H.expected(k, operations, reads, read_op, interest)
    got = engine.pop_rewrite(k, vocab.two_v, *H.encode(vocab, operations, reads, read_op, interest))
    off = got["out_off"].tolist()
    assert off[0] == 0 and all(x <= y for x, y in zip(off, off[1:])) and off[-1] == len(got["out_tok"]) == len(got["out_src"])
    have = H.from_arrays(vocab, got)
    for key in ("op_veto", "status", "first_shared", "last_shared", "genes", "src"):
        assert have[key] == want[key], key
    return want


def spanning(worse, left=(), right=()):
    """reads that hold the whole worse path, on either strand"""
    read = list(left) + list(worse) + list(right)
    return [read, H.mirrored(read)]


# ------------------------------------------------------------------ chosen bubbles
BUBBLES = {
    "substitution": ([a, b, c, D, e, f, a], [a, b, c, d, e, f, a]),
    "insertion": ([a, b, c, e, f, a], [a, b, c, d, e, f, a]),        # (the worse path has a gene more)
    "deletion": ([a, b, c, d, e, f, a], [a, b, c, e, f, a]),
}


@pytest.mark.parametrize("kind", sorted(BUBBLES))
def test_bubbles_with_reads_along_the_whole_path_and_cut_reads(engine, vocab, kind):
    better, worse = BUBBLES[kind]
    reads = spanning(worse) + spanning(worse, [F, E], [Cc, B])
    reads += [worse[2:] + [Cc], [E] + worse[:4], H.mirrored(worse[1:5])]   # start or end inside the path
    want = check(engine, vocab, 3, [(better, worse)], reads)
    assert want["status"] == [2] * len(reads)
    assert [i["way"] for i in want["info"]] == ["fw", "rv", "fw", "rv", "fw", "fw", "rv"]
    assert want["genes"][0] == better and want["genes"][1] == H.mirrored(better)
    assert want["first_shared"][4] == 0 and want["last_shared"][5] == 4      # (the subset is cut at the read's end)


def test_a_read_that_shares_only_a_flank_keeps_its_genes(engine, vocab):
    better, worse = BUBBLES["substitution"]
    reads = [[F, E, a, b, c, Cc, B], [B, Cc] + H.mirrored([a, b, c])]
    want = check(engine, vocab, 3, [(better, worse)], reads)
    assert want["status"] == [2, 2]
    assert [i["second_alignment"] for i in want["info"]] == [False, False]
    assert want["genes"] == reads and want["src"] == [list(range(7)), list(range(5))]


def test_a_mismatch_column_does_not_advance_the_position_counter(engine, vocab):
    """(D, d) in the second alignment: D gets no position, and e after it gets the position of d (the reference's way)"""
    better, worse = BUBBLES["substitution"]
    want = check(engine, vocab, 3, [(better, worse)], [list(worse)])
    assert want["info"][0]["second_alignment"]
    assert want["src"][0] == [0, 1, 2, -1, 3, 4, 5]


# ------------------------------------------------------------------ orientation
def test_orientation_ties_leave_the_read_alone(engine, vocab):
    better, worse = BUBBLES["substitution"]
    reads = [[F, F, E, E, D, D], [], [a, b], worse[:3] + H.mirrored(worse[:3]),
             worse[:4] + [F, F] + H.mirrored(worse[2:6])]
    want = check(engine, vocab, 3, [(better, worse)], reads)
    assert want["status"] == [1] * 5
    assert [(i["fw_count"], i["rv_count"]) for i in want["info"]] == [(0, 0), (0, 0), (0, 0), (1, 1), (2, 2)]


def test_orientation_counts_distinct_gene_mers_not_occurrences(engine, vocab):
    better, worse = BUBBLES["substitution"]
    read = worse[:3] + [F, F] + worse[:3] + [F, F] + H.mirrored(worse[2:6])
    want = check(engine, vocab, 3, [(better, worse)], [read, H.mirrored(read)])
    assert (want["info"][0]["fw_count"], want["info"][0]["rv_count"]) == (1, 2)
    assert [i["way"] for i in want["info"]] == ["rv", "fw"]


def test_worse_path_with_a_repeated_gene_mer(engine, vocab):
    better, worse = [a, b, c, d, a, b, c, e], [a, b, c, a, b, c, e]
    reads = [[a, b, c] + H.mirrored([a, b, c, e]), [a, b, c, a, b, c] + H.mirrored([c, a, b]), [F] + worse,
             H.mirrored(worse) + [F]]
    want = check(engine, vocab, 3, [(better, worse)], reads)
    # (a, b, c) twice on the path is one gene-mer: 1 : 2 and 3 : 1, where occurrences would say 2 : 2 and 4 : 1
    assert [(i["fw_count"], i["rv_count"]) for i in want["info"][:2]] == [(1, 2), (3, 1)]


# ------------------------------------------------------------------ the common run
def test_of_two_equally_long_runs_the_first_wins(engine, vocab):
    better, worse = [a, b, c, D, e, f, a, b], [a, b, c, d, e, f, a, b]
    reads = [[e, f, a, F, a, b, c], [a, b, c, F, e, f, a], [F, b, c, d, F, d, e, f, F]]
    want = check(engine, vocab, 3, [(better, worse)], reads)
    # in (path, read) order: the run earlier on the PATH, wherever it is on the read
    assert [(x, y) for x, y in zip(want["first_shared"], want["last_shared"])] == [(4, 6), (0, 2), (1, 3)]


@pytest.mark.parametrize("length,at", [(64, 56), (65, 57), (65, 56), (200, 60), (200, 124), (200, 192)])
def test_a_run_across_the_lanes_boundary(engine, vocab, length, at):
    """reads of 64, 65 and 200 genes whose run with the path ends at, or straddles, read index 63 / 64 and 127 / 128"""
    better, worse = [a, b, c, D, E, f, a, d], [a, b, c, d, e, f, a, d]
    for strand in (0, 1):
        read = [F] * at + (H.mirrored(worse) if strand else worse) + [F] * (length - at - 8)
        want = check(engine, vocab, 3, [(better, worse)], [read])
        assert (want["first_shared"][0], want["last_shared"][0]) == (at, at + 7) and len(read) == length


# ------------------------------------------------------------------ alignment ties
TIES = {
    "all mismatch": ([a, b, c, d], [A, B, Cc, D, E]),
    "all mismatch, better longer": ([a, b, c, d, e, f], [A, B, Cc, D]),
    "one gene, better shorter": ([a] * 5, [a] * 8),
    "one gene, better longer": ([a] * 9, [a] * 4),
    "shifted tandem": ([a, b, a, b, a, b, c], [b, a, b, a, b, a, c]),
}


@pytest.mark.parametrize("name", sorted(TIES))
def test_alignment_ties(engine, vocab, name):
    """the operation's alignment seen through reads that hold the whole worse path: their subset is all of it"""
    better, worse = TIES[name]
    reads = spanning(worse) + spanning(worse, [F, F], [F])
    want = check(engine, vocab, 3, [(better, worse)], reads)
    assert want["status"] == [2] * 4


def test_alignment_ties_of_a_tandem_array_read_set(engine):
    """tests/golden/data/nw_tie_case.json.xz holds reads of a genome with tandem arrays, found by the fuzzer for an
    alignment tie: every read with the next one of the file as (better, worse), cut to 128 genes, and a read that is
    the worse list"""
    from amira_amd.tokens import Vocabulary
    path = os.path.join(os.path.dirname(__file__), "golden", "data", "nw_tie_case.json.xz")
    reads = list(json.loads(lzma.open(path, "rt").read())["reads"].values())
    lists = [r[:128] for r in reads if len(r) >= 3]
    operations = list(zip(lists[:-1], lists[1:]))[:200]
    own = Vocabulary([x[1:] for r in lists for x in r])
    span = [list(w) for _, w in operations]
    want = check(engine, own, 3, operations, span, list(range(len(operations))))
    assert want["status"].count(2) == len(operations)
    assert sum(i["second_alignment"] for i in want["info"]) > 100


# ------------------------------------------------------------------ the veto
@pytest.mark.parametrize("kind,interest,veto", [
    ("insertion", ["g3"], 1),            # d of the worse path against a gap
    ("substitution", ["g3"], 0),         # d against D: the same gene on the other strand
    ("substitution", ["g0"], 0),         # a against a
    ("insertion", ["g0", "g1"], 0),      # the gene against the gap is none of interest
    ("insertion", None, 0),
    ("insertion", [], 0),
])
def test_veto(engine, vocab, kind, interest, veto):
    better, worse = BUBBLES[kind]
    want = check(engine, vocab, 3, [(better, worse)], spanning(worse), interest=interest)
    assert want["op_veto"] == [veto] and want["status"] == [0 if veto else 2] * 2


def test_veto_against_an_unflagged_gene_and_not_against_a_flagged_one(engine, vocab):
    better, worse = [a, b, c, e, f, a, b], [a, b, c, d, f, a, b]     # (e, d) is a column
    for interest, veto in ((["g3"], 1), (["g3", "g4"], 0), (["g4"], 0)):
        want = check(engine, vocab, 3, [(better, worse)], spanning(worse), interest=interest)
        assert want["op_veto"] == [veto]


# ------------------------------------------------------------------ lengths
def _lists(rng, n, rate=0.08):
    better = [rng.choice(H.GENES) for _ in range(n)]
    while True:
        worse = H.with_errors(rng, better, rate)[:n]
        if len(worse) == n:
            return better, worse


@pytest.mark.parametrize("k", [1, 3, 16])
def test_lists_of_exactly_k_genes(engine, vocab, k):
    rng = random.Random(k)
    better, worse = _lists(rng, k, 0.2)
    reads = spanning(worse) + spanning(worse, [F], [F, E]) + [worse[:-1], [F] * 20]
    want = check(engine, vocab, k, [(better, worse)], reads)
    assert want["status"] == [2, 2, 2, 2, 1, 1 if k > 1 or F not in worse else 2]


@pytest.mark.parametrize("k", [1, 3, 16])
@pytest.mark.parametrize("n", [63, 64, 65, 128])
def test_long_lists(engine, vocab, n, k):
    rng = random.Random(n * 100 + k)
    better, worse = _lists(rng, n)
    reads = spanning(worse) + spanning(worse, [F] * 5, [E] * 70) + [worse[10:50], H.mirrored(worse[n - 40:]),
                                                                    H.with_errors(rng, worse, 0.05)]
    want = check(engine, vocab, k, [(better, worse)], reads)
    assert k == 1 or want["status"][:4] == [2] * 4     # (single genes of both strands on the path: a tie at k = 1)


def _raw_call(engine, vocab, k, operations, reads, read_op, cap=None, pad=16, n_ops=None, bad_token=None,
              claimed_reads=None, claimed_last_read=None):
    """the C entry point with outputs filled with a sentinel, `pad` words of it beyond cap.  claimed_reads: the read
    count handed over (the arrays stay those of `reads`: a count outside the limits is refused before any is looked
    at); claimed_last_read: the length the offsets give the last read (refused before a token is read)"""
    from amira_amd import _ffi
    bt, bo, wt, wo, flags, rt, ro, rop = H.encode(vocab, operations, reads, read_op)
    if bad_token is not None:
        rt[3] = bad_token
    if claimed_last_read is not None:
        ro[-1] = ro[-2] + claimed_last_read
    bound = len(rt) + sum(len(operations[o][0]) for o in read_op if 0 <= o < len(operations))
    cap = bound if cap is None else cap
    n_ops, n_reads = len(operations) if n_ops is None else n_ops, len(reads)
    out = {"op_veto": np.full(n_ops + pad, 0x77, np.uint8), "status": np.full(n_reads + pad, 0x77, np.uint8),
           "first_shared": np.full(n_reads + pad, -7, np.int32), "last_shared": np.full(n_reads + pad, -7, np.int32),
           "out_off": np.full(n_reads + 1 + pad, -7, np.int64), "out_tok": np.full(cap + pad, -7, np.int32),
           "out_src": np.full(cap + pad, -7, np.int32)}
    n_out = C.c_int64(-7)
    rc = _ffi.lib.amg_pop_rewrite(engine._h, k, vocab.two_v, n_ops, _ffi.ptr(bt), _ffi.ptr(bo), _ffi.ptr(wt), _ffi.ptr(wo),
                                  None, n_reads if claimed_reads is None else claimed_reads, _ffi.ptr(rt), _ffi.ptr(ro), _ffi.ptr(rop), cap, _ffi.ptr(out["op_veto"]),
                                  _ffi.ptr(out["status"]), _ffi.ptr(out["first_shared"]), _ffi.ptr(out["last_shared"]),
                                  _ffi.ptr(out["out_off"]), _ffi.ptr(out["out_tok"]), _ffi.ptr(out["out_src"]),
                                  C.byref(n_out))
    return rc, out, n_out.value, bound


def _untouched(out):
    return all((v == (0x77 if v.dtype == np.uint8 else -7)).all() for v in out.values())


def test_refusals_leave_the_outputs_alone(engine, vocab):
    from amira_amd import _ffi
    rng = random.Random(129)
    long_list, other = _lists(rng, 129)
    ok = _lists(rng, 20)
    one = dict(operations=[ok], reads=[ok[1]], read_op=[0], k=3)
    for change in (
            dict(operations=[(long_list, other[:100])]),              # 129 better genes
            dict(operations=[(other[:100], long_list)]),              # 129 worse genes
            dict(operations=[ok, (ok[0], ok[1][:2])]),                # a list shorter than k
            dict(k=0), dict(k=17), dict(read_op=[1]), dict(read_op=[-1]),
            dict(reads=[ok[1], ok[1]], read_op=[0, 0], cap=79),       # the bound is 2 * (20 + 20)
            dict(reads=[], read_op=[]), dict(n_ops=0),
            dict(claimed_reads=(1 << 20) + 1), dict(n_ops=(1 << 20) + 1),   # the upper bounds on reads and operations
            dict(claimed_last_read=(1 << 24) + 1, cap=1 << 25),             # a read beyond 2^24 genes
            dict(bad_token=-1), dict(bad_token=vocab.two_v)):
        rc, out, n_out, _ = _raw_call(engine, vocab, **{**one, **change})
        assert rc == _ffi.E_ARG, sorted(change)
        assert _untouched(out) and n_out == -7, sorted(change)
    # the engine says so with that code (correct_bubble_paths then takes the loop on the host)
    with pytest.raises(_ffi.AmgError) as err:
        engine.pop_rewrite(3, vocab.two_v, *H.encode(vocab, [(long_list, other[:100])], [other[:30]], [0]))
    assert err.value.code == _ffi.E_ARG
    # which the product's caller knows beforehand from the sizes alone, so that no other refusal passes for this one
    declines = type(engine).pop_rewrite_declines
    assert declines(3, [long_list], [other[:100]], [other[:30]]) and declines(3, [other[:100]], [long_list], [other[:30]])
    assert declines(3, [ok[0]], [ok[1][:2]], [ok[1]]) and declines(17, [long_list[:20]], [other[:20]], [ok[1]])
    assert not declines(3, [long_list[:128]], [other[:3]], [[], other])
    # and the call before the refusals still works after them
    assert _raw_call(engine, vocab, **one)[0] == 0


# ------------------------------------------------------------------ packing
def test_packing_with_every_status_and_nothing_written_beyond(engine, vocab):
    from amira_amd import _ffi
    sub, ins = BUBBLES["substitution"], BUBBLES["insertion"]
    operations = [sub, ins, ([a, b, c, e, f, a, b], [a, b, c, d, f, a, b])]
    reads = [list(sub[1]), [F, F, F], list(ins[1]), H.mirrored(sub[1]) + [F], [], list(operations[2][1]), [E] + list(sub[1])]
    read_op = [0, 0, 1, 0, 2, 2, 0]
    want = check(engine, vocab, 3, operations, reads, read_op, interest=["g3"])
    assert want["op_veto"] == [0, 1, 1] and want["status"] == [2, 1, 0, 2, 0, 0, 2]
    # the same call without genes of interest, into sentinel-filled arrays with exactly the bound as cap
    want = H.expected(3, operations, reads, read_op)
    rc, out, n_out, bound = _raw_call(engine, vocab, 3, operations, reads, read_op)
    assert rc == 0
    n_ops, n_reads = len(operations), len(reads)
    off = out["out_off"][:n_reads + 1].tolist()
    assert off[0] == 0 and off == sorted(off) and off[-1] == n_out == sum(len(x) for x in want["genes"] if x is not None)
    assert n_out < bound
    got = H.from_arrays(vocab, {"op_veto": out["op_veto"][:n_ops], "status": out["status"][:n_reads],
                                "first_shared": out["first_shared"][:n_reads], "last_shared": out["last_shared"][:n_reads],
                                "out_off": out["out_off"][:n_reads + 1], "out_tok": out["out_tok"][:n_out],
                                "out_src": out["out_src"][:n_out]})
    for key in got:
        assert got[key] == want[key], key
    for key, n in (("op_veto", n_ops), ("status", n_reads), ("first_shared", n_reads), ("last_shared", n_reads),
                   ("out_off", n_reads + 1), ("out_tok", n_out), ("out_src", n_out)):
        tail = out[key][n:]
        assert len(tail) >= 16 and (tail == (0x77 if tail.dtype == np.uint8 else -7)).all(), key


# ------------------------------------------------------------------ seeded fuzz
FUZZ_SEED = 11   # chosen on the CPU: the oracle's answers alone satisfy the assertions below


def test_seeded_fuzz(engine, vocab):
    operations, reads, read_op = H.planted(FUZZ_SEED)
    assert len(operations) == 40 and len(reads) == 320
    assert all(3 <= len(x) <= 40 for op in operations for x in op)
    want = check(engine, vocab, 3, operations, reads, read_op, interest=["g0"])
    # not vacuous, by the oracle's own answers
    for status in (0, 1, 2):
        assert want["status"].count(status) >= 0.05 * len(reads), status
    rewritten = [i for s, i in zip(want["status"], want["info"]) if s == 2]
    assert {i["way"] for i in rewritten} == {"fw", "rv"}
    assert {i["second_alignment"] for i in rewritten} == {True, False}
    cores = [x for i in rewritten for x in i["core_src"]]
    assert -1 in cores and any(x >= 0 for x in cores)


# ------------------------------------------------------------------ the whole step
CASES = [(71, 300, 30, 120, 3, 0.04), (72, 400, 25, 90, 3, 0.05), (73, 300, 40, 150, 5, 0.04)]


def _graph(seed, N, L, V, k, err, min_cov=3):
    from amira_amd import GeneMerGraph, synth
    ids, sts = synth.loop_reads(seed, N, L, V, err, 0)
    calls = synth.to_read_dict(ids, sts, synth.gene_names(V, 0))
    pos = {r: [(80 * i, 80 * i + 59) for i in range(len(g))] for r, g in calls.items()}
    fq = P.synth_fastq(calls, pos, flank=40)
    g = GeneMerGraph(calls, k, pos)
    g.filter_graph(min_cov, 1)
    calls, pos = g.correct_reads(fq)
    return GeneMerGraph(calls, k, pos), fq


def test_whole_step_with_and_without_the_device_call(monkeypatch):
    rewritten = 0
    for case in CASES:
        results = []
        for switch in (None, "0"):
            if switch is None:
                monkeypatch.delenv("AMG_POP_REWRITE", raising=False)
            else:
                monkeypatch.setenv("AMG_POP_REWRITE", switch)
            g, fq = _graph(*case)
            before = dict(g._engine.pop_rewrite_stats)
            assert before["declined"] == 0
            reads, pos, covs, _ = g.correct_low_coverage_paths(fq, set(), 1, 2, set(), use_minimizers=True)
            after = g._engine.pop_rewrite_stats
            if switch is None:
                rewritten += after["rewritten"] - before["rewritten"]
                assert after["declined"] == 0   # (no quiet way round the call)
            else:
                assert after == before
            results.append(({r: list(v) for r, v in reads.items()}, {r: [tuple(p) for p in v] for r, v in pos.items()},
                            [float(x) for x in covs]))
        assert results[0][0] == results[1][0]
        assert results[0][1] == results[1][1]
        assert results[0][2] == results[1][2]
    assert rewritten >= 1
