"""CPU: tests/select_oracle.py — the numpy statement the GPU tests of amg_select_reads take their expectations from —
held to the pinned pure-Python oracle (amira_oracle's remove_junk_reads / get_valid_reads_only; the goldens misc_* pin
those to the reference) on the named case of select_oracle.named_case."""
import numpy as np
import pytest

import select_oracle as S

WANT = S.CASE_WANT


@pytest.fixture(scope="module")
def case():
    from amira_oracle import GeneMerGraph
    reads, pos, _ = S.named_case()
    g = GeneMerGraph(dict(reads), S.CASE_K, {r: list(v) for r, v in pos.items()})
    g.filter_graph(3, 1)
    vocab, toks, offs, ids, tok_node, fix = S.arrays_of_oracle_graph(g, reads)
    gs = np.asarray([p[0] for r in ids for p in pos[r]], np.int64)
    ge = np.asarray([p[1] for r in ids for p in pos[r]], np.int64)
    return {"g": g, "reads": reads, "pos": pos, "vocab": vocab, "toks": toks, "offs": offs, "ids": ids,
            "tok_node": tok_node, "fix": fix, "gs": gs, "ge": ge}


def _as_dicts(c, out):
    """the selected set of select_oracle.select as the reference's two dicts"""
    ids = [c["ids"][r] for r in out["rows"].tolist()]
    off = out["read_offsets"].tolist()
    reads = {r: c["vocab"].decode(out["tokens"][off[i]:off[i + 1]]) for i, r in enumerate(ids)}
    pos = {r: list(zip(out["gene_start"][off[i]:off[i + 1]].tolist(), out["gene_end"][off[i]:off[i + 1]].tolist()))
           for i, r in enumerate(ids)}
    return reads, pos


def test_the_case_is_what_the_tests_need(case):
    g, offs = case["g"], case["offs"]
    w = S.windows(offs, S.CASE_K)
    assert len(g.get_short_read_annotations()) == 58 and len(g.get_readNodes()) == 342
    assert len(g.get_reads_to_correct()) == 235 and len(g.get_valid_reads_only()) == 165
    assert {0, 1, 64, 65, 66, 88} <= set(w.tolist())
    assert int((w > 64).sum()) > 0                      # a listed read beyond one wave of windows
    assert int((np.diff(offs) == 0).sum()) > 0          # a read without a gene
    m = S.masked_windows(offs, S.CASE_K, case["tok_node"])
    assert int(((m == w) & (w > 0)).sum()) == 16        # reads whose every window is masked


@pytest.mark.parametrize("rate", S.CASE_RATES)
def test_junk_equals_the_oracle(case, rate):
    c = case
    keep, keep_pos, drop, drop_pos = c["g"].remove_junk_reads(rate)
    assert (len(keep), len(drop)) == WANT[rate]
    w = S.windows(c["offs"], S.CASE_K)
    table = S.allowed_table(rate, int(w.max()))
    for invert, (want_reads, want_pos) in ((0, (keep, keep_pos)), (1, (drop, drop_pos))):
        out = S.select(c["toks"], c["offs"], S.CASE_K, c["tok_node"], c["fix"], S.JUNK, invert, table, c["gs"], c["ge"])
        got_reads, got_pos = _as_dicts(c, out)
        # the reference fills its dicts in the order of _readNodes, which is read order
        assert list(got_reads) == list(want_reads) and got_reads == {r: list(v) for r, v in want_reads.items()}
        assert got_pos == {r: [tuple(p) for p in v] for r, v in want_pos.items()}
    v = S.verdicts(c["offs"], S.CASE_K, c["tok_node"], c["fix"], S.JUNK, table)
    assert int((v == S.UNLISTED).sum()) == 58 and np.array_equal(v == S.UNLISTED, w == 0)
    if rate in (0.8, 0.75, 0.5):
        assert len(keep) > 0 and len(drop) > 0
    if rate in (0.75, 0.5):
        # reads the rounding decides: w * (1 - rate) is x.5 and the masked windows are floor or floor + 1 of it
        m = S.masked_windows(c["offs"], S.CASE_K, c["tok_node"])
        prod = w * (1 - rate)
        half = (w > 0) & (prod - np.floor(prod) == 0.5)
        decided = half & ((m == np.floor(prod)) | (m == np.floor(prod) + 1))
        assert int(decided.sum()) == {0.75: 33, 0.5: 38}[rate]
        for r in np.flatnonzero(decided).tolist():   # half to even, not half up
            assert table[w[r]] == int(np.floor(prod[r])) + (int(np.floor(prod[r])) % 2)


def test_valid_equals_the_oracle(case):
    c = case
    want = c["g"].get_valid_reads_only()
    out = S.select(c["toks"], c["offs"], S.CASE_K, c["tok_node"], c["fix"], S.VALID, 0, None, c["gs"], c["ge"])
    got_reads, got_pos = _as_dicts(c, out)
    assert list(got_reads) == list(want) and got_reads == {r: list(v) for r, v in want.items()}
    assert got_pos == {r: [tuple(p) for p in c["pos"][r]] for r in want}
    assert any(len(v) == 0 for v in got_reads.values())   # a read without a gene stays, as []
    rejected = S.select(c["toks"], c["offs"], S.CASE_K, c["tok_node"], c["fix"], S.VALID, 1)
    assert [c["ids"][r] for r in rejected["rows"].tolist()] == [r for r in c["ids"] if r in c["g"].get_reads_to_correct()]
    assert not (S.verdicts(c["offs"], S.CASE_K, c["tok_node"], c["fix"], S.VALID) == S.UNLISTED).any()


def test_a_table_that_ends_before_the_longest_read_is_refused(case):
    c = case
    longest = int(S.windows(c["offs"], S.CASE_K).max())
    assert S.verdicts(c["offs"], S.CASE_K, c["tok_node"], c["fix"], S.JUNK, [0] * longest) is None
    assert S.verdicts(c["offs"], S.CASE_K, c["tok_node"], c["fix"], S.JUNK, [0] * (longest + 1)) is not None
