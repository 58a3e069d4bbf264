"""The path memo's search with one lane per question (k_gap_dfs_lanes, amg_gap_memo.hip) against the wave per question
(k_gap_dfs, AMG_GAP_DFS_WAVE=1) and against no memo at all (AMG_NO_GAP_MEMO=1).

Every case is a constructed read set of a few hundred reads at most, whose gapped reads have at most 64 windows (longer
ones take no part in the memo).  It runs three times, each time through `correct_case` of test_gpu_correct_limits:
exact equality with the pinned Python oracle after build, filter, correction and rebuild.  The route reports of the
first two runs must be equal as dicts (same questions, same answers spilled or unfit, same reads handed on).

What the cases are built for: the lane kernel's grid edges (a full wave, one lane into the next wave, one lane into
the next workgroup), the accept / retreat rule at exactly 2k and 2k + 1 nodes, searches without an answer, one wave
whose lanes end in every way (one answer, two answers inline, an answer set beyond GM_INLINE that takes the wave's
turn, none), the no-node-twice rule on repeated genes, searches that start in direction -1, a row whose list has to be
walked entry by entry, and k = 7 / 8: the last k of the lane kernel (its stack of 16 levels filled) and the first k of
the wave kernel by the k rule."""
import pytest

from test_gpu_correct_limits import backbone, bubbles, correct_case, expect, tandem_reads

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from amira_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def three_ways(eng, monkeypatch, reads, k, **want):
    """lane kernel (default), wave kernel, no memo: each equal to the oracle; the first two with equal route reports"""
    lanes, r2 = correct_case(eng, monkeypatch, reads, k)
    monkeypatch.setenv("AMG_GAP_DFS_WAVE", "1")
    wave, _ = correct_case(eng, monkeypatch, reads, k)
    monkeypatch.delenv("AMG_GAP_DFS_WAVE")
    monkeypatch.setenv("AMG_NO_GAP_MEMO", "1")
    no_memo, _ = correct_case(eng, monkeypatch, reads, k)
    monkeypatch.delenv("AMG_NO_GAP_MEMO")
    assert lanes == wave, {n: (lanes[n], wave[n]) for n in lanes if lanes[n] != wave[n]}
    assert no_memo["memo_questions"] == 0 and no_memo["keep_orig"] == lanes["keep_orig"]
    expect(lanes, **want)
    return lanes, r2


def reverse(read):
    """the same molecule read from the other strand"""
    return [("-" if g[0] == "+" else "+") + g[1:] for g in reversed(read)]


# ------------------------------------------------------------------ the grid's edges
@pytest.mark.parametrize("n_questions", [1, 64, 65, 257])
def test_question_counts(eng, monkeypatch, n_questions):
    """k = 5: noisy slices of 19 genes of a long genome, each with one substituted gene at a place of its own: as many
    distinct questions as slices (the last lane of a wave, the first of the next wave, the first of the next workgroup)"""
    k = 5
    n_genes = n_questions + 20
    reads = backbone(n_genes, [dict(a=p - 9, b=p + 10, subs=(p,)) for p in range(10, 10 + n_questions)])
    routes, r2 = three_ways(eng, monkeypatch, reads, k, gapped=n_questions, memo_questions=n_questions, keep_orig=0,
                            memo_spilled=0, memo_unfit=0, by_lean=n_questions)
    genome = reads["c000"]
    for j, p in enumerate(range(10, 10 + n_questions)):
        assert r2[f"n{j:03d}"] == genome[p - 9:p + 10]


# ------------------------------------------------------------------ the length rule, and the stack at its limit
@pytest.mark.parametrize("k", [3, 5, 7, 8])
def test_path_length_at_the_limit(eng, monkeypatch, k):
    """a read that lacks d genes asks for a path of k + 1 + d nodes.  d = k - 1: 2k nodes, accepted; d = k: 2k + 1
    nodes, reached but not accepted, and the search goes one node further before it retreats (2k + 2 levels: all 16 at
    k = 7, the last k of the lane kernel; k = 8 takes the wave kernel by the k rule); a third read with one
    substituted gene (k + 2 nodes)"""
    reads = backbone(60, [dict(a=0, b=60, cuts=[(25, k - 1)]), dict(a=0, b=60, cuts=[(25, k)]),
                          dict(a=0, b=60, subs=(30,))])
    routes, r2 = three_ways(eng, monkeypatch, reads, k, gapped=3, memo_questions=3, keep_orig=1, memo_spilled=0,
                            memo_unfit=0)
    assert r2["n000"] == reads["c000"] and r2["n001"] == reads["n001"] and r2["n002"] == reads["c000"]


def test_dead_end(eng, monkeypatch):
    """k = 5: a deletion of 2k + 3 genes, further than any search reaches, beside a read that is re-threaded"""
    k = 5
    reads = backbone(70, [dict(a=0, b=70, cuts=[(30, 2 * k + 3)]), dict(a=10, b=50, subs=(30,))])
    routes, r2 = three_ways(eng, monkeypatch, reads, k, gapped=2, memo_questions=2, keep_orig=1)
    assert r2["n000"] == reads["n000"] and r2["n001"] == reads["c000"][10:50]


# ------------------------------------------------------------------ one wave, every kind of answer
def test_one_wave_of_every_kind(eng, monkeypatch):
    """k = 5, a record of k + 2 nodes is 16 ints.  A site with two alleles (32 ints: inline), a site with five (80
    ints: beyond GM_INLINE = 64, the lane hands the question to its wave, which spills the answer), a substituted gene
    where the genome has one path, and a deletion nothing bridges: four questions in one wave"""
    k = 5
    n = 66
    sites = {10: 2, 30: 5}

    def genome(allele, unknown=()):
        return [(f"+u{i}" if i in unknown else f"+s{i}a{allele % sites[i]}") if i in sites else f"+g{i}"
                for i in range(n)]

    reads = {"q_two": genome(0, unknown=(10,)), "q_many": genome(0, unknown=(30,))}
    one = genome(0)
    one[50] = "+x50"
    reads["q_one"] = one
    reads["q_none"] = genome(0)[:40] + genome(0)[40 + 2 * k + 3:]
    for a in range(5):
        for c in range(3 + a):  # (depths differ: no two candidates tie on coverage)
            reads[f"a{a}_{c}"] = genome(a)
    routes, r2 = three_ways(eng, monkeypatch, reads, k, gapped=4, memo_questions=4, memo_spilled=1, memo_unfit=0,
                            keep_orig=1, by_lean=1)
    assert r2["q_none"] == reads["q_none"] and r2["q_one"] == genome(0)


def test_many_alleles_take_the_waves_turn(eng, monkeypatch):
    """`bubbles` with five alleles at each of two sites, k = 5: both questions go through the wave's turn"""
    routes, _ = three_ways(eng, monkeypatch, bubbles(2, 5, 8), 5, gapped=1, memo_questions=2, memo_spilled_min=1,
                           memo_unfit=0)
    assert routes["memo_spilled"] == 2


def test_the_waves_turn_finds_the_pool_used_up(eng, monkeypatch):
    """the same read set with AMG_TEST_MEMO_SPILL=100: of the two spilled answers (80 ints each) one finds room behind
    the inline stretches, the other does not fit, and its read goes to the general kernel — same corrected reads"""
    monkeypatch.setenv("AMG_TEST_MEMO_SPILL", "100")
    three_ways(eng, monkeypatch, bubbles(2, 5, 8), 5, gapped=1, memo_questions=2, memo_spilled=1, memo_unfit=1,
               on_memo_unfit=1, by_general=1)


# ------------------------------------------------------------------ no node twice
def test_repeated_gene(eng, monkeypatch):
    """k = 5: the genome has the same gene twice in a row at two places; reads that lack one of the two copies, and
    reads with a substituted gene beside them"""
    reads = backbone(70, [dict(a=0, b=40, cuts=[(21, 1)]), dict(a=30, b=70, cuts=[(51, 1)], subs=(40,)),
                          dict(a=0, b=60, subs=(19,)), dict(a=10, b=64, subs=(22, 52))], twice=(20, 50))
    routes, r2 = three_ways(eng, monkeypatch, reads, 5, gapped=4, keep_orig=0)
    genome = reads["c000"]
    assert r2["n000"] == genome[:40] and r2["n001"] == genome[30:70] and r2["n002"] == genome[:60]
    assert r2["n003"] == genome[10:64]


@pytest.mark.parametrize("seed,k", [(3, 3), (4, 5)])
def test_tandem_arrays(eng, monkeypatch, seed, k):
    """tandem gene arrays (the same gene 7 to 20 times in a row) in reads of 30 to 60 genes: a search meets its own
    path again and may not step on it"""
    reads, _, _ = tandem_reads(seed, 120, (30, 44, 52, 60), 0.04)
    three_ways(eng, monkeypatch, reads, k, memo_questions_min=20)


# ------------------------------------------------------------------ direction -1, and a list that is walked
def test_reverse_strand(eng, monkeypatch):
    """k = 5: every noisy read twice, as written and from the other strand: the same stretch of the genome is asked for
    from both ends, one of the two searches starts in direction -1"""
    k = 5
    reads = backbone(90, [dict(a=p - 12, b=p + 13, subs=(p,)) for p in range(15, 75, 6)])
    for name in [r for r in reads if r.startswith("n")]:
        reads["r" + name[1:]] = reverse(reads[name])
    routes, r2 = three_ways(eng, monkeypatch, reads, k, gapped=20, keep_orig=0, memo_questions=20)
    genome = reads["c000"]
    for j, p in enumerate(range(15, 75, 6)):
        assert r2[f"n{j:03d}"] == genome[p - 12:p + 13] and r2[f"r{j:03d}"] == reverse(genome[p - 12:p + 13])


def test_junction_with_five_successors(eng, monkeypatch):
    """k = 5: a common stretch followed by five different ones, four clean reads each: the last node of the common
    stretch has five live successors.  For every branch one read with the first gene behind the junction substituted
    (the search starts AT the junction and walks its list until it is on the right branch) and one with the last gene
    before it substituted (the junction is met in mid-path); wrong branches are walked to the length limit"""
    k = 5
    common = [f"+p{i}" for i in range(24)]
    branch = [[f"+b{b}_{i}" for i in range(24)] for b in range(5)]
    reads = {}
    for b in range(5):
        whole = common + branch[b]
        at = whole[6:42]
        at[24 - 6] = f"+x{b}"
        reads[f"at{b}"] = at
        mid = whole[4:40]
        mid[23 - 4] = f"+y{b}"
        reads[f"mid{b}"] = mid
        for c in range(4):
            reads[f"c{b}_{c}"] = list(whole)
    routes, r2 = three_ways(eng, monkeypatch, reads, k, gapped=10, memo_questions=10, keep_orig=0, memo_spilled=0)
    for b in range(5):
        whole = common + branch[b]
        assert r2[f"at{b}"] == whole[6:42] and r2[f"mid{b}"] == whole[4:40]
