"""amg_correct_reads at the capacity limits where a read is handed from a faster kernel to a more general one
(amg_correct.h: GF_MAXW, GF_MAXGAP, GF_POOL, GF_MAXCOMBO, GF_CAND, GM_INLINE, LEAN_CHUNK, NWF_MAX_M / NWF_MAX_N,
NW_LDS_CELLS, NW_LDS_N; the path memo's pool and the general kernel's pool in corr_gapped).

Every case is a constructed read set.  It asserts (a) equality with the pinned Python oracle — graph arrays after
build and after filter, corrected genes, read order and positions, then the rebuild from the corrected reads — and
(b), through the route report (AMG_CORR_ROUTES=1, Engine.correct_routes()), that the reads built for a route took it,
for the reason they were built for.  All comparisons are exact.

Two generators: `backbone` (a genome of distinct genes, five clean reads over it, noisy reads with substituted or
missing genes at chosen places) and `bubbles` (sites with several alleles, carried by groups of reads of different
depth, and a read with an unknown gene at every site: the oracle enumerates al ** nb candidates).

Oracle time per case on one CPU core (build + filter + correct + rebuild), measured when the cases were written:
every case below 1 s except the 1 100-gene read (about 3 s), the 2 000-gene read (about 10 s) and the whole sweeps at
k = 15 / 16 and over tandem arrays (2 - 6 s each).

Not covered HERE: N = 128 corrected genes against M <= 64 original ones (the far corner of nw_fast_ok): a None run
adds at most about k genes, so real reads cannot get there.  tests/test_gpu_carry_over.py hands the carry-over kernels
such pairs directly (amg_nw_probe), with every other shape at their limits.  A single path record only exceeds
GM_INLINE at k = 16 (a path of 2k = 32 nodes is 2 + 64 ints; at k = 15 the longest is 62 ints), so the k = 15 read of
that case stays inline."""
import numpy as np
import pytest

import procedures as P
from helpers import check_corrected, compare_engine_to_oracle, flat_positions, oracle_arrays

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from amira_amd import Engine
    e = Engine(0)
    yield e
    e.close()


# ------------------------------------------------------------------ generators
def noisy(genome, a, b, subs=(), cuts=(), tag="x"):
    """genes a .. b-1 of the genome with the genes at `subs` (genome coordinates) replaced by genes nobody else has
    and, for every (at, d) of `cuts`, the d genes from `at` on left out"""
    gone = {i for at, d in cuts for i in range(at, at + d)}
    return [f"+{tag}{i}" if i in subs else genome[i] for i in range(a, b) if i not in gone]


def backbone(n_genes, noisy_reads, n_clean=5, extra=(), twice=()):
    """noisy reads first (read order matters to nothing but is part of what is compared), then the clean ones; the
    gene at p + 1 repeats the one at p for every p of `twice`"""
    genome = [f"+g{i}" for i in range(n_genes)]
    for p in twice:
        genome[p + 1] = genome[p]
    reads = {}
    for j, spec in enumerate(noisy_reads):
        reads[f"n{j:03d}"] = noisy(genome, tag=f"x{j}_", **spec)
    for j in range(n_clean):
        reads[f"c{j:03d}"] = list(genome)
    for j, r in enumerate(extra):
        reads[f"e{j:03d}"] = list(r)
    return reads


def bubbles(nb, al, space, first=5, tail=None, queries=None, depth=lambda g: 3 + g):
    """backbone with nb sites `space` genes apart and al alleles per site; read group g (depth(g) reads) carries
    allele (g + s) % al at site s, so the best allele differs from site to site; query q has an unknown gene at the
    first queries[q] sites and allele 0 behind them"""
    tail = space if tail is None else tail
    n = first + space * (nb - 1) + 1 + tail
    sites = {first + space * s: s for s in range(nb)}
    reads = {}
    for qi, nq in enumerate(queries if queries is not None else [nb]):
        reads[f"q{qi}"] = [(f"+u{qi}_{sites[i]}" if sites[i] < nq else f"+s{sites[i]}a0") if i in sites else f"+g{i}"
                           for i in range(n)]
    for g in range(al):
        for c in range(depth(g)):
            reads[f"a{g:02d}_{c}"] = [f"+s{sites[i]}a{(g + sites[i]) % al}" if i in sites else f"+g{i}" for i in range(n)]
    return reads


LONG_TANDEM_ARRAYS = ((12, "t0", 9), (60, "t1", 14), (110, "t2", 12), (170, "t3", 20), (230, "t4", 7))


def tandem_reads(seed, n_reads, lengths, err):
    """_tandem_reads of test_gpu_sweep.py over a longer genome with longer tandem arrays, read lengths from `lengths`"""
    from test_gpu_sweep import _tandem_reads
    return _tandem_reads(seed, n_reads, None, err, glen=260, arrays=LONG_TANDEM_ARRAYS, lengths=lengths)


# ------------------------------------------------------------------ one case against the oracle
def positions_and_lengths(reads):
    """gene i at [1000 i, 1000 i + 899], read length 1000 n + 100: a repaired last position (length - 1) is no gene's
    end"""
    from amira_amd import synth
    return synth.positions_for(reads), P.FakeFastq(synth.fake_fastq_lengths(reads))


def correct_case(eng, monkeypatch, reads, k, min_cov=3):
    """build, filter, correct, rebuild — everything compared with the oracle; returns the route report and the
    oracle's corrected reads"""
    from amira_amd import tokenize
    from amira_oracle import GeneMerGraph
    monkeypatch.setenv("AMG_CORR_ROUTES", "1")
    pos, fq = positions_and_lengths(reads)
    vocab, toks, offs, read_ids = tokenize(reads)
    eng.set_reads(toks, offs, vocab.two_v)
    gs, ge = flat_positions(read_ids, reads, pos)
    eng.set_positions(gs, ge, np.asarray([len(fq[r]["sequence"]) for r in read_ids], dtype=np.int64))
    eng.build(k)
    g1 = GeneMerGraph(reads, k, {r: list(v) for r, v in pos.items()})
    compare_engine_to_oracle(eng, oracle_arrays(g1, vocab, read_ids, offs, k))
    eng.filter(min_cov, 1)
    g1.filter_graph(min_cov, 1)
    compare_engine_to_oracle(eng, oracle_arrays(g1, vocab, read_ids, offs, k), live_only=True)
    r2, p2 = g1.correct_reads(fq)
    ids2, out2 = check_corrected(eng, vocab, read_ids, r2, p2)
    routes = eng.correct_routes()
    print("routes:", {n: v for n, v in routes.items() if v})
    eng.adopt_corrected()
    eng.build(k)
    g2 = GeneMerGraph(r2, k, p2)
    compare_engine_to_oracle(eng, oracle_arrays(g2, vocab, ids2, out2["read_offsets"], k))
    return routes, r2


def expect(routes, **want):
    """exact tallies; a name ending in _min asks for at least that many"""
    for name, v in want.items():
        if name.endswith("_min"):
            assert routes[name[:-4]] >= v, (name, v, routes)
        else:
            assert routes[name] == v, (name, v, routes)


MEMO = [pytest.param({}, id="memo"), pytest.param({"AMG_NO_GAP_MEMO": "1"}, id="no_memo")]


def setenv(monkeypatch, env):
    for name, v in env.items():
        monkeypatch.setenv(name, v)


def every(n, step, start=5):
    return tuple(range(start, n, step))


# ------------------------------------------------------------------ re-threading: the wave-per-read kernel's limits
@pytest.mark.parametrize("env", MEMO)
def test_windows_at_gf_maxw(eng, monkeypatch, env):
    """k = 5, reads of 132 and 133 genes = 128 and 129 windows: the first is finished by the wave-per-read kernel, the
    second is handed on for its windows"""
    setenv(monkeypatch, env)
    reads = backbone(133, [dict(a=0, b=132, subs=every(126, 11)), dict(a=0, b=133, subs=every(127, 11, 7))])
    routes, r2 = correct_case(eng, monkeypatch, reads, 5)
    assert r2["n000"] == reads["c000"][:132] and r2["n001"] == reads["c000"]
    expect(routes, gapped=2, by_fast=1, by_general=1, on_windows=1, no_memo_slots=2, keep_orig=0)


@pytest.mark.parametrize("env", MEMO)
def test_windows_at_the_memo_cut(eng, monkeypatch, env):
    """k = 5, 64 and 65 windows: the first read has memo slots (and one answer per question: sixteen lanes do it), the
    second has none and searches for itself in the wave-per-read kernel"""
    setenv(monkeypatch, env)
    reads = backbone(69, [dict(a=0, b=68, subs=every(62, 9)), dict(a=0, b=69, subs=every(63, 9, 7))])
    routes, r2 = correct_case(eng, monkeypatch, reads, 5)
    assert r2["n000"] == reads["c000"][:68] and r2["n001"] == reads["c000"]
    if env:
        expect(routes, gapped=2, by_fast=2, by_lean=0, no_memo_slots=2, memo_questions=0)
    else:
        expect(routes, gapped=2, by_lean=1, by_fast=1, lean_no_slots=1, no_memo_slots=1, memo_questions_min=7)


@pytest.mark.parametrize("env", MEMO)
def test_runs_at_gf_maxgap(eng, monkeypatch, env):
    """k = 3, substitutions 7 genes apart: 16 None runs stay in the wave-per-read kernel, 17 are handed on (114 and 121 windows: neither has memo
    slots, both search for themselves)"""
    setenv(monkeypatch, env)
    reads = backbone(124, [dict(a=0, b=116, subs=every(111, 7)), dict(a=0, b=123, subs=every(118, 7))])
    routes, r2 = correct_case(eng, monkeypatch, reads, 3)
    assert r2["n000"] == reads["c000"][:116] and r2["n001"] == reads["c000"][:123]
    expect(routes, gapped=2, by_fast=1, by_general=1, on_runs=1, keep_orig=0)


@pytest.mark.parametrize("env", MEMO)
def test_runs_at_the_memo_cut(eng, monkeypatch, env):
    """k = 2, substitutions 3 genes apart in reads of at most 64 windows: with 16 runs (52 windows) the read has memo
    slots and sixteen lanes finish it; with 17 (55 windows) the memo leaves it out (k_gap_queries), the sixteen lanes
    leave it for that, and the wave-per-read kernel hands it on for its runs"""
    setenv(monkeypatch, env)
    reads = backbone(60, [dict(a=0, b=53, subs=every(50, 3, 3)), dict(a=0, b=56, subs=every(53, 3, 3))])
    routes, r2 = correct_case(eng, monkeypatch, reads, 2)
    assert r2["n000"] == reads["c000"][:53] and r2["n001"] == reads["c000"][:56]
    expect(routes, gapped=2, by_general=1, on_runs=1, keep_orig=0)
    if env:
        expect(routes, by_fast=1, no_memo_slots=2)
    else:
        expect(routes, by_lean=1, by_fast=0, lean_no_slots=1, no_memo_slots=1, memo_questions=16)


@pytest.mark.parametrize("env", MEMO)
def test_combinations_at_gf_maxcombo(eng, monkeypatch, env):
    """9 sites 6 genes apart, 2 alleles, k = 5, 56 windows: the read with 8 unknown sites has exactly 256 candidates
    (wave-per-read kernel), the one with 9 has 512 (handed on for its combinations; 18 records of 16 ints = 288)"""
    setenv(monkeypatch, env)
    routes, _ = correct_case(eng, monkeypatch, bubbles(9, 2, 6, queries=[8, 9]), 5)
    expect(routes, gapped=2, by_fast=1, by_general=1, on_combos=1, keep_orig=0)
    if not env:
        expect(routes, lean_answers=2, no_memo_slots=0, memo_unfit=0)


@pytest.mark.parametrize("env", MEMO)
def test_path_records_at_gf_pool(eng, monkeypatch, env):
    """k = 9: a path of k + 2 nodes is a record of 24 ints.  3 sites with 6 alleles: 216 candidates, 432 ints of
    records (handed on for its records, every answer of 144 ints spilled past GM_INLINE); 3 sites with 5 alleles: 125
    candidates, 360 ints (stays)"""
    setenv(monkeypatch, env)
    routes, _ = correct_case(eng, monkeypatch, bubbles(3, 6, 11, first=10, depth=lambda g: 3 + g % 3), 9)
    expect(routes, gapped=1, by_general=1, on_records=1)
    if not env:
        expect(routes, memo_questions=3, memo_spilled=3, memo_unfit=0)
    routes, _ = correct_case(eng, monkeypatch, bubbles(3, 5, 11, first=10, depth=lambda g: 3 + g % 3), 9)
    expect(routes, gapped=1, by_fast=1, by_general=0)


@pytest.mark.parametrize("env", MEMO)
def test_one_answer_beyond_gf_pool(eng, monkeypatch, env):
    """k = 9, one site with 17 alleles: the answer (408 ints) does not fit the searching wave's own staging — with the
    memo that is an answer that "did not fit", without it the read's records overflow"""
    setenv(monkeypatch, env)
    routes, _ = correct_case(eng, monkeypatch, bubbles(1, 17, 11, first=10, depth=lambda g: 3 + g % 2), 9)
    if env:
        expect(routes, gapped=1, by_general=1, on_records=1)
    else:
        expect(routes, gapped=1, by_general=1, on_memo_unfit=1, memo_questions=1, memo_unfit=1)


@pytest.mark.parametrize("env", MEMO)
def test_candidate_length_at_gf_cand(eng, monkeypatch, env):
    """k = 5: reads that lack three stretches of 4 genes (a path of 2k = 10 nodes bridges each).  124 windows + 12
    nodes = 136 = GF_CAND stays; 128 windows + 12 = 140 is handed on after the candidate was being assembled"""
    setenv(monkeypatch, env)
    cuts = [(30, 4), (70, 4), (100, 4)]
    reads = backbone(144, [dict(a=0, b=140, cuts=cuts), dict(a=0, b=144, cuts=cuts)])
    assert len(reads["n000"]) == 128 and len(reads["n001"]) == 132
    routes, r2 = correct_case(eng, monkeypatch, reads, 5)
    assert r2["n000"] == reads["c000"][:140] and r2["n001"] == reads["c000"]
    expect(routes, gapped=2, by_fast=1, by_general=1, on_cand=1, keep_orig=0)


# ------------------------------------------------------------------ GM_INLINE, k = 15 and 16
@pytest.mark.parametrize("k,lean", [(15, 2), (16, 1)])
def test_single_answer_at_gm_inline(eng, monkeypatch, k, lean):
    """a read that lacks k - 1 genes asks a question whose one answer is a path of 2k nodes: 62 ints at k = 15 (inline:
    sixteen lanes finish the read), 66 at k = 16 (spilled: sixteen lanes hand it to the wave); a read with one
    substituted gene (k + 2 nodes) beside it"""
    reads = backbone(60, [dict(a=0, b=60, cuts=[(25, k - 1)]), dict(a=0, b=60, subs=(30,))])
    routes, r2 = correct_case(eng, monkeypatch, reads, k)
    assert r2["n000"] == reads["c000"] and r2["n001"] == reads["c000"]
    expect(routes, gapped=2, by_lean=lean, by_fast=2 - lean, lean_long=2 - lean, memo_spilled=2 - lean, by_general=0)


@pytest.mark.parametrize("k", [15, 16])
def test_alleles_at_large_k(eng, monkeypatch, k):
    """2 sites with 3 alleles at k = 15 / 16: records of 2 + 2 (k + 2) ints, three per question (spilled)"""
    routes, _ = correct_case(eng, monkeypatch, bubbles(2, 3, k + 2, first=k + 1), k)
    expect(routes, gapped=1, by_fast=1, lean_answers=1, memo_questions=2, memo_spilled=2)


@pytest.mark.parametrize("k", [15, 16])
def test_sweep_at_large_k(eng, k):
    from test_gpu_sweep import run_sweep
    reads, pos, fq = P.synth_inputs(41 + k, 500, 60, 300, 0.02)
    run_sweep(eng, reads, pos, fq, k)


# ------------------------------------------------------------------ the two host capacities, through their test hooks
def test_memo_pool_used_up(eng, monkeypatch):
    """AMG_TEST_MEMO_SPILL=200: of the three spilled answers (144 ints each) of test_path_records_at_gf_pool's second
    read set one fits; its read is handed on for an answer that did not fit, same corrected reads"""
    monkeypatch.setenv("AMG_TEST_MEMO_SPILL", "200")
    routes, _ = correct_case(eng, monkeypatch, bubbles(3, 5, 11, first=10, depth=lambda g: 3 + g % 3), 9)
    expect(routes, gapped=1, by_general=1, on_memo_unfit=1, memo_questions=3, memo_unfit=2, memo_spilled=1)


@pytest.mark.parametrize("env", MEMO)
def test_general_pool_grows(eng, monkeypatch, env):
    """AMG_TEST_GAP_POOL=64: the general kernel's first pool cannot hold the 512-candidate read's records: it reports
    the overflow, the host grows the pool and repeats the step"""
    setenv(monkeypatch, env)
    monkeypatch.setenv("AMG_TEST_GAP_POOL", "64")
    routes, _ = correct_case(eng, monkeypatch, bubbles(9, 2, 6, queries=[8, 9]), 5)
    expect(routes, gapped=2, by_fast=1, by_general=1, on_combos=1, pool_retries=1)
    monkeypatch.setenv("AMG_NO_FAST_GAPPED", "1")
    routes, _ = correct_case(eng, monkeypatch, bubbles(3, 6, 11, first=10, depth=lambda g: 3 + g % 3), 9)
    expect(routes, gapped=1, by_general=1, on_not_tried=1, pool_retries=1)


# ------------------------------------------------------------------ dead ends in every tier
@pytest.mark.parametrize("env", MEMO)
def test_dead_ends_in_every_tier(eng, monkeypatch, env):
    """k = 3: a read that lacks 4 genes has a run with no path within 2k nodes: its genes and positions are kept.  In
    a short read (found by the wave-per-read kernel), in a read of 140 windows and in a read of 17 runs (both found
    by the general kernel, behind runs that do have paths); a fourth read is re-threaded as usual"""
    setenv(monkeypatch, env)
    reads = backbone(150, [dict(a=0, b=44, cuts=[(20, 4)]),
                           dict(a=0, b=146, cuts=[(60, 4)], subs=(10, 100, 130)),
                           dict(a=0, b=127, cuts=[(116, 4)], subs=every(111, 7)),
                           dict(a=50, b=90, subs=(70,))])
    routes, r2 = correct_case(eng, monkeypatch, reads, 3)
    for r in ("n000", "n001", "n002"):
        assert r2[r] == reads[r]
    assert r2["n003"] == reads["c000"][50:90]
    expect(routes, gapped=4, keep_orig=3, by_general=2, on_windows=1, on_runs=1, nw_fast=1, nw_lds=0, nw_global=0)


# ------------------------------------------------------------------ position carry-over
@pytest.mark.parametrize("env", MEMO)
def test_carry_over_at_nwf_max_m(eng, monkeypatch, env):
    """corrected and original reads of 64 genes (the wave-per-read carry-over) and of 65 (general kernel, LDS matrix);
    60 and 61 windows: with the memo both are staged by the sixteen-lanes kernel, without it by the wave-per-read
    kernel's own search"""
    setenv(monkeypatch, env)
    reads = backbone(65, [dict(a=0, b=64, subs=every(58, 9)), dict(a=0, b=65, subs=every(59, 9, 7))])
    routes, r2 = correct_case(eng, monkeypatch, reads, 5)
    assert r2["n000"] == reads["c000"][:64] and r2["n001"] == reads["c000"]
    expect(routes, gapped=2, nw_fast=1, nw_lds=1, nw_global=0, by_general=0)
    if env:
        expect(routes, by_fast=2, by_lean=0, no_memo_slots=2)
    else:
        expect(routes, by_lean=2, by_fast=0, no_memo_slots=0)


@pytest.mark.parametrize("env", MEMO)
def test_carry_over_at_nw_lds_cells(eng, monkeypatch, env):
    """128 x 128 = 16 384 cells fit the LDS matrix, 129 x 129 take the global scratch"""
    setenv(monkeypatch, env)
    reads = backbone(129, [dict(a=0, b=128, subs=every(122, 9)), dict(a=0, b=129, subs=every(123, 9, 7))])
    routes, _ = correct_case(eng, monkeypatch, reads, 5)
    expect(routes, gapped=2, by_fast=2, nw_fast=0, nw_lds=1, nw_global=1)


@pytest.mark.parametrize("n_genes,n_err", [(1100, 20), (2000, 30)])
def test_carry_over_beyond_nw_lds_n(eng, monkeypatch, n_genes, n_err):
    """a read of more than 1 024 genes: the general re-threading kernel, then a pointer matrix of 1.2 M / 4 M cells in
    global scratch"""
    subs = tuple(int(x) for x in np.linspace(8, n_genes - 9, n_err).astype(int))
    reads = backbone(n_genes, [dict(a=0, b=n_genes, subs=subs)])
    routes, r2 = correct_case(eng, monkeypatch, reads, 5)
    assert r2["n000"] == reads["c000"]
    expect(routes, gapped=1, by_general=1, on_windows=1, nw_global=1)


def test_gap_placement_tie_in_every_carry_over(eng, monkeypatch):
    """the genome has the same gene twice in a row and a read lacks one of the two: the corrected read has one gene
    more than the original, and the gap may sit against either copy at the same score.  The reference's tie order
    (UP > LEFT > DIAG) decides which copy keeps the original position and which gets a repaired one.  Reads of 39, 99
    and 139 original genes: the wave-per-read carry-over, the general kernel with its LDS matrix, and with global
    scratch"""
    reads = backbone(150, [dict(a=0, b=40, cuts=[(21, 1)]), dict(a=0, b=100, cuts=[(51, 1)], subs=(20,)),
                           dict(a=5, b=145, cuts=[(111, 1)], subs=(30, 60))], twice=(20, 50, 110))
    routes, r2 = correct_case(eng, monkeypatch, reads, 5)
    assert r2["n000"] == reads["c000"][:40] and r2["n001"] == reads["c000"][:100] and r2["n002"] == reads["c000"][5:145]
    expect(routes, gapped=3, nw_fast=1, nw_lds=1, nw_global=1, keep_orig=0)


@pytest.mark.parametrize("seed,k,lengths", [(3, 3, (62, 64, 66, 126, 128, 130)), (4, 5, (63, 65, 70, 127, 129, 135))])
def test_ties_beyond_the_fast_carry_over(eng, monkeypatch, seed, k, lengths):
    """tandem arrays in reads of 62 .. 135 genes: near-periodic gene lists whose alignments tie, carried over by the
    general kernel (its tie order UP > LEFT > DIAG decides); first correction with the route report, then the whole
    sweep"""
    from test_gpu_sweep import run_sweep
    reads, pos, fq = tandem_reads(seed, 240, lengths, 0.04)
    routes, _ = correct_case(eng, monkeypatch, reads, k)
    expect(routes, nw_lds_min=1, nw_global_min=1, nw_fast_min=1)
    run_sweep(eng, reads, pos, fq, k)


# ------------------------------------------------------------------ one chunk of the wave-per-read kernel, mixed
@pytest.mark.parametrize("env", MEMO)
def test_mixed_chunk(eng, monkeypatch, env):
    """fewer than LEAN_CHUNK = 32 re-threaded reads, so one workgroup of the wave-per-read kernel meets them all:
    reads the sixteen lanes finished, reads it finishes itself, reads it hands on (windows, runs, combinations) and
    reads that keep their genes, interleaved in read order"""
    setenv(monkeypatch, env)
    k = 5
    genome = [f"+g{i}" for i in range(140)]
    sites = {5 + 6 * s: s for s in range(9)}
    alt = [f"+alt{sites[i]}" if i in sites else genome[i] for i in range(60)]
    special = [noisy(genome, 0, 133, subs=every(127, 11), tag="w"),                       # 129 windows
               noisy(genome, 30, 138, subs=tuple(35 + 6 * i for i in range(17)), tag="r"),  # 17 runs, 104 windows
               [f"+u{sites[i]}" if i in sites else genome[i] for i in range(60)],          # 512 candidates
               noisy(genome, 0, 46, cuts=[(20, 6)], tag="d"),                              # dead end: genes kept
               noisy(genome, 40, 130, subs=(60, 100), tag="f"),                            # 86 windows: the wave's own
               noisy(genome, 70, 116, cuts=[(90, 6)], tag="e")]                            # dead end
    reads = {}
    for j, s in enumerate(special):
        for c in range(3):  # ordinary short reads, one substituted gene each
            a = 62 + (7 * (3 * j + c)) % 48
            reads[f"m{j}_{c}"] = noisy(genome, a, a + 30, subs=(a + 12 + c,), tag=f"o{j}{c}_")
        reads[f"m{j}_s"] = s
    for c in range(5):
        reads[f"c{c:03d}"] = list(genome)
    for c in range(4):
        reads[f"alt{c}"] = list(alt)
    routes, r2 = correct_case(eng, monkeypatch, reads, k)
    assert r2["m3_s"] == reads["m3_s"] and r2["m5_s"] == reads["m5_s"] and r2["m0_s"] == genome[:133]
    assert routes["gapped"] == 24 and routes["gapped"] <= 32
    expect(routes, keep_orig=2, on_windows=1, on_runs=1, on_combos=1, by_general=3, by_fast_min=3)
    if not env:
        expect(routes, by_lean=18)
