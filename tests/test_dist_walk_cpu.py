"""CPU: what the drivers of the read walks across ranks (amira_amd/dist.py) do with the answers — the mean rule shared
with get_overall_mean_node_coverages, the 80 % rule and the early break of k selection — against engines that return
canned answers.  No GPU: the walks themselves are tested in tests/test_gpu_dist_walk.py."""
import statistics

import numpy as np
import pytest

from amira_amd import _ffi, dist
from amira_amd.graph_utils import components_valid, mean_of_ints


@pytest.mark.parametrize("values", [[6, 6, 6, 6], [1, 2], [1, 1, 2], [0, 0, 0], [7], [10 ** 17, 1, 1], [3, 3, 4, 5, 5, 5, 9],
                                    [2 ** 53, 2 ** 53, 1]])
def test_mean_rule_is_statistics_mean(values):
    got, want = mean_of_ints(sum(values), len(values)), statistics.mean(values)
    assert got == want and type(got) is type(want)


def test_mean_of_no_node_is_zero():
    assert mean_of_ints(0, 0) == 0 and type(mean_of_ints(0, 0)) is int
    assert mean_of_ints(np.int64(12), np.int64(4)) == 3 and type(mean_of_ints(np.int64(12), np.int64(4))) is int


def test_eighty_percent_rule():
    assert components_valid([], [])
    assert components_valid([0, 5, 10], [0, 4, 8])           # exactly 80 %; a component without reads is valid
    assert not components_valid([0, 5, 10], [0, 3, 10])
    assert not components_valid([1], [0])


class FakeEngine:
    """answers dist_walk_local from canned tables; `k` is what the last (fake) merged build was asked for"""
    def __init__(self, log, depth=None, comp=None):
        self.log, self.depth, self.comp, self.k = log, depth, comp, None

    @staticmethod
    def dist_walk_local(engines, which, flags, min_genes):
        e = engines[0]
        assert all(x.k == e.k for x in engines)
        e.log.append((which, None if min_genes is None else list(min_genes)))
        if which == _ffi.WALK_DEPTH:
            pairs, n_alive = e.depth
            assert list(min_genes) == list(range(3, 16, 2))
            return np.asarray(list(pairs) + [n_alive], np.int64)
        if which == _ffi.WALK_COMPONENT_READS:
            assert list(min_genes) == [2 * e.k - 1]
            n_reads, n_long = e.comp[e.k]
            return np.asarray(list(n_reads) + list(n_long), np.int64)
        return np.asarray([4], np.int64)


def fake_ranks(monkeypatch, **kw):
    log = []
    engines = [FakeEngine(log, **kw) for _ in range(3)]

    def build(engs, k, *thresholds):
        log.append(("build", k))
        for e in engs:
            e.k = k
    monkeypatch.setattr(dist, "dist_build_loopback", build)
    return engines, log


def test_mean_node_coverages_from_partial_sums(monkeypatch):
    engines, _ = fake_ranks(monkeypatch, depth=([24, 12, 7, 5, 1, 0, 0], 4))
    got = dist.dist_mean_node_coverages_loopback(engines)
    assert got == {3: 6, 5: 3, 7: 1.75, 9: 1.25, 11: 0.25, 13: 0, 15: 0}
    assert [type(got[k]) for k in (3, 5, 7, 13)] == [int, int, float, int]
    engines, _ = fake_ranks(monkeypatch, depth=([0] * 7, 0))
    assert dist.dist_mean_node_coverages_loopback(engines) == {k: 0 for k in range(3, 16, 2)}
    pairs, n_alive = dist.dist_depth_by_length_loopback(engines, list(range(3, 16, 2)))
    assert pairs.tolist() == [0] * 7 and n_alive == 0
    assert dist.dist_remove_non_amr_nodes_loopback(engines, np.ones(3, np.uint8)) == 4


def test_choose_kmer_size_rule_and_early_break(monkeypatch):
    ok, bad = ([0, 10, 5], [0, 8, 5]), ([0, 10, 5], [0, 7, 5])      # a component without reads; 80 % exactly; 70 %
    # valid at 3, 5, 7, not at 9: the search ends there although 11 would be valid again
    engines, log = fake_ranks(monkeypatch, comp={3: ok, 5: ok, 7: ok, 9: bad, 11: ok, 13: ok, 15: ok})
    assert dist.dist_choose_kmer_size_loopback(engines, 20, None) == 7
    assert [x[1] for x in log if x[0] == "build"] == [3, 5, 7, 9]
    assert [x for x in log if x[0] != "build"] == [(_ffi.WALK_COMPONENT_READS, [2 * k - 1]) for k in (3, 5, 7, 9)]
    # valid everywhere (and a graph without components): 15 after seven builds
    engines, log = fake_ranks(monkeypatch, comp={k: ([], []) if k == 15 else ok for k in range(3, 16, 2)})
    assert dist.dist_choose_kmer_size_loopback(engines, 25.0, None) == 15 and len(log) == 14
    # not valid at 3: the answer is still 3, after one build
    engines, log = fake_ranks(monkeypatch, comp={3: bad})
    assert dist.dist_choose_kmer_size_loopback(engines, 20, None) == 3 and log[0] == ("build", 3) and len(log) == 2
    # a mean coverage below 20: no build at all
    engines, log = fake_ranks(monkeypatch, comp={})
    assert dist.dist_choose_kmer_size_loopback(engines, 19.99, None) == 3 and log == []
