"""bench.py --dump-outputs (bench.dump_outputs) on a stand-in for the engine: what it writes is exact, within the
budget, and the same sample from run to run.  CPU only."""
import os

import numpy as np

import bench


class FakeEngine:
    """the read-back calls dump_outputs makes, on arrays of the engine's dtypes"""

    def __init__(self, n_nodes, n_edges, n_tokens, k=5, seed=1):
        rng = np.random.default_rng(seed)
        self.k, self.n_tokens = k, n_tokens
        self._nodes = {"tokens": rng.integers(0, 40_000, (n_nodes, k), dtype=np.int32),
                       "coverage": rng.integers(1, 500, n_nodes).astype(np.uint32),
                       "first_token": np.sort(rng.choice(n_tokens, n_nodes, replace=False)).astype(np.int64),
                       "first_dir": rng.choice(np.array([-1, 1], np.int8), n_nodes),
                       "component": rng.integers(0, n_nodes, n_nodes, dtype=np.int32),
                       "alive": rng.integers(0, 2, n_nodes).astype(np.uint8)}
        self._edges = {"src": rng.integers(0, n_nodes, n_edges, dtype=np.int32),
                       "tgt": rng.integers(0, n_nodes, n_edges, dtype=np.int32),
                       "sdir": rng.choice(np.array([-1, 1], np.int8), n_edges),
                       "tdir": rng.choice(np.array([-1, 1], np.int8), n_edges),
                       "coverage": rng.integers(1, 500, n_edges).astype(np.uint32),
                       "alive": np.ones(n_edges, np.uint8)}
        self._tok_node = rng.integers(-2, n_nodes, n_tokens, dtype=np.int32)
        self._tok_dir = rng.choice(np.array([-1, 0, 1], np.int8), n_tokens)

    def sizes(self):
        return 1000, self.n_tokens

    def graph_sizes(self):
        return len(self._nodes["alive"]), len(self._edges["src"]), self.k

    def nodes(self):
        return self._nodes

    def edges(self):
        return self._edges

    def read_nodes(self):
        return self._tok_node, self._tok_dir


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_small_outputs_are_written_whole_and_exact(tmp_path):
    eng = FakeEngine(300, 700, 5000)
    bench.dump_outputs(eng, str(tmp_path), seed=3)
    got = _load(tmp_path)
    assert not any(name.endswith("_rows") for name in got)
    assert got["sizes"].tolist() == [1000, 5000, 300, 700, 5]
    for c, a in eng.nodes().items():
        assert got["node_" + c].dtype == np.float32 and np.array_equal(got["node_" + c], a)
    for c, a in eng.edges().items():
        assert got["edge_" + c].dtype == np.float32 and np.array_equal(got["edge_" + c], a)
    assert np.array_equal(got["window_node"], eng._tok_node) and np.array_equal(got["window_dir"], eng._tok_dir)


def test_large_outputs_are_a_fixed_sample_within_the_budget(tmp_path):
    eng = FakeEngine(20_000, 50_000, 400_000)
    eng._nodes["first_token"] += 1 << 25   # beyond float32's exact integers
    budget = 1_000_000
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(eng, str(a), seed=3, budget=budget)
    bench.dump_outputs(eng, str(b), seed=3, budget=budget)
    assert sum(os.path.getsize(os.path.join(a, f)) for f in os.listdir(a)) <= budget
    got, again = _load(a), _load(b)
    assert got.keys() == again.keys()
    assert all(np.array_equal(got[n], again[n]) for n in got)
    assert got["node_first_token"].dtype == np.float64
    for group, src in (("node", eng.nodes()), ("edge", eng.edges())):
        rows = got[group + "_rows"].astype(np.int64)
        assert len(rows) > 0 and np.all(np.diff(rows) > 0)
        for c, arr in src.items():
            assert np.array_equal(got[f"{group}_{c}"], arr[rows])
    rows = got["window_rows"].astype(np.int64)
    assert np.array_equal(got["window_node"], eng._tok_node[rows])

    # a later dump that fits leaves no row index of the earlier sample behind
    bench.dump_outputs(FakeEngine(30, 70, 500), str(a), seed=3, budget=budget)
    assert not any(f.endswith("_rows.npy") for f in os.listdir(a))
