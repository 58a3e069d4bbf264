"""The junction path search of bubble popping on ARBITRARY graphs: a plain reference (numpy and Python, nothing of the
product) and the graphs it is asked about, as graph_shapes.Shapes (gene-mer size 1: a read of two genes is one edge).

The reference works on the edge arrays src, tgt, sdir, tdir (token_oracle.Sweep(...).edges(), Engine.edges()) and the
alive bytes of edges and nodes:

  rows        row 2 * src holds the live edges with sdir > 0, row 2 * src + 1 the others, in ascending edge id;
  junctions   rows of live nodes with more than one live edge, ascending: row 2n is (n, +1), row 2n + 1 is (n, -1);
  search      depth first from a start junction (n, s): a node taken in direction +1 is left through its forward row
              (2n), in -1 through its backward row, in row order; the next node is taken in the edge's tdir; no node
              twice on a path; a node is entered while the path has at most `distance` nodes and a path of exactly
              `distance` nodes is not extended; every entered node other than the start whose row on the ARRIVAL side
              (direction +1 arrives through the backward row) is a junction gives a record (stop junction, path so far);
  output      per start in junction order, its stops in junction order, a stop's records in search order, stops with
              fewer than two records dropped: the arrays of Engine.junction_paths;
  multi       some entered node (not the start) is a junction on either side and has more than one live edge, in
              either direction, between it and the node before it on the path;
  enters[j]   nodes entered from start j, the start included.

tests/test_junction_search_cpu.py holds all of this to the Python oracle."""
from collections import namedtuple

import numpy as np

from graph_shapes import Shape, _pairs

Found = namedtuple("Found", "junction_node junction_dir path_start path_off path_node path_dir multi enters "
                            "stops_per_start other_side_only")
ARRAYS = ("junction_node", "junction_dir", "path_start", "path_off", "path_node", "path_dir")


# ------------------------------------------------------------------ liveness, rows, junctions
def live_after(edges, n_nodes, dead_nodes=(), dead_edges=(), edge_alive=None, node_alive=None):
    """(edge alive, node alive) bytes after removals: an edge is dead when it was removed or either end is dead"""
    na = np.ones(n_nodes, np.uint8) if node_alive is None else np.array(node_alive, np.uint8)
    ea = np.ones(len(edges["src"]), np.uint8) if edge_alive is None else np.array(edge_alive, np.uint8)
    na[np.asarray(dead_nodes, np.int64)] = 0
    ea[np.asarray(dead_edges, np.int64)] = 0
    ea[(na[edges["src"]] == 0) | (na[edges["tgt"]] == 0)] = 0
    return ea, na


def live_rows(edges, edge_alive, n_nodes):
    """(off[2 n_nodes + 1], ids): row r holds the live edge ids ids[off[r]:off[r + 1]], ascending"""
    live = np.flatnonzero(np.asarray(edge_alive) != 0)
    row = 2 * edges["src"][live].astype(np.int64) + (edges["sdir"][live] <= 0)
    ids = live[np.argsort(row, kind="stable")]
    off = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=2 * n_nodes))]).astype(np.int64)
    return off, ids


def junction_rows(edges, edge_alive, node_alive):
    off, _ = live_rows(edges, edge_alive, len(node_alive))
    return np.flatnonzero((np.diff(off) > 1) & np.repeat(np.asarray(node_alive) != 0, 2))


# ------------------------------------------------------------------ the search
def search(edges, edge_alive, node_alive, distance):
    src, tgt, tdir = edges["src"].tolist(), edges["tgt"].tolist(), edges["tdir"].tolist()
    D = len(node_alive)
    off, ids = live_rows(edges, edge_alive, D)
    off_l, ids_l = off.tolist(), ids.tolist()
    row = [[(tgt[e], tdir[e]) for e in ids_l[off_l[r]:off_l[r + 1]]] for r in range(2 * D)]
    between = {}                                    # live edges from a to b, either row
    for e in ids_l:
        between[src[e], tgt[e]] = between.get((src[e], tgt[e]), 0) + 1
    jrows = junction_rows(edges, edge_alive, node_alive).tolist()
    index = {r: j for j, r in enumerate(jrows)}
    multi, other_side_only = False, 0
    enters, stops_per_start = [], []
    p_start, p_off, p_node, p_dir = [], [0], [], []
    for j, r0 in enumerate(jrows):
        start = (r0 >> 1, -1 if r0 & 1 else 1)
        path, on, entered, records = [start], {start[0]}, 1, []
        walks = [iter(row[r0])]
        while walks:
            step = next(walks[-1], None)
            if step is None:
                walks.pop()
                on.discard(path.pop()[0])
                continue
            t, d = step
            if t in on:
                continue
            path.append(step)
            entered += 1
            arrival, other = 2 * t + (1 if d == 1 else 0), 2 * t + (0 if d == 1 else 1)
            if arrival in index or other in index:
                prev = path[-2][0]
                if between.get((prev, t), 0) > 1 or between.get((t, prev), 0) > 1:
                    multi = True
                if arrival in index:
                    records.append((index[arrival], list(path)))
                else:
                    other_side_only += 1
            if len(path) >= distance:
                path.pop()
            else:
                on.add(t)
                walks.append(iter(row[2 * t + (0 if d == 1 else 1)]))
        enters.append(entered)
        stops_per_start.append(len({s for s, _ in records}))
        by_stop = {}
        for s, p in records:
            by_stop.setdefault(s, []).append(p)
        for s in sorted(by_stop):
            if len(by_stop[s]) < 2:
                continue
            for p in by_stop[s]:
                p_start.append(j)
                p_node += [n for n, _ in p]
                p_dir += [x for _, x in p]
                p_off.append(len(p_node))
    jr = np.asarray(jrows, np.int64)
    return Found((jr >> 1).astype(np.int32), np.where(jr & 1, -1, 1).astype(np.int8), np.asarray(p_start, np.int32),
                 np.asarray(p_off, np.int64), np.asarray(p_node, np.int32), np.asarray(p_dir, np.int8), multi,
                 np.asarray(enters, np.int64), np.asarray(stops_per_start, np.int64), other_side_only)


def paths_of(found):
    """[(start junction index, [(node, direction), ...]), ...] in output order"""
    off, n, d = found.path_off.tolist(), found.path_node.tolist(), found.path_dir.tolist()
    return [(j, list(zip(n[off[p]:off[p + 1]], d[off[p]:off[p + 1]]))) for p, j in enumerate(found.path_start.tolist())]


def self_loop_junctions(edges, edge_alive, node_alive):
    """junction rows that would not be one without their self-loops"""
    rows = junction_rows(edges, edge_alive, node_alive)
    no_loops = np.asarray(edge_alive) * (edges["src"] != edges["tgt"])
    return np.setdiff1d(rows, junction_rows(edges, no_loops, node_alive))


def row_changes(edges, n_nodes, before, after):
    """before, after: (edge alive, node alive).  (junction rows that lost their first entry and stayed junctions,
    rows that fell from three or more entries to exactly one and so left the junction list)"""
    off0, ids0 = live_rows(edges, before[0], n_nodes)
    off1, _ = live_rows(edges, after[0], n_nodes)
    was, now = junction_rows(edges, *before), set(junction_rows(edges, *after).tolist())
    lost_first = [r for r in was.tolist() if r in now and after[0][ids0[off0[r]]] == 0]
    fell = [r for r in was.tolist() if r not in now and off0[r + 1] - off0[r] >= 3 and off1[r + 1] - off1[r] == 1
            and after[1][r >> 1] != 0]
    return lost_first, fell


# ------------------------------------------------------------------ shapes
def _node_strands(D, pairs, seed):
    """one seeded strand per NODE, each read given from either end: (a, b) on (s_a, s_b) or (b, a) on (-s_b, -s_a) —
    the same edge, so every path of the all-'+' graph is still a path, through rows and directions that vary"""
    rng = np.random.default_rng(seed)
    s = np.where(rng.integers(0, 2, D) == 1, 1, -1)
    flip = rng.integers(0, 2, len(pairs)) == 1
    a, b = pairs[:, 0], pairs[:, 1]
    return (np.where(flip[:, None], pairs[:, ::-1], pairs),
            np.where(flip[:, None], np.stack([-s[b], -s[a]], 1), np.stack([s[a], s[b]], 1)))


def _plus(D, pairs, strand_seed):
    pairs = _pairs(pairs)
    if strand_seed is None:
        return Shape(D, pairs, np.ones((len(pairs), 2), np.int64), True)
    pairs, strands = _node_strands(D, pairs, strand_seed)
    return Shape(D, pairs, strands, True)


def ladder(rail_a=62, rail_b=62, tail=3, strand_seed=None):
    """tail -> S -> two rails of rail_a and rail_b nodes -> T -> tail; ids: the first tail, S, rail a, rail b, T, the
    second tail.  S .. T over rail x is rail_x + 2 nodes.  Returns (Shape, S, T)"""
    S = tail
    a0, b0 = S + 1, S + 1 + rail_a
    T = b0 + rail_b
    D = T + 1 + tail
    chain = lambda ids: [(ids[i], ids[i + 1]) for i in range(len(ids) - 1)]    # noqa: E731
    pairs = (chain(list(range(0, S + 1))) + chain([S] + list(range(a0, a0 + rail_a)) + [T])
             + chain([S] + list(range(b0, b0 + rail_b)) + [T]) + chain(list(range(T, D))))
    return _plus(D, pairs, strand_seed), S, T


def random_pairs(D, n_pairs, n_loops, seed, repeats=0, times=None, low_ends=False):
    """n_pairs distinct unordered pairs of different nodes and n_loops self-loops, every end on a seeded random strand;
    repeats: that many of the pairs given once more with the strand of ONE end turned, (a, b) on (s_a, -s_b): the
    other class of the same pair of ids, a second edge between the two nodes (turning both strands gives the same edge
    again).  The two edges share a row at one end — which one, the stored orientations decide — and sit one in each
    row at the other.  The first end is therefore always a junction, and the search from it enters the second end as
    its second node: `multi` is true at every distance unless the second end of every repeated pair has no other edge.
    low_ends: the repeated pairs are not seeded random ones but those whose ends have the fewest other edges, so that
    both answers occur;
    times: (lo, hi) — every read given lo .. hi times"""
    rng = np.random.default_rng(seed)
    all_pairs = np.stack(np.triu_indices(D, 1), 1)
    pairs = all_pairs[rng.permutation(len(all_pairs))[:n_pairs]]
    pairs = np.where((rng.integers(0, 2, n_pairs) == 1)[:, None], pairs[:, ::-1], pairs)
    loops = rng.integers(0, D, n_loops)
    pairs = np.concatenate([pairs, _pairs(loops, loops)])
    strands = np.where(rng.integers(0, 2, (len(pairs), 2)) == 1, 1, -1)
    if repeats:
        again = rng.permutation(n_pairs)[:repeats]
        if low_ends:
            degree = np.bincount(pairs[:n_pairs].reshape(-1), minlength=D)
            again = np.argsort(degree[pairs[:n_pairs]].min(1), kind="stable")[:repeats]
        pairs = np.concatenate([pairs, pairs[again]])
        strands = np.concatenate([strands, strands[again] * np.array([1, -1])])
    if times is not None:
        t = rng.integers(times[0], times[1] + 1, len(pairs))
        pairs, strands = np.repeat(pairs, t, axis=0), np.repeat(strands, t, axis=0)
    return Shape(D, pairs, strands)


def dead_end_pair(turn):
    """node 0 hangs on node 1 by two edges, (0, 1) on (+, +) and on (+, -) (turn = 1) or (-, +) (turn = 0), and has no
    other edge; behind node 1 a bubble 1 -> {2, 3} -> 4.  At the end where the two edges share a row they make a
    junction; where that end is node 1, node 0 is entered over two edges and is no junction: `multi` stays false"""
    pairs = [(0, 1), (0, 1), (1, 2), (1, 3), (2, 4), (3, 4)]
    strands = np.ones((6, 2), np.int64)
    strands[1, turn] = -1
    return Shape(5, _pairs(pairs), strands, True)


def bubble_chain(n):
    """n two-way bubbles S -> {a, b} -> T -> link -> the next S: 5 n nodes, 2 n junctions ((S, +1) and (T, -1))"""
    base = 5 * np.arange(n)[:, None]
    inside = np.array([[0, 1], [0, 2], [1, 3], [2, 3], [3, 4]])
    pairs = (base[:, :, None] + inside[None]).reshape(-1, 2)
    links = np.stack([5 * np.arange(n - 1) + 4, 5 * np.arange(1, n)], 1)
    return _plus(5 * n, np.concatenate([pairs, links]), None)


def layered(layers=8, width=3):
    """one start, then `layers` layers of `width` nodes, each layer fully joined to the next"""
    pairs = [(0, 1 + w) for w in range(width)]
    for l in range(layers - 1):
        pairs += [(1 + l * width + a, 1 + (l + 1) * width + b) for a in range(width) for b in range(width)]
    return _plus(1 + layers * width, pairs, None)


# ------------------------------------------------------------------ the cases of the tests
SEEDS = tuple(range(12))
DISTINCT = [(40, d) for d in (2, 3, 6, 10)] + [(30, 5)]     # (D, distance) of the distinct-pair family, 60 pairs each


def distinct_pairs(D, seed):
    return random_pairs(D, 60, 2 if D == 40 else 0, 1000 + 50 * D + seed)


def repeated_pairs(D, seed):
    """odd seeds: the three pairs with the lowest-degree ends repeated; even seeds: three seeded random ones"""
    return random_pairs(D, 60, 2 if D == 40 else 0, 1000 + 50 * D + seed, repeats=3, low_ends=seed % 2 == 1)


def weighted_pairs(seed):
    return random_pairs(40, 60, 2, 5000 + seed, times=(1, 3))
