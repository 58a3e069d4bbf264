"""Arbitrary graphs as read sets, for the component labellers and what reads their labels.

At gene-mer size 1 every gene is a node whatever its strand, and a read of two genes is one edge.  A prefix of D reads
of one gene each fixes the first-seen ids (node g = gene rank g); what follows can be any edge list in any order.  A
shape is (D, pairs): pairs an int array [P, 2] over the node ids 0 .. D - 1, a row per read, repeats and (g, g) allowed.
The makers return a Shape, which adds what two of them need: fixed strands, and a read order that is kept.

labels() is the reference: numpy alone, nothing of the kernels' hooks, halving or run links."""
from collections import namedtuple

import numpy as np

# strands: None (seeded random) or int [P, 2] of +1 / -1; ordered: the pair reads stay in the order given
Shape = namedtuple("Shape", "D pairs strands ordered", defaults=(None, False))


def _pairs(a, b=None):
    if b is None:
        return np.asarray(a, np.int64).reshape(-1, 2)
    return np.stack([np.asarray(a, np.int64), np.asarray(b, np.int64)], 1).reshape(-1, 2)


# ------------------------------------------------------------------ reads
def as_tokens(D, pairs, seed, strands=None, ordered=False):
    """(tokens int32, read_offsets int64, two_v) with V = D: D reads of one token, V + g for g = 0 .. D - 1, then one
    read of two tokens per pair, each gene on a seeded random strand (V + g or V - 1 - g) unless `strands` fixes them,
    in a seeded random read order unless `ordered`"""
    V = int(D)
    pairs = _pairs(pairs)
    n = len(pairs)
    assert V >= 1 and (n == 0 or (0 <= pairs.min() and pairs.max() < V))
    rng = np.random.default_rng(seed)
    plus = rng.integers(0, 2, (n, 2)) == 1 if strands is None else np.asarray(strands).reshape(n, 2) > 0
    order = np.arange(n) if ordered else rng.permutation(n)
    two = np.where(plus, V + pairs, V - 1 - pairs)[order]
    tokens = np.concatenate([V + np.arange(V, dtype=np.int64), two.reshape(-1)]).astype(np.int32)
    read_off = np.concatenate([np.arange(V, dtype=np.int64), V + 2 * np.arange(n + 1, dtype=np.int64)])
    return tokens, read_off, 2 * V


def as_reads(D, pairs, seed, strands=None, ordered=False):
    """the read set of as_tokens as {read id: ["+name" / "-name", ...]} in the same order (small D: for
    amira_amd.tokenize and the Python oracle); gene g is called g<g>"""
    tokens, off, _ = as_tokens(D, pairs, seed, strands, ordered)
    names = [("+g%d" % (t - D)) if t >= D else ("-g%d" % (D - 1 - t)) for t in tokens.tolist()]
    return {"r%d" % r: names[off[r]:off[r + 1]] for r in range(len(off) - 1)}


def shape_tokens(shape, seed):
    return as_tokens(shape.D, shape.pairs, seed, shape.strands, shape.ordered)


def shape_reads(shape, seed):
    return as_reads(shape.D, shape.pairs, seed, shape.strands, shape.ordered)


# ------------------------------------------------------------------ the reference
def labels(D, pairs):
    """(component[D] int32, n_components): component id = 1 + rank of the component's smallest node id among those
    minima.  Every node carries the smallest id it has heard of: each round every pair hands the smaller of its two
    ends' values to the node that the larger one names, then every node jumps to the value of the node its value
    names, until nothing moves."""
    pairs = _pairs(pairs)
    low = np.arange(D, dtype=np.int64)
    a, b = pairs[:, 0], pairs[:, 1]
    while len(pairs):
        la, lb = low[a], low[b]
        if np.array_equal(la, lb):
            break
        np.minimum.at(low, np.maximum(la, lb), np.minimum(la, lb))
        while True:
            nxt = low[low]
            if np.array_equal(nxt, low):
                break
            low = nxt
    is_min = low == np.arange(D)
    rank = np.cumsum(is_min) - 1
    return (rank[low] + 1).astype(np.int32), int(is_min.sum())


# ------------------------------------------------------------------ shapes
def consecutive_joins(pairs):
    pairs = _pairs(pairs)
    return int((np.abs(pairs[:, 0] - pairs[:, 1]) == 1).sum())


def _chain_order(ids, rng):
    """a seeded order of ids in which no two neighbours are consecutive ids (where one exists: the best of 64 draws)"""
    best = None
    for _ in range(64):
        p = rng.permutation(ids)
        bad = int((np.abs(np.diff(p)) == 1).sum())
        if best is None or bad < best[0]:
            best = (bad, p)
        if bad == 0:
            break
    return best[1]


def shuffled_chain(D, seed):
    """(p[i], p[i + 1]) over a permutation p: no pair joins consecutive ids, so the run pre-link does nothing, every
    pair goes through the union kernel and the trees are deep before halving"""
    p = _chain_order(np.arange(D), np.random.default_rng(seed))
    return Shape(D, _pairs(p[:-1], p[1:]))


def ascending_chain(D, seed=0):
    """(i, i + 1): all one run, nothing is left for the union kernel"""
    return Shape(D, _pairs(np.arange(D - 1), np.arange(1, D)))


def runs_and_bridges(D, seed):
    """runs of consecutive ids of length 1 .. 300 (short ones more often: about 4 500 runs at D = 200 000), half of
    the runs bridged to another run between random members: thousands of components made of runs"""
    rng = np.random.default_rng(seed)
    lens = 1 + (300 * rng.random(D) ** 6).astype(np.int64)
    lens = lens[:int(np.searchsorted(np.cumsum(lens), D, side="left")) + 1]
    start = np.concatenate([[0], np.cumsum(lens)[:-1]])
    lens[-1] = D - start[-1]
    R = len(lens)
    inside = np.ones(D, bool)
    inside[start] = False                                   # (i - 1, i) for every i that does not start a run
    i = np.flatnonzero(inside)
    if R < 2:
        return Shape(D, _pairs(i - 1, i))
    src = rng.permutation(R)[:R // 2]
    dst = (src + 1 + rng.integers(0, R - 1, len(src))) % R  # another run
    ba = start[src] + rng.integers(0, 1 << 30, len(src)) % lens[src]
    bb = start[dst] + rng.integers(0, 1 << 30, len(dst)) % lens[dst]
    return Shape(D, np.concatenate([_pairs(i - 1, i), _pairs(ba, bb)]))


def star(D, hub, leaves, seed):
    """`leaves` other nodes joined to one hub, either way round: every hook contends on one root (hub = 0: it is the
    root from the start; hub = D - 1: it is hooked under ever smaller leaves); the other nodes stay isolated"""
    rng = np.random.default_rng(seed)
    others = np.delete(np.arange(D), hub)
    leaf = rng.permutation(others)[:leaves]
    flip = rng.integers(0, 2, len(leaf)) == 1
    hubs = np.full(len(leaf), hub)
    return Shape(D, _pairs(np.where(flip, leaf, hubs), np.where(flip, hubs, leaf)))


def triples(D, seed=0, repeat=None):
    """paths (i, i + D/3, i + 2 D/3): D/3 components of non-consecutive members (and D mod 3 isolated nodes).
    repeat: times the two reads of path i are given (int per path; default 1)"""
    n = D // 3
    i = np.arange(n)
    pairs = np.concatenate([_pairs(i, i + n), _pairs(i + n, i + 2 * n)])
    if repeat is not None:
        pairs = np.repeat(pairs, np.concatenate([repeat, repeat]), axis=0)
    return Shape(D, pairs)


def sparse_random(D, seed):
    """D / 2 uniformly random pairs, self-loops and repeats left in: an emerging giant component, many small ones,
    isolated nodes"""
    rng = np.random.default_rng(seed)
    return Shape(D, rng.integers(0, D, (D // 2, 2)))


def late_bridge(D, seed):
    """two shuffled chains over the halves of a permutation, joined by the very last read"""
    rng = np.random.default_rng(seed)
    p = rng.permutation(D)
    h = D // 2
    x, y = _chain_order(p[:h], rng), _chain_order(p[h:], rng)
    chains = np.concatenate([_pairs(x[:-1], x[1:]), _pairs(y[:-1], y[1:])])
    chains = chains[rng.permutation(len(chains))]
    bridge = _pairs([x[len(x) // 2]], [y[len(y) // 2]]) if h >= 1 else _pairs([])
    return Shape(D, np.concatenate([chains, bridge]), None, True)


def both_signs(D, seed, n=3000):
    """n pairs of consecutive ids and n random pairs, each given as (+a, +b) and as (-b, -a) — one edge met from both
    ends; n more given as (+a, +b) and (+a, -b) — the two classes of one pair of ids; and (g, g) reads on one strand
    and on both"""
    rng = np.random.default_rng(seed)
    n = min(n, max(D // 8, 0))
    if D < 2 or n == 0:
        return Shape(D, _pairs([]), np.zeros((0, 2), np.int64))
    a = rng.integers(0, D - 1, n)
    near = _pairs(a, a + 1)
    far = rng.integers(0, D, (n, 2))
    both = np.concatenate([near, far])
    c = rng.integers(0, D - 1, n // 2)
    two = np.concatenate([_pairs(c, c + 1), rng.integers(0, D, (n - n // 2, 2))])
    g = rng.integers(0, D, n)
    loops = _pairs(g, g)
    pairs = np.concatenate([both, both[:, ::-1], two, two, loops])
    ones = np.ones((len(both), 2), np.int64)
    loop_strands = np.stack([np.ones(n, np.int64), np.where(rng.integers(0, 2, n) == 1, 1, -1)], 1)
    strands = np.concatenate([ones, -ones, np.ones((len(two), 2), np.int64),
                              np.stack([np.ones(len(two), np.int64), -np.ones(len(two), np.int64)], 1), loop_strands])
    return Shape(D, pairs, strands)


def with_isolated(shape, n, seed):
    """the shape with n more nodes that no pair touches, at seeded places among the ids (the order of the others kept)"""
    rng = np.random.default_rng(seed)
    D = shape.D + n
    keep = np.ones(D, bool)
    keep[rng.permutation(D)[:n]] = False
    new_id = np.flatnonzero(keep)
    return Shape(D, new_id[_pairs(shape.pairs)], shape.strands, shape.ordered)


def caterpillar(spine, seed, leg_times=None, island_times=None):
    """a spine of `spine` nodes in shuffled ids, a leg of two nodes on every fourth spine node, and spine / 2 islands of
    two nodes that are their whole component; ids: spine, then legs, then islands, all shuffled among each other.
    leg_times / island_times: times the reads of leg j / island j are given (default 1).
    Returns (Shape, dict of the id arrays: spine, leg_mid, leg_tip, island [n, 2])"""
    rng = np.random.default_rng(seed)
    n_leg, n_isl = (spine + 3) // 4, spine // 2
    D = spine + 2 * n_leg + 2 * n_isl
    ids = rng.permutation(D)
    sp = _chain_order(ids[:spine], rng)
    mid, tip = ids[spine:spine + n_leg], ids[spine + n_leg:spine + 2 * n_leg]
    isl = ids[spine + 2 * n_leg:].reshape(n_isl, 2)
    leg_times = np.ones(n_leg, np.int64) if leg_times is None else np.asarray(leg_times, np.int64)
    island_times = np.ones(n_isl, np.int64) if island_times is None else np.asarray(island_times, np.int64)
    pairs = np.concatenate([_pairs(sp[:-1], sp[1:]),
                            np.repeat(_pairs(sp[::4], mid), leg_times, axis=0),
                            np.repeat(_pairs(mid, tip), leg_times, axis=0),
                            np.repeat(isl, island_times, axis=0)])
    return Shape(D, pairs), {"spine": sp, "leg_mid": mid, "leg_tip": tip, "island": isl}


# ------------------------------------------------------------------ the cases of the tests
WORKING_D = 200_000     # three times the 65 536-thread grid of k_comp_hist: each of its threads meets several nodes
SMALL_D = (1, 2, 255, 256, 257)   # either side of one 256-thread workgroup
STAR_LEAVES = 70_000


def make(name, D):
    """the shape called `name` at D nodes (seeds fixed here: every test of a name and size sees the same graph)"""
    if name in ("star_last", "star_first"):     # 70 000 leaves at the working size, 7 nodes in 20 below it
        leaves = STAR_LEAVES if D > 2 * STAR_LEAVES else max(D - 1, 0) * 7 // 20
        return star(D, D - 1, leaves, 11) if name == "star_last" else star(D, 0, leaves, 12)
    if name == "prefix_only":
        return Shape(D, _pairs([]))
    if name.endswith("+isolated"):      # the routes' variant: a hundredth of the nodes no pair touches
        extra = D // 100
        return with_isolated(make(name[:-len("+isolated")], D - extra), extra, 13)
    seeds = {"shuffled_chain": 1, "ascending_chain": 2, "runs_and_bridges": 3, "triples": 4, "sparse_random": 5,
             "late_bridge": 6, "both_signs": 7}
    return globals()[name](D, seeds[name])


SHAPES = ("shuffled_chain", "ascending_chain", "runs_and_bridges", "star_last", "star_first", "triples",
          "sparse_random", "late_bridge", "both_signs")
EDGE_SHAPES = ("shuffled_chain", "triples", "sparse_random")    # these also run at SMALL_D
ROUTE_SHAPES = ("shuffled_chain", "runs_and_bridges", "triples", "sparse_random")
# every (name, D) of the labellers' main test
CASES = ([(s, WORKING_D) for s in SHAPES] + [(s, d) for s in EDGE_SHAPES for d in SMALL_D] + [("prefix_only", 257)])


# ------------------------------------------------------------------ inputs of the consumers' tests
def low_coverage_case(name):
    """(Shape, m) for remove_low_coverage_components(m): m leaves at least a quarter of the components alive and kills
    at least a quarter.  Node coverage = 1 (the prefix read) + the pair reads on the node."""
    if name == "sparse_random":
        # 1 + degree: m = 2 kills the isolated nodes (e^-1 of the nodes, nearly three quarters of the components),
        # every component with a pair read survives
        return make("sparse_random", WORKING_D), 2
    if name == "sparse_random_m3":
        # m = 3 kills the two-node components as well: about an eighth of the components survive, half the nodes
        return make("sparse_random", WORKING_D), 3
    # three paths in ten have their reads three times: ends 4, middle 7; the others 2 and 3.  (A tenth of the paths
    # cannot leave a quarter of the components alive.)
    rng = np.random.default_rng(21)
    n = WORKING_D // 3
    times = np.where(rng.random(n) < 0.3, 3, 1)
    return triples(WORKING_D, 0, times), 4


CLIP_SPINE, CLIP_MIN_LENGTH = 80_000, 4


def clip_case(filtered):
    """(Shape, parts) of the caterpillar with islands.  filtered: for a filter(3, 1) before the clip — half the legs
    and half the islands have their reads twice: such a leg lives on whole (tip 3, middle 5), the other legs lose
    their tip (2) and keep the middle (3) as a one-node tip; such an island lives on (3, 3) and is its whole
    component, the others die.  The spine nodes have 3 or more throughout."""
    if not filtered:
        return caterpillar(CLIP_SPINE, 31)
    rng = np.random.default_rng(32)
    n_leg, n_isl = (CLIP_SPINE + 3) // 4, CLIP_SPINE // 2
    return caterpillar(CLIP_SPINE, 31, 1 + (rng.random(n_leg) < 0.5), 1 + (rng.random(n_isl) < 0.5))
