"""The position carry-over of a re-threaded read as the reference makes it, for pairs of gene lists chosen by the
tests (tests/test_carry_over_cpu.py, tests/test_gpu_carry_over.py against amg_nw_probe):

  carry_over        the pinned oracle's needleman_wunsch, the loop of process_read_correction over the alignment
                    (oracle/amira_oracle/graph.py:752-762) and replace_invalid_gene_positions, on Python ints
  carry_over_fast   the same computed a matrix row at a time on numpy arrays, for volume (held equal to carry_over on
                    thousands of the generated pairs by the CPU test)
  predicted_route   which of its routes the device must take for a pair: the two shortcut rules are the functions of
                    test_nw_shortcut_cpu.py (proved there against the reference's alignment), the limits are those of
                    amg_correct.h restated
  expected_totals   the three totals of the shape fetch that these sizes imply
  the generators    the pair sets of the GPU tests, from fixed seeds

Ops are numbered as the kernels number their pointers: 0 a diagonal column, 1 a gene of x against a gap (LEFT), 2 a
gene of y against a gap (UP); front to back."""
import random

import numpy as np

from test_nw_shortcut_cpu import certificate_positions, shortcut_says_diagonal

NWF_MAX_N, NWF_MAX_M = 128, 64          # amg_correct.h: what k_corr_nw_fast takes
NW_LDS_N, NW_LDS_CELLS = 1024, 16384    # amg_correct.h: what k_corr_nw keeps in LDS
NO_FAST, NO_SHORTCUT, POOLED = 1, 2, 4  # flag bits of amg_nw_probe
R_NONE, R_EQUAL, R_CERT, R_FILL, R_LDS, R_GLOBAL = range(6)


class _Len:
    """stands in for a read's sequence: replace_invalid_gene_positions only takes its len()"""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n


def carry_over(x, y, pos, read_len):
    """(starts, ends, ops) by the oracle's own three functions.  pos: (start, end) per gene of y; read_len None:
    no read lengths were set (the engine then takes 0 for it)"""
    from amira_oracle.graph import GeneMerGraph
    new_pos, ops, cur = [], [], 0
    for a, b in GeneMerGraph.needleman_wunsch(None, list(x), list(y)):
        if a != "*":
            ops.append(1 if b == "*" else 0)
            if b != a:
                new_pos.append((None, None))
            else:
                new_pos.append(tuple(pos[cur]))
                cur += 1
        else:
            ops.append(2)
            cur += 1
    fastq = {0: {"sequence": _Len(0 if read_len is None else int(read_len))}}
    out = GeneMerGraph.replace_invalid_gene_positions(None, new_pos, fastq, 0)
    return [s for s, _ in out], [e for _, e in out], ops


def carry_over_fast(x, y, pos, read_len):
    """carry_over restated: the matrix a row at a time (F[i, j] = max(c_j, F[i, j-1] - 1) is a running maximum of
    c_k + k), pointers with the reference's tie order UP > LEFT > DIAG, the same traceback, loop and repair"""
    n, m = len(x), len(y)
    xa, ya = np.asarray(x, np.int64), np.asarray(y, np.int64)
    cols = np.arange(m, dtype=np.int64)
    prev = -cols                       # F[-1, j] = -j
    ptr = np.empty((n, m), np.uint8)
    for i in range(n):
        diag = np.empty(m, np.int64)   # F[i-1, j-1]
        diag[0] = 0 if i == 0 else -(i - 1)
        diag[1:] = prev[:-1]
        s_d = diag + (ya == xa[i])
        s_l = prev - 1
        c = np.maximum(s_d, s_l)
        row = np.maximum(np.maximum.accumulate(c + cols), -i - 1) - cols   # F[i, -1] = -i enters as k = -1
        s_u = np.empty(m, np.int64)    # F[i, j-1] - 1
        s_u[0] = -i - 1
        s_u[1:] = row[:-1] - 1
        ptr[i] = np.where(s_u >= c, 2, np.where(s_l >= s_d, 1, 0))
        prev = row
    back = []
    i, j = n - 1, m - 1
    P = ptr.tolist()
    while i >= 0 and j >= 0:
        p = P[i][j]
        back.append(p)
        if p == 0:
            i, j = i - 1, j - 1
        elif p == 1:
            i -= 1
        else:
            j -= 1
    back += [1] * (i + 1) + [2] * (j + 1)
    ops = back[::-1]
    starts, ends, xi, yj, cur = [], [], 0, 0, 0
    for p in ops:
        if p == 0:
            if x[xi] == y[yj]:
                starts.append(pos[cur][0])
                ends.append(pos[cur][1])
                cur += 1
            else:
                starts.append(None)
                ends.append(None)
            xi, yj = xi + 1, yj + 1
        elif p == 1:
            starts.append(None)
            ends.append(None)
            xi += 1
        else:
            cur, yj = cur + 1, yj + 1
    rl = 0 if read_len is None else int(read_len)
    valid = [s is not None for s in starts]
    nxt, nxt_of = None, [None] * n     # the next start that was valid before the repair
    for q in range(n - 1, -1, -1):
        nxt_of[q] = nxt
        if valid[q]:
            nxt = starts[q]
    prev_end = 0
    for q in range(n):
        if valid[q]:
            prev_end = ends[q]
        else:
            starts[q] = prev_end
            ends[q] = nxt_of[q] if nxt_of[q] is not None else rl - 1
    return starts, ends, ops


def fast_ok(n, m):
    return 0 < n <= NWF_MAX_N and 0 < m <= NWF_MAX_M


def in_lds(n, m):
    return n <= NW_LDS_N and m <= NW_LDS_N and n * m <= NW_LDS_CELLS


def predicted_route(x, y, flags=0, keep=False):
    n, m = len(x), len(y)
    if keep:
        return R_NONE
    if (flags & NO_FAST) or not fast_ok(n, m):
        return R_LDS if in_lds(n, m) else R_GLOBAL
    if not flags & NO_SHORTCUT:
        if n == m and shortcut_says_diagonal(x, y):     # the kernel's order: the equal-length rule first,
            return R_EQUAL
        if 2 <= n <= m and certificate_positions(x, y) is not None:   # the certificate only for N <= M, N >= 2
            return R_CERT
    return R_FILL


def expected_totals(pairs, routes):
    """(bytes of global scratch, positions, pairs for the general kernel) as k_nw_sizes makes them"""
    big = 0
    for (x, y), r in zip(pairs, routes):
        n, m = len(x), len(y)
        if r != R_NONE and not in_lds(n, m):
            big += ((n * m + n + m + 15) & ~15) + ((3 * (n + 1) * 4 + 15) & ~15)
    return big, sum(len(x) for (x, _), r in zip(pairs, routes) if r != R_NONE), sum(r in (R_LDS, R_GLOBAL) for r in routes)


# ------------------------------------------------------------------ positions and read lengths
_BITS = (12, 20, 31, 32, 33, 41, 44, 62)


def _value(rng):
    return rng.randrange(1 << rng.choice(_BITS))


def positions_for(rng, m):
    """m (start, end) pairs: random, in no order, all 2 m values distinct, below 2^12 up to 2^62"""
    seen = set()
    while len(seen) < 2 * m:
        seen.add(_value(rng))
    v = list(seen)
    rng.shuffle(v)
    return [(v[2 * i], v[2 * i + 1]) for i in range(m)]


def read_len_for(rng):
    return 1 + _value(rng)


# ------------------------------------------------------------------ the generated pair sets
def _fresh(rng):
    return rng.randrange(100000, 200000)   # a gene no generated y holds


def gen_equal(rng):
    """equal length: tandem arrays, a shift by one (of the whole list or of a short stretch, which is what ties with
    the diagonal at two to four mismatches), 0 to 6 substitutions"""
    n = rng.randint(1, 64)
    alpha = rng.choice((1, 2, 4, 1000))
    y = [rng.randrange(alpha) for _ in range(n)]
    if rng.random() < 0.6:
        at, ln = rng.randrange(n), rng.randint(2, 6)
        y[at:at + ln] = [y[at]] * min(ln, n - at)
    x = list(y)
    u = rng.random()
    if u < 0.2:                       # the whole list shifted by one
        x = x[1:] + [rng.randrange(alpha)]
    elif u < 0.75:                    # a stretch of one to four genes
        at, ln = rng.randrange(n), rng.choice((1, 2, 3, 3, 4, 4))
        for i in range(at, min(at + ln, n)):
            x[i] = y[i + 1] if i + 1 < n else rng.randrange(alpha)
    for _ in range(rng.choice((0, 0, 0, 1, 1, 2, 2, 3, 4, 5, 6))):
        x[rng.randrange(n)] = rng.randrange(alpha + 1)
    return x, y


def gen_trimmed(rng):
    """y with an end trimmed and 0 to 5 genes replaced, sometimes by a gene y holds elsewhere; sometimes a gene twice
    in y, sometimes new genes in front of or behind the slice (the matches' offset then leaves [0, M - N])"""
    m = rng.randint(2, 64)
    y = rng.sample(range(1000), m)
    if rng.random() < 0.2:
        y[rng.randrange(m)] = y[rng.randrange(m)]
    a = rng.randint(0, min(4, m - 1))
    b = max(a + 1, m - rng.randint(0, 4))
    x = y[a:b]
    for _ in range(rng.randint(0, 5)):
        x[rng.randrange(len(x))] = rng.choice(y) if rng.random() < 0.2 else _fresh(rng)
    if rng.random() < 0.2:
        extra = [_fresh(rng) for _ in range(rng.randint(1, 3))]
        x = extra + x if rng.random() < 0.5 else x + extra
    return x[:NWF_MAX_N], y


def gen_edit(rng):
    """y with random substitutions, deletions and insertions"""
    m = rng.randint(1, 64)
    alpha = rng.choice((4, 50, 1000))
    y = [rng.randrange(alpha) for _ in range(m)]
    x = []
    rate = rng.choice((0.02, 0.1, 0.3))
    for g in y:
        u = rng.random()
        if u < rate:
            x.append(rng.randrange(alpha))           # substituted
        elif u < 2 * rate:
            pass                                     # deleted
        elif u < 3 * rate:
            x += [g, rng.randrange(alpha)]           # inserted behind
        else:
            x.append(g)
    return (x or [rng.randrange(alpha)])[:NWF_MAX_N], y


def gen_uniform(rng):
    """uniform random lists over a small alphabet: the fill with as many ties as possible"""
    alpha = rng.choice((1, 2, 4, 50))
    return ([rng.randrange(alpha) for _ in range(rng.randint(1, 128))],
            [rng.randrange(alpha) for _ in range(rng.randint(1, 64))])


def gen_tall(rng):
    """alignments beyond 128 columns: y with a few genes left out (a gap in x each) and genes of its own put in until
    x has 120 to 128 genes"""
    alpha = rng.choice((4, 50, 1000))
    y = [rng.randrange(alpha) for _ in range(rng.randint(40, 64))]
    gone = set(rng.sample(range(len(y)), rng.randint(3, 12)))
    x = [g for i, g in enumerate(y) if i not in gone]
    spots = [rng.randint(0, len(x)) for _ in range(rng.randint(1, 3))]   # in one to three places: elsewhere a gene
    for _ in range(rng.randint(120, 128) - len(x)):                      # left out stays a gap
        at = rng.choice(spots)
        x.insert(at, rng.randrange(alpha) if rng.random() < 0.3 else _fresh(rng))
        spots = [q + 1 if q > at else q for q in spots]
    return x, y


def gen_disjoint(rng):
    """x shares no gene with y: every position is repaired"""
    return ([_fresh(rng) for _ in range(rng.randint(1, 128))], rng.sample(range(1000), rng.randint(1, 64)))


def gen_middle(rng):
    """x matches y only in its middle: repairs at both ends, 0 at the head and read length - 1 at the tail"""
    m = rng.randint(3, 64)
    y = rng.sample(range(1000), m)
    a = rng.randrange(m - 1)
    b = rng.randint(a + 1, m)
    head = [_fresh(rng) for _ in range(rng.randint(1, 30))]
    tail = [_fresh(rng) for _ in range(rng.randint(1, 30))]
    return head + y[a:b] + tail, y


SETS = (  # name, generator, pairs, seed
    ("equal", gen_equal, 1600, 101),
    ("trimmed", gen_trimmed, 600, 102),
    ("edit", gen_edit, 400, 103),
    ("uniform", gen_uniform, 500, 104),
    ("tall", gen_tall, 150, 105),
    ("disjoint", gen_disjoint, 60, 106),
    ("middle", gen_middle, 120, 107),
)
NO_READ_LEN = "edit"   # the set that runs without read lengths


class PairSet:
    """pairs with positions and read lengths; the reference's answer is computed on first use and kept"""

    def __init__(self, name, pairs, seed, with_read_len=True):
        rng = random.Random(seed ^ 0x5eed)
        self.name = name
        self.pairs = [(list(x), list(y)) for x, y in pairs]
        self.pos = [positions_for(rng, len(y)) for _, y in self.pairs]
        self.read_len = [read_len_for(rng) for _ in self.pairs] if with_read_len else None
        self._ref = None

    def rl(self, p):
        return None if self.read_len is None else self.read_len[p]

    @property
    def ref(self):
        if self._ref is None:
            self._ref = [carry_over_fast(x, y, self.pos[p], self.rl(p)) for p, (x, y) in enumerate(self.pairs)]
        return self._ref

    def routes(self, flags=0, keep=None):
        return [predicted_route(x, y, flags, bool(keep and keep[p])) for p, (x, y) in enumerate(self.pairs)]


_GENERATED = {}


def generated(name):
    if name not in _GENERATED:
        _, gen, count, seed = next(s for s in SETS if s[0] == name)
        rng = random.Random(seed)
        _GENERATED[name] = PairSet(name, [gen(rng) for _ in range(count)], seed, with_read_len=name != NO_READ_LEN)
    return _GENERATED[name]
