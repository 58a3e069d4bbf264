"""GPU: the scans' lane groups (amg_scan.hip: a lane takes E consecutive elements per row, a tile is T elements, and
both belong to the loader), through amg_scan_probe against numpy.

Every probe kind 0-6 at the sizes where a lane group, a row, a tile or a round of the look-back begins or ends, on
all-zero, all-set and sparse contents (about 1 set in 250: the live-edge regime); the kinds whose values are array
entries also with values that take a tile's sum past 2^32; arrays laid at every offset of a vector (probe kind |
offset << 8), with a head, a body and a tail, and shorter than one vector; the live-edge compaction (kind 6), which
test_gpu_scan.py does not reach; two arrays in one launch whose tile counts differ (kind 7).

Two things the sizes cannot be made to do: the widths of kinds 1 and 5 are 1 or 2 by construction, so no tile of
theirs sums past 2 T (their "large" content is ids at the top of the 31-bit range, every class two edges wide); and the
two loaders of kind 4 read one array with one tile size, so their tile counts are always equal — kind 7 (two arrays of
one length, each at an offset of its own) is where they differ."""

import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# elements per lane (E) and per tile (T = 512 threads x ROWS x E) of the loader behind every probe kind: the table in
# the header comment of amira_amd/csrc/amg_scan.hip (E, ROWS of LoadByteSet, LoadPairWidth<2>, LoadFlagWords,
# LoadApplyKill, LoadNonzero / LoadArrN<u32>, LoadPairWidth<1>, LoadByteSet, LoadArrN<u32>)
E_OF = {0: 16, 1: 2, 2: 2, 3: 8, 4: 4, 5: 1, 6: 16, 7: 4}
T_OF = {0: 16384, 1: 8192, 2: 8192, 3: 8192, 4: 8192, 5: 8192, 6: 16384, 7: 8192}
CONTENTS = ["zero", "set", "sparse"]


def sizes(kind):
    E, T = E_OF[kind], T_OF[kind]
    # 65 T + 1: a look-back of more than one round of 64
    return list(dict.fromkeys([0, 1, E - 1, E, E + 1, 64 * E - 1, 64 * E + 1, T - 1, T, T + 1, 2 * T - 1, 2 * T + 1,
                               64 * T - 1, 64 * T, 64 * T + 1, 65 * T + 1]))


def cases(kind, contents=CONTENTS):
    return [pytest.param(n, c, id=f"{c}-{n}") for c in contents for n in sizes(kind)]


@pytest.fixture(scope="module")
def eng():
    from amira_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def probe(eng, kind, inp, n, out_words, aux_bytes, mis=0, mis_b=0):
    from amira_amd import _ffi
    out = np.zeros(out_words, np.int64)
    aux = np.zeros(max(aux_bytes, 1), np.uint8)
    inp = np.ascontiguousarray(inp)
    _ffi.check(_ffi.lib.amg_scan_probe(eng._h, kind | (mis << 8) | (mis_b << 16), _ffi.ptr(inp) if inp.size else None,
                                       n, _ffi.ptr(out), _ffi.ptr(aux)))
    return out, aux[:aux_bytes]


def exscan(v):
    return np.concatenate([[0], np.cumsum(v, dtype=np.int64)])


def ro(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def flags(content, n, seed):
    """n bytes: none set, all set (any non-zero value), about 1 in 250, or (tenth) 1 in 10"""
    rng = np.random.default_rng(seed)
    if content == "zero":
        return np.zeros(n, np.uint8)
    if content == "set":
        return rng.integers(1, 256, n).astype(np.uint8)
    return ((rng.random(n) < (0.1 if content == "tenth" else 0.004)) * rng.integers(1, 256, n)).astype(np.uint8)


# ---- inputs and what numpy makes of them, once per (content, n); shared by the plain and the misaligned cases

@functools.lru_cache(maxsize=4)
def bytes_case(content, n):
    a = flags(content, n, n)
    return ro(a, exscan(a != 0))


@functools.lru_cache(maxsize=4)
def pair_case(content, n):
    """keys of n edge classes; zero: every class a self-loop of node 0 (width 1), set: every class two wide, sparse: 1
    self-loop in 250, large: two wide with ids at the top of the 31-bit range"""
    rng = np.random.default_rng(n + 1)
    top = (1 << 31) - 2
    if content == "zero":
        lo = np.zeros(n, np.int64)
        hi = lo
    elif content == "large":
        lo = rng.integers(top - 1000, top, n, dtype=np.int64)
        hi = lo + 1
    else:
        lo = rng.integers(0, top, n, dtype=np.int64)
        hi = np.where(rng.random(n) < 0.004, lo, lo + 1) if content == "sparse" else lo + 1
    keys = (lo.astype(np.uint64) << np.uint64(32)) | (hi + 1).astype(np.uint64)
    return ro(keys, lo, hi, exscan(np.where(lo == hi, 1, 2)))


@functools.lru_cache(maxsize=2)
def flagword_case(content, n):
    f = (flags(content, 32 * n, n + 2) != 0).astype(np.uint8)  # (the ranking's flag bytes are 0 or 1)
    rows = f.reshape(n, 32)
    words = np.packbits(rows, axis=1, bitorder="little").view(np.uint32).reshape(n)
    return ro(f, words, exscan(rows.sum(axis=1, dtype=np.int64)))


@functools.lru_cache(maxsize=4)
def kill_case(content, n):
    """marks (none, all, 1 in 250) on nodes that are all alive, or (sparse) seven in ten of them"""
    kill = flags(content, n, n + 3)
    alive = flags("set", n, n + 13)
    if content == "sparse":
        alive = np.where(np.random.default_rng(n + 23).random(n) < 0.7, alive, 0).astype(np.uint8)
    f = (kill != 0) & (alive != 0)
    return ro(np.concatenate([kill, alive]), exscan(f), f.astype(np.uint8), np.where(f, 0, alive).astype(np.uint8))


@functools.lru_cache(maxsize=4)
def len_case(content, n, seed=4):
    rng = np.random.default_rng(n + seed)
    if content == "zero":
        ln = np.zeros(n, np.uint32)
    elif content == "set":
        ln = rng.integers(1, 200, n).astype(np.uint32)
    elif content == "sparse":
        ln = ((rng.random(n) < 0.004) * rng.integers(1, 200, n)).astype(np.uint32)
    else:  # large: the 8 192 of a tile are 2^32 and more, 65 tiles stay below 2^40 (the scans count below 2^48)
        ln = np.where(rng.random(n) < 0.1, 0, rng.integers(1 << 19, 1 << 20, n)).astype(np.uint32)
    return ro(ln, exscan(ln != 0), exscan(ln))


@functools.lru_cache(maxsize=4)
def live_case(content, n):
    rng = np.random.default_rng(n + 6)
    alive = flags(content, n, n + 16)
    src = rng.integers(0, 1 << 30, n).astype(np.int32)
    sdir = np.where(rng.random(n) < 0.5, 1, -1).astype(np.int8)
    inp = np.concatenate([src.view(np.uint8), alive, sdir.view(np.uint8)])
    live = np.flatnonzero(alive).astype(np.uint32)
    rows = (2 * src[live].astype(np.int64) + (sdir[live] <= 0)).astype(np.uint32)  # adj_row_of(src, sdir)
    return ro(inp, live, rows)


# ---- the checks

def check_bytes(eng, n, content, mis=0):
    a, want = bytes_case(content, n)
    out, aux = probe(eng, 0, a, n, n + 1, n, mis)
    assert np.array_equal(out, want)
    assert not aux.any()  # the side range is zeroed by the scan's workgroups


def check_kill(eng, n, content, mis=0):
    inp, want, kill_after, alive_after = kill_case(content, n)
    out, aux = probe(eng, 3, inp, n, n + 1, 2 * n, mis)
    assert np.array_equal(out, want)
    assert np.array_equal(aux[:n], kill_after)
    assert np.array_equal(aux[n:], alive_after)


def check_len(eng, n, content, mis=0):
    ln, keep, off = len_case(content, n)
    out, _ = probe(eng, 4, ln, n, 2 * (n + 1), 0, mis)
    assert np.array_equal(out[:n + 1], keep)
    assert np.array_equal(out[n + 1:], off)


def check_live(eng, n, content, mis=0):
    inp, live, rows = live_case(content, n)
    out, aux = probe(eng, 6, inp, n, 1, 8 * n, mis)
    tot = live.size
    assert out[0] == tot
    keys, edge_of = aux[:4 * n].view(np.uint32), aux[4 * n:].view(np.uint32)
    assert np.array_equal(edge_of[:tot], live)  # the set bytes' indices, ascending
    assert np.array_equal(keys[:tot], rows)
    # nothing written behind the last pair
    assert (keys[tot:] == 0xffffffff).all() and (edge_of[tot:] == 0xffffffff).all()


@pytest.mark.parametrize("n,content", cases(0))
def test_bytes_set(eng, n, content):
    check_bytes(eng, n, content)


@pytest.mark.parametrize("n,content", cases(1, CONTENTS + ["large"]))
def test_pair_width(eng, n, content):
    keys, _, _, want = pair_case(content, n)
    out, _ = probe(eng, 1, keys, n, n + 1, 0)
    assert np.array_equal(out, want)


@pytest.mark.parametrize("n,content", cases(2))
def test_flag_words(eng, n, content):
    f, words, want = flagword_case(content, n)
    out, aux = probe(eng, 2, f, n, n + 1, 4 * n)
    assert np.array_equal(aux.view(np.uint32), words)
    assert np.array_equal(out, want)


@pytest.mark.parametrize("n,content", cases(3))
def test_apply_kill(eng, n, content):
    check_kill(eng, n, content)


@pytest.mark.parametrize("n,content", cases(4, CONTENTS + ["large"]))
def test_keep_and_len(eng, n, content):
    check_len(eng, n, content)


@pytest.mark.parametrize("n,content", cases(5, CONTENTS + ["large"]))
def test_emit_edges(eng, n, content):
    keys, lo, hi, base = pair_case(content, n)
    rng = np.random.default_rng(n + 5)
    first = rng.integers(0, 8, n).astype(np.uint64)
    cnt = rng.integers(1, 1000, n).astype(np.uint32)
    inp = np.concatenate([keys.view(np.uint8), first.view(np.uint8), cnt.view(np.uint8)])
    E = 2 * n
    out, aux = probe(eng, 5, inp, n, 1, 15 * E)
    tot = int(base[-1])
    assert out[0] == tot
    src = aux[:4 * E].view(np.int32)
    tgt = aux[4 * E:8 * E].view(np.int32)
    cov = aux[8 * E:12 * E].view(np.uint32)
    sdir = aux[12 * E:13 * E].view(np.int8)
    tdir = aux[13 * E:14 * E].view(np.int8)
    alv = aux[14 * E:15 * E]
    f = first.astype(np.int64)
    X, Y = np.where(f & 1, lo, hi), np.where(f & 1, hi, lo)
    dX, dY = np.where(f & 2, 1, -1), np.where(f & 4, 1, -1)
    e = base[:-1]
    w = np.empty((5, tot), np.int64)
    w[:, e] = X, Y, dX, dY, np.where(lo == hi, 2 * cnt.astype(np.int64), cnt)
    two = lo != hi
    w[:, e[two] + 1] = Y[two], X[two], -dY[two], -dX[two], cnt[two]
    assert np.array_equal(src[:tot], w[0]) and np.array_equal(tgt[:tot], w[1])
    assert np.array_equal(sdir[:tot], w[2]) and np.array_equal(tdir[:tot], w[3])
    assert np.array_equal(cov[:tot], w[4])
    assert (alv[:tot] == 1).all() and (alv[tot:] == 0xff).all()  # nothing written behind the last edge


@pytest.mark.parametrize("n,content", cases(6))
def test_live_edges(eng, n, content):
    check_live(eng, n, content)


# ---- arrays that begin anywhere: every offset of a vector; a head, a body (whole waves of vector loads) and a tail, and
# arrays shorter than one vector

def mis_sizes(kind):
    E, T = E_OF[kind], T_OF[kind]
    return [1, E - 1, 2 * T + 3 * E + 1, 2 * T + 8 * E]  # (the last: a multiple of 8, kind 3's two arrays sit alike)


def mis_cases(kind):
    return [pytest.param(n, m, id=f"{n}+{m}") for n in mis_sizes(kind) for m in range(1, E_OF[kind])]


@pytest.mark.parametrize("n,mis", mis_cases(0))
def test_bytes_set_misaligned(eng, n, mis):
    check_bytes(eng, n, "sparse", mis)


@pytest.mark.parametrize("n,mis", mis_cases(3))
def test_apply_kill_misaligned(eng, n, mis):
    check_kill(eng, n, "sparse", mis)


@pytest.mark.parametrize("n,mis", mis_cases(4))
def test_keep_and_len_misaligned(eng, n, mis):
    check_len(eng, n, "large", mis)


@pytest.mark.parametrize("n,mis", mis_cases(6))
def test_live_edges_misaligned(eng, n, mis):
    check_live(eng, n, "sparse", mis)


@pytest.mark.parametrize("content", ["set", "tenth"])
def test_live_edges_misaligned_dense(eng, content):
    """rows with a hundred live edges and more (their sources are loaded row by row, not edge by edge), with holes"""
    n = 2 * T_OF[6] + 5
    for mis in (0, 1, 7, 15):
        check_live(eng, n, content, mis)


@pytest.mark.parametrize("n", [T_OF[6] - 1, 65 * T_OF[6] + 1])
def test_live_edges_one_in_ten(eng, n):
    check_live(eng, n, "tenth")


# ---- two arrays in one launch, each on a grid of its own: n + 1 elements and the offset make one tile more in one
# array than in the other (both ways round), or the same number

@pytest.mark.parametrize("n,mis_a,mis_b", [(T_OF[7] - 2, 3, 0), (T_OF[7] - 2, 0, 3), (T_OF[7] - 2, 1, 2),
                                           (2 * T_OF[7] - 3, 2, 3), (2 * T_OF[7] - 3, 3, 1), (1, 3, 2), (0, 1, 3),
                                           (64 * T_OF[7] - 2, 0, 2)])
def test_pair_of_arrays_tile_counts_differ(eng, n, mis_a, mis_b):
    a, _, want_a = len_case("large", n)
    b, _, want_b = len_case("sparse", n, seed=9)
    out, _ = probe(eng, 7, np.concatenate([a, b]), n, 2 * (n + 1), 0, mis_a, mis_b)
    assert np.array_equal(out[:n + 1], want_a)
    assert np.array_equal(out[n + 1:], want_b)
