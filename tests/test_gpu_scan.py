"""GPU: the one-launch exclusive scans (amg_scan.hip) and what their loaders and emitters do on the way, against numpy,
at sizes 0, 1, the 8 192-element tile boundaries +- 1 and up to 6 M elements, and over enough back-to-back scans to wrap
the 14-bit epoch of the tile status words."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = 8192  # elements per workgroup of the scan (SC_TILE)
SIZES = [0, 1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE + 1, 64 * TILE - 1, 64 * TILE,
         64 * TILE + 1, 65 * TILE + 1, 1_000_003, 6_000_000]


@pytest.fixture(scope="module")
def eng():
    from amira_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def probe(eng, kind, inp, n, out_words, aux_bytes):
    from amira_amd import _ffi
    out = np.zeros(out_words, np.int64)
    aux = np.zeros(max(aux_bytes, 1), np.uint8)
    inp = np.ascontiguousarray(inp)
    _ffi.check(_ffi.lib.amg_scan_probe(eng._h, kind, _ffi.ptr(inp) if inp.size else None, n, _ffi.ptr(out),
                                       _ffi.ptr(aux)))
    return out, aux[:aux_bytes]


def exscan(v):
    return np.concatenate([[0], np.cumsum(v, dtype=np.int64)])


def pair_keys(rng, n):
    lo = rng.integers(0, 1 << 31, n, dtype=np.int64)
    hi = np.where(rng.random(n) < 0.1, lo, rng.integers(0, 1 << 31, n, dtype=np.int64))
    return ((lo.astype(np.uint64) << np.uint64(32)) | (hi + 1).astype(np.uint64)), lo, hi


@pytest.mark.parametrize("n", SIZES)
def test_bytes_set_and_side_clear(eng, n):
    rng = np.random.default_rng(n)
    a = (rng.random(n) < 0.3).astype(np.uint8) * rng.integers(1, 256, n).astype(np.uint8)
    out, aux = probe(eng, 0, a, n, n + 1, n)
    assert np.array_equal(out, exscan(a != 0))
    assert not aux.any()  # the side range is zeroed by the scan's workgroups


@pytest.mark.parametrize("n", SIZES)
def test_pair_width(eng, n):
    keys, lo, hi = pair_keys(np.random.default_rng(n + 1), n)
    out, _ = probe(eng, 1, keys, n, n + 1, 0)
    assert np.array_equal(out, exscan(np.where(lo == hi, 1, 2)))


@pytest.mark.parametrize("n", [0, 1, 127, 128, 129, TILE - 1, TILE + 1, 64 * TILE + 1, 1_875_968])
def test_flag_words(eng, n):
    rng = np.random.default_rng(n + 2)
    flags = (rng.random(32 * n) < 0.2).astype(np.uint8)
    out, aux = probe(eng, 2, flags, n, n + 1, 4 * n)
    words = (flags.reshape(n, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)
    assert np.array_equal(aux.view(np.uint32), words)
    assert np.array_equal(out, exscan(flags.reshape(n, 32).sum(axis=1)))


@pytest.mark.parametrize("n", SIZES)
def test_apply_kill(eng, n):
    rng = np.random.default_rng(n + 3)
    kill = (rng.random(n) < 0.2).astype(np.uint8)
    alive = (rng.random(n) < 0.7).astype(np.uint8)
    out, aux = probe(eng, 3, np.concatenate([kill, alive]), n, n + 1, 2 * n)
    f = (kill != 0) & (alive != 0)
    assert np.array_equal(out, exscan(f))
    assert np.array_equal(aux[:n], f.astype(np.uint8))
    assert np.array_equal(aux[n:], np.where(f, 0, alive).astype(np.uint8))


@pytest.mark.parametrize("n", SIZES)
def test_keep_and_len(eng, n):
    rng = np.random.default_rng(n + 4)
    ln = np.where(rng.random(n) < 0.1, 0, rng.integers(1, 200, n)).astype(np.uint32)
    out, _ = probe(eng, 4, ln, n, 2 * (n + 1), 0)
    assert np.array_equal(out[:n + 1], exscan(ln != 0))
    assert np.array_equal(out[n + 1:], exscan(ln))


@pytest.mark.parametrize("n", [0, 1, 2, TILE - 1, TILE, TILE + 1, 64 * TILE + 1, 1_000_003, 6_000_000])
def test_emit_edges(eng, n):
    """the pair-width scan that writes the directed edges of every class at its prefix (the compaction fused in)"""
    rng = np.random.default_rng(n + 5)
    keys, lo, hi = pair_keys(rng, n)
    first = rng.integers(0, 8, n).astype(np.uint64)
    cnt = rng.integers(1, 1000, n).astype(np.uint32)
    inp = np.concatenate([keys.view(np.uint8), first.view(np.uint8), cnt.view(np.uint8)])
    E = 2 * n
    out, aux = probe(eng, 5, inp, n, 1, 15 * E)
    width = np.where(lo == hi, 1, 2)
    base = exscan(width)
    assert out[0] == base[-1]
    tot = int(base[-1])
    src = aux[:4 * E].view(np.int32)
    tgt = aux[4 * E:8 * E].view(np.int32)
    cov = aux[8 * E:12 * E].view(np.uint32)
    sdir = aux[12 * E:13 * E].view(np.int8)
    tdir = aux[13 * E:14 * E].view(np.int8)
    alv = aux[14 * E:15 * E]
    f = first.astype(np.int64)
    X = np.where(f & 1, lo, hi)
    Y = np.where(f & 1, hi, lo)
    dX = np.where(f & 2, 1, -1)
    dY = np.where(f & 4, 1, -1)
    e = base[:-1]
    w_src = np.empty(tot, np.int64)
    w_tgt = np.empty(tot, np.int64)
    w_sd = np.empty(tot, np.int64)
    w_td = np.empty(tot, np.int64)
    w_cov = np.empty(tot, np.int64)
    w_src[e], w_tgt[e], w_sd[e], w_td[e] = X, Y, dX, dY
    w_cov[e] = np.where(lo == hi, 2 * cnt.astype(np.int64), cnt)
    two = lo != hi
    e2 = e[two] + 1
    w_src[e2], w_tgt[e2], w_sd[e2], w_td[e2], w_cov[e2] = Y[two], X[two], -dY[two], -dX[two], cnt[two]
    assert np.array_equal(src[:tot], w_src) and np.array_equal(tgt[:tot], w_tgt)
    assert np.array_equal(sdir[:tot], w_sd) and np.array_equal(tdir[:tot], w_td)
    assert np.array_equal(cov[:tot], w_cov)
    assert (alv[:tot] == 1).all() and (alv[tot:] == 0xff).all()  # nothing written behind the last edge


def test_epoch_wrap(eng):
    """more back-to-back scans than the 14-bit epoch of the status words counts: every one stays exact"""
    rng = np.random.default_rng(7)
    sizes = [1, TILE + 1, 3 * TILE - 1]
    data = [(rng.random(n) < 0.5).astype(np.uint8) for n in sizes]
    want = [exscan(a) for a in data]
    for j in range((1 << 14) + 40):
        s = j % len(sizes)
        out, _ = probe(eng, 0, data[s], sizes[s], sizes[s] + 1, sizes[s])
        assert np.array_equal(out, want[s]), j
