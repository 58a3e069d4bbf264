"""GPU: the scan over the edges' alive bytes whose emitter writes the dense list of live edges itself (EmitLiveKeys,
amg_scan.hip; probe kind 6), against numpy: every live edge's {row, id} at its rank in edge order, the count, and
nothing written from the count on."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = 8192  # elements per workgroup of the scan (SC_TILE)
SIZES = [0, 1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 65 * TILE + 1]
PATTERNS = ["none", "all", "p30", "p03", "first", "last"]


@pytest.fixture(scope="module")
def eng():
    from amira_amd import Engine
    e = Engine(0)
    yield e
    e.close()


def alive_bytes(rng, n, pattern):
    a = np.zeros(n, np.uint8)
    if pattern == "all":
        a[:] = 1
    elif pattern == "p30":
        a = (rng.random(n) < 0.3).astype(np.uint8) * rng.integers(1, 256, n).astype(np.uint8)  # any set byte is alive
    elif pattern == "p03":
        a = (rng.random(n) < 0.003).astype(np.uint8)
    elif pattern == "first" and n:
        a[0] = 1
    elif pattern == "last" and n:
        a[n - 1] = 1
    return a


def adj_row_of(src, sdir):
    """amg_rows.h: row 2n = forward list of node n, row 2n + 1 = its backward list"""
    return (2 * src.astype(np.int64) + np.where(sdir > 0, 0, 1)).astype(np.uint32)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", SIZES)
def test_live_edges(eng, n, pattern):
    from amira_amd import _ffi
    rng = np.random.default_rng(1000 * SIZES.index(n) + PATTERNS.index(pattern))
    src = rng.integers(0, 1 << 30, n).astype(np.int32)
    sdir = np.where(rng.random(n) < 0.5, 1, -1).astype(np.int8)
    alive = alive_bytes(rng, n, pattern)
    inp = np.concatenate([src.view(np.uint8), alive, sdir.view(np.uint8)])
    out = np.zeros(1, np.int64)
    aux = np.zeros(max(8 * n, 1), np.uint8)
    _ffi.check(_ffi.lib.amg_scan_probe(eng._h, 6, _ffi.ptr(inp) if inp.size else None, n, _ffi.ptr(out), _ffi.ptr(aux)))
    live = np.flatnonzero(alive)
    count = live.size
    assert out[0] == count
    keys = aux[:4 * n].view(np.uint32)
    edge_of = aux[4 * n:8 * n].view(np.uint32)
    assert np.array_equal(edge_of[:count], live)
    assert np.array_equal(keys[:count], adj_row_of(src[live], sdir[live]))
    assert (keys[count:].view(np.uint8) == 0xff).all() and (edge_of[count:].view(np.uint8) == 0xff).all()
