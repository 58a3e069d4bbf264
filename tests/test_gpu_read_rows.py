"""GPU: amg_get_read_nodes_rows (k_gather_read_nodes, amg_api.hip) — the node ids of the windows of a few reads laid
end to end — against slices of the whole per-window array (read_node_ids): row counts around the four rows of a
workgroup, row lengths around the 64 lanes of a wave, repeated and descending rows, ranges that start inside a read,
and what the call refuses.  Integer equality throughout."""
import numpy as np
import pytest

import procedures as P

pytestmark = pytest.mark.gpu

WAVE = 64
ROWS_PER_BLOCK = 4
K = 3
N_ROWS = [0, 1, 3, 4, 5, 257]
ROW_LENGTHS = [0, 1, 63, 64, 65, 148]
E_ARG = -2


@pytest.fixture(scope="module")
def built():
    """(engine, node id per window, read offsets): 40 reads of 150 genes at k = 3, 148 windows a read"""
    from amira_amd import Engine, tokenize
    reads, _, _ = P.synth_inputs(5, 40, 150, 60, 0.05)
    vocab, toks, offs, _ = tokenize(reads)
    e = Engine(0)
    e.set_reads(toks, offs, vocab.two_v)
    e.build(K)
    ids = e.read_node_ids()
    assert (np.diff(offs) - (K - 1)).max() == ROW_LENGTHS[-1] and (ids >= 0).sum() == 40 * 148
    yield e, ids, offs
    e.close()


def check(built, first, n_win):
    eng, ids, _ = built
    first, n_win = np.asarray(first, np.int64), np.asarray(n_win, np.int64)
    got, starts = eng.read_node_ids_of(first, n_win)
    want = np.concatenate([ids[f:f + n] for f, n in zip(first, n_win)]) if len(first) else np.zeros(0, np.int32)
    assert starts.tolist() == [0] + np.cumsum(n_win).tolist()
    assert got.dtype == np.int32 and np.array_equal(got, want), (first, n_win)


@pytest.mark.parametrize("length", ROW_LENGTHS)
@pytest.mark.parametrize("n_rows", N_ROWS)
def test_row_counts_by_lengths(built, n_rows, length):
    offs = built[2]
    reads = np.arange(n_rows) * 7 % 40          # (257 rows of 40 reads: every read asked for several times)
    check(built, offs[reads], np.full(n_rows, length))
    assert (n_rows % ROWS_PER_BLOCK != 0) == (n_rows in (1, 3, 5, 257))   # a last workgroup with idle waves


@pytest.mark.parametrize("n_rows", N_ROWS)
def test_mixed_lengths(built, n_rows):
    offs = built[2]
    rng = np.random.default_rng(n_rows)
    reads = rng.integers(0, 40, n_rows)
    n_win = rng.choice(ROW_LENGTHS, n_rows)
    check(built, offs[reads], n_win)
    check(built, offs[reads], np.where(np.arange(n_rows) % 2 == 0, 0, n_win))      # empty rows between full ones
    check(built, offs[reads], np.where(np.arange(n_rows) == n_rows - 1, 65, 0))    # only the last row holds anything


def test_the_same_read_twice_and_descending_reads(built):
    offs = built[2]
    check(built, offs[[3, 3]], [148, 148])
    check(built, offs[[3, 3, 3, 3, 3]], [148, 64, 0, 65, 148])
    down = np.arange(39, -1, -1)
    check(built, offs[down], np.full(40, 148))
    check(built, offs[down[:5]], [1, 63, 64, 65, 148])


def test_ranges_that_start_inside_a_read(built):
    offs = built[2]
    check(built, offs[[0, 1, 2, 39]] + [1, 63, 64, 100], [147, 65, 64, 48])
    check(built, offs[[7, 7, 7]] + [10, 11, 12], [64, 64, 64])              # overlapping ranges of one read
    # up to the very last place of the array, the last k - 1 places of the last read included
    check(built, [int(offs[-1]) - 150, int(offs[-1]) - 1, int(offs[-1])], [150, 1, 0])


def test_all_rows_empty(built):
    offs = built[2]
    for n_rows in (1, 4, 5):
        check(built, offs[np.arange(n_rows)], np.zeros(n_rows, np.int64))


def raw(built, first, starts, n_rows=None):
    from amira_amd import _ffi
    eng = built[0]
    first, starts = np.asarray(first, np.int64), np.asarray(starts, np.int64)
    out = np.full(max(int(starts.max()), 1) + 8, -7, np.int32)
    rc = _ffi.lib.amg_get_read_nodes_rows(eng._h, _ffi.ptr(first), _ffi.ptr(starts),
                                          len(first) if n_rows is None else n_rows, _ffi.ptr(out))
    return rc, out


def test_refusals(built):
    _, ids, offs = built
    T = int(offs[-1])
    assert raw(built, [T - 5], [0, 5])[0] == 0                      # the last five places: fine
    assert raw(built, [T - 5], [0, 6])[0] == E_ARG                  # ends one past n_tokens
    assert raw(built, [0, T - 5, 0], [0, 4, 10, 14])[0] == E_ARG    # the same in a middle row
    assert raw(built, [-1], [0, 5])[0] == E_ARG                     # negative first_token
    assert raw(built, [0, -1], [0, 5, 5])[0] == E_ARG               # ... of an empty row
    assert raw(built, [0, 10], [1, 5, 9])[0] == E_ARG               # out_start[0] != 0
    assert raw(built, [0, 10, 20], [0, 8, 4, 12])[0] == E_ARG       # decreasing starts
    assert raw(built, [0], [0, 5], n_rows=-1)[0] == E_ARG
    rc, out = raw(built, [0, 10], [0, 5, 9])                        # and a good call through the same path
    assert rc == 0 and np.array_equal(out[:9], np.concatenate([ids[0:5], ids[10:14]])) and (out[9:] == -7).all()
