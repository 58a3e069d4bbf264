"""The recipe of the 256-bit node / edge names with the interpreter's own pickle, hashlib and hash(), and the boundary
vocabulary the names tests share (tests/test_names_cpu.py, tests/test_gpu_names.py).  Nothing of the product is
imported here.

A vocabulary is a table of 32-byte big-endian "digests" in rank order; with V of them a token t in [0, 2V) stands for
+table[t - V] when t >= V and for -table[V - 1 - t] below (amira_amd/tokens.py)."""
import functools
import hashlib
import pickle

import numpy as np

# save_long's boundaries: BININT1 / BININT2 / BININT, and LONG1 lengths around a byte boundary, where a negative value
# loses its trailing ff (only at 2^(8m - 1)) and a positive one gains a 00
MAGNITUDES = sorted([0, 1, 255, 256, 65535, 65536, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1] + [
    v for m in (5, 8, 31, 32) for v in (2 ** (8 * m - 1) - 1, 2 ** (8 * m - 1), 2 ** (8 * m - 1) + 1, 2 ** (8 * m) - 1)])
assert len(MAGNITUDES) == 25 and len(set(MAGNITUDES)) == 25

PROTOCOLS = (4, 5)


def table_bytes(values):
    """uint8 [len(values), 32]: every value big-endian"""
    return np.frombuffer(b"".join(int(v).to_bytes(32, "big") for v in values), np.uint8).reshape(len(values), 32).copy()


def boundary_table():
    return table_bytes(MAGNITUDES)


def signed_value(values, t):
    V = len(values)
    return values[t - V] if t >= V else -values[V - 1 - t]


def name_of(signed_tuple, protocol=pickle.DEFAULT_PROTOCOL):
    return hashlib.sha256(pickle.dumps(tuple(signed_tuple), protocol)).digest()


def message_length(signed_tuple, protocol=pickle.DEFAULT_PROTOCOL):
    return len(pickle.dumps(tuple(signed_tuple), protocol))


def names_of_rows(values, rows, protocol=pickle.DEFAULT_PROTOCOL):
    """(uint8 [n, 32], int64 [n]) of token rows (an int array [n, k]) over the table `values` (Python ints)"""
    rows = np.asarray(rows)
    signed = [-v for v in reversed(values)] + list(values)   # token -> signed value
    digests = [name_of([signed[t] for t in row], protocol) for row in rows.tolist()]
    out = np.frombuffer(b"".join(digests), np.uint8).reshape(len(digests), 32).copy() if digests else np.zeros((0, 32), np.uint8)
    return out, np.asarray([hash(int.from_bytes(d, "big")) for d in digests], np.int64)


def edge_name(src_name, tgt_name, sdir, tdir, protocol=pickle.DEFAULT_PROTOCOL):
    """Edge.__hash__ (construct_edge.py:104-124) from the two node names (ints): the 32 bytes of the smaller"""
    s, t = src_name * sdir, tgt_name * tdir
    return min(name_of((s, t), protocol), name_of((-s, -t), protocol))


def all_pairs(two_v):
    """every ordered pair of tokens: int32 [two_v ** 2, 2]"""
    a = np.arange(two_v, dtype=np.int32)
    return np.stack(np.meshgrid(a, a, indexing="ij"), -1).reshape(-1, 2)


def random_rows(seed, two_v, n, k):
    return np.random.default_rng(seed).integers(0, two_v, size=(n, k), dtype=np.int32)


KS = (1, 2, 3, 4, 5, 16, 17, 64, 256)


@functools.lru_cache(maxsize=None)
def boundary_rows(k):
    """the rows over the boundary vocabulary every test of a k shares: every ordered pair at k = 2 (2 500 rows), 5 000
    random rows otherwise"""
    two_v = 2 * len(MAGNITUDES)
    rows = all_pairs(two_v) if k == 2 else random_rows(100 + k, two_v, 5000, k)
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def boundary_case(k, protocol):
    """(rows, digests, py_hash) of boundary_rows(k) by pickle + hashlib + hash(): made once, never changed"""
    rows = boundary_rows(k)
    digests, py_hash = names_of_rows(MAGNITUDES, rows, protocol)
    digests.setflags(write=False)
    py_hash.setflags(write=False)
    return rows, digests, py_hash
