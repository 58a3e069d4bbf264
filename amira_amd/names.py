"""The 256-bit names of nodes and edges as libamg restates them (amira_amd/csrc/amg_names.h: pickle's bytes for a
tuple of signed 256-bit ints, SHA-256, Python's hash of the result), held against the running interpreter.

The device makes names in bulk (Engine.node_names / edge_names); what it must reproduce is whatever THIS interpreter's
`pickle.dumps(t)` and `hash()` give, because the rest of the object view still uses them.  `names_ok()` checks the
restatement — through the host twin `amg_names_host`, built from the same header as the kernel — against hashlib,
pickle and hash() before the device path is relied on: on an interpreter whose default pickle protocol or integer hash
differ, the host recipe (amira_amd.graph_view.node_hash_of_tokens, Edge.__hash__) stays in charge."""
import hashlib
import pickle
import random

import numpy as np

from . import _ffi
from ._ffi import check, ptr

_OK = None


def names_host(gene_digests, rows, pickle_protocol=None):
    """(uint8 [n, 32], int64 [n]): the names of the rows of tokens `rows` (an int array [n, k]) over the table
    gene_digests (uint8 [V, 32], rank order) by the host twin, and Python's hash() of each.  No device is involved: this
    is what the rule is tested with; the product names on the device or by the interpreter's own pickle."""
    table = np.ascontiguousarray(gene_digests, dtype=np.uint8).reshape(-1, 32)
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    assert rows.ndim == 2
    n, k = rows.shape
    protocol = pickle.DEFAULT_PROTOCOL if pickle_protocol is None else int(pickle_protocol)
    digests, py_hash = np.zeros((n, 32), np.uint8), np.zeros(n, np.int64)
    check(_ffi.lib.amg_names_host(ptr(table) if len(table) else None, len(table), protocol, ptr(rows) if n else None, n,
                                  k, ptr(digests) if n else None, ptr(py_hash) if n else None))
    return digests, py_hash


def names_ok():
    """does the restated recipe give what this interpreter's pickle, hashlib and hash() give?  (a few dozen tuples over
    the boundaries of pickle's integer encodings, once per process, well under a millisecond of hashing)"""
    global _OK
    if _OK is None:
        why = "its pickle.dumps or hash() of a tuple of big ints differ from the restated recipe"
        try:
            _OK = _self_check()
        except Exception as err:  # noqa: BLE001 - an unknown protocol, a missing symbol: the host recipe stays in charge
            _OK, why = False, repr(err)
        if not _OK:
            import sys
            sys.stderr.write("amira_amd: node and edge names are not made on the device with this interpreter "
                             f"({why}); they are hashed one by one on the host, with the same results\n")
    return _OK


def _self_check():
    rng = random.Random(20261021)
    values = [0, 1, 255, 256, 65535, 65536, 2 ** 31 - 1, 2 ** 31, 2 ** 39, 2 ** 63, 2 ** 247, 2 ** 255, 2 ** 256 - 1]
    values += [rng.getrandbits(256) for _ in range(11)]
    values.sort()
    V = len(values)
    table = np.frombuffer(b"".join(v.to_bytes(32, "big") for v in values), np.uint8).reshape(V, 32)
    signed = [-v for v in reversed(values)] + values
    for k in (1, 2, 3, 4, 5, 16):
        rows = [[rng.randrange(2 * V) for _ in range(k)] for _ in range(8)]
        digests, py_hash = names_host(table, np.asarray(rows, np.int32))
        for row, d, h in zip(rows, digests, py_hash.tolist()):
            want = hashlib.sha256(pickle.dumps(tuple(signed[t] for t in row))).digest()
            if d.tobytes() != want or h != hash(int.from_bytes(want, "big")):
                return False
    return True
