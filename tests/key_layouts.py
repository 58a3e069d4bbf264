"""Read sets that put a build through every key scheme and record layout, for tests/test_key_layouts_cpu.py (what the
sets hold, from the oracle alone) and tests/test_gpu_key_layouts.py (the engine against the oracle on them).

Which slot and which record a build uses follows from k and two_v alone (amg_build_x.hip bx_bits / bx_tuple_fits,
amg_build_fp.hip packed_nodes, amg_dist.h held_node_bytes): layout() restates the rule.  One read set per vocabulary
size, as token arrays for Engine.set_reads (no gene names): a genome of 400 random tokens with the vocabulary's edge
tokens pinned into it, 320 reads that are slices of it on either strand, some shorter than any k, 30 % with one
substituted token.  No token stands next to its own complement (flip - t), so no even k has a palindromic gene-mer;
odd k has none anyway (2 t = flip has no solution, flip is odd).

edge_class_reads is the tiny-vocabulary generator of test_gpu_build.test_edge_classes_of_single_nodes, kept here so
that the 32-byte path takes the same reads."""
import numpy as np

KS = tuple(range(2, 17))
# 16, 3, 15, 2, 14, 4, 13, 5, ...: neighbours differ as much as possible in tuple and record size
K_ORDER = (16, 3, 15, 2, 14, 4, 13, 5, 12, 6, 11, 7, 10, 8, 9)
GENOME, N_READS, PIN_COPIES = 400, 320, 3

# name -> (two_v, tokens pinned into the genome, seed)
VOCABS = {
    "small": (600, (0, 599, 299, 300), 1),
    "edge16": (65536, (0, 65535, 32767, 32768), 1),
    "wide": (65538, (0, 65537, 65536, 32768), 5),
}

_read_sets = {}   # name -> (tokens, offsets, two_v): made once, never changed
_oracle = {}      # (name, k) -> token_oracle.build's dict: made once, never changed
_sweeps = {}      # (name, k, thresholds) -> helpers.live_arrays of the filtered oracle sweep


def _draw(rng, two_v, banned):
    """a token that is none of `banned`"""
    while True:
        t = int(rng.integers(0, two_v))
        if t not in banned:
            return t


def read_set(name):
    """(tokens int32, read offsets int64, two_v) of the vocabulary `name`"""
    if name in _read_sets:
        return _read_sets[name]
    two_v, pinned, seed = VOCABS[name]
    flip = two_v - 1
    rng = np.random.default_rng(seed)
    # every pinned token at PIN_COPIES places, no two of them neighbours
    spots = 20 + 28 * np.arange(len(pinned) * PIN_COPIES) + rng.integers(0, 20, len(pinned) * PIN_COPIES)
    pin_at = {int(s): pinned[i % len(pinned)] for i, s in enumerate(spots)}
    genome = np.empty(GENOME, np.int64)
    for i in range(GENOME):
        if i in pin_at:
            genome[i] = pin_at[i]
            continue
        banned = set()
        if i > 0:
            banned.add(flip - int(genome[i - 1]))
        if i + 1 in pin_at:
            banned.add(flip - pin_at[i + 1])
        genome[i] = _draw(rng, two_v, banned)
    reads = []
    for r in range(N_READS):
        n = int(rng.integers(1, 46)) if r % 9 == 8 else int(rng.integers(20, 46))
        start = int(rng.integers(0, GENOME - n + 1))
        s = genome[start:start + n].copy()
        if rng.random() < 0.3:
            p = int(rng.integers(0, n))
            banned = {int(s[p])}
            if p > 0:
                banned.add(flip - int(s[p - 1]))
            if p + 1 < n:
                banned.add(flip - int(s[p + 1]))
            s[p] = _draw(rng, two_v, banned)
        reads.append(s if rng.random() < 0.5 else flip - s[::-1])
    toks = np.concatenate(reads).astype(np.int32)
    offs = np.zeros(len(reads) + 1, np.int64)
    np.cumsum([len(x) for x in reads], out=offs[1:])
    assert not np.any((toks[:-1] + toks[1:] == flip) & ~np.isin(np.arange(1, len(toks)), offs))
    _read_sets[name] = (toks, offs, two_v)
    return _read_sets[name]


def oracle(name, k):
    """the sequential C build of the read set at k"""
    import token_oracle
    if (name, k) not in _oracle:
        toks, offs, two_v = read_set(name)
        _oracle[(name, k)] = token_oracle.build(toks, offs, k, two_v)
    return _oracle[(name, k)]


def filtered_oracle(name, k, thr):
    """helpers.live_arrays of the C sweep oracle after build(k) and filter(*thr)"""
    import token_oracle
    from helpers import live_arrays
    if (name, k, thr) not in _sweeps:
        toks, offs, two_v = read_set(name)
        s = token_oracle.Sweep(toks, offs, two_v)
        try:
            s.build(k)
            s.filter(*thr)
            _sweeps[(name, k, thr)] = live_arrays(s)
        finally:
            s.close()
    return _sweeps[(name, k, thr)]


def shard_bounds(n_reads, world):
    return [(r * n_reads) // world for r in range(world + 1)]


# ------------------------------------------------------------------ the rule: which layout (k, two_v) selects
def key_bits(k, two_v):
    """bits per token of a packed key: 16 while k tokens of 16 bits fit the 94 key bits, else what the vocabulary needs"""
    need = max(int(two_v) - 1, 1).bit_length()
    return 16 if need <= 16 and 16 * k <= 94 else need


def tuple_fits(k, two_v):
    return k * key_bits(k, two_v) <= 94


def layout(k, two_v, fp_mode, merged):
    """What runs, as a dict:
      exact_keys  what amg_counts reports: a single engine 1 (the tuple is the key), 2 (16-byte slots keyed by its
                  verified 94-bit fingerprint) or 0 (32-byte slots); the shards of a merged build 1 or 0
      slots       "exact, one word" / "exact, two words" / "fp94" / "fp, packed" / "fp, unpacked"
      held        the node record of a merge: "16-bit tokens, full" / "16-bit tokens, padded" / "32-bit tokens"; None
                  in a single-engine build"""
    bits = key_bits(k, two_v)
    if not fp_mode and tuple_fits(k, two_v):
        exact, slots = 1, "exact, one word" if k * bits <= 63 else "exact, two words"
    elif not fp_mode and not merged:
        exact, slots = 2, "fp94"
    else:
        exact, slots = 0, "fp, packed" if two_v <= 65536 and k <= 14 else "fp, unpacked"
    held = None
    if merged:
        held = "32-bit tokens" if two_v > 65536 else "16-bit tokens, " + ("padded" if k % 2 else "full")
    return {"exact_keys": exact, "slots": slots, "held": held}


# ------------------------------------------------------------------ tiny vocabularies
def edge_class_reads(seed, V, n_reads, k):
    """(tokens, offsets) over 2 V tokens: random reads of 1 to 14 genes and, one for every ten of them, a planted
    period-2 read a b a b ... of k + 2 to k + 5 genes with strands of their own, forwards or reverse-complemented:
    self-loops, and edge classes of both signs between one pair of nodes"""
    rng = np.random.default_rng(seed)
    reads = [rng.integers(0, 2 * V, int(rng.integers(1, 15))) for _ in range(n_reads)]
    for _ in range(n_reads // 10):
        a, b = rng.integers(0, 2 * V, 2)
        r = np.where(np.arange(int(rng.integers(k + 2, k + 6))) % 2 == 0, a, b)
        reads.append(r if rng.random() < 0.5 else 2 * V - 1 - r[::-1])
    order = rng.permutation(len(reads))
    reads = [reads[i] for i in order]
    toks = np.concatenate(reads).astype(np.int32)
    offs = np.zeros(len(reads) + 1, np.int64)
    np.cumsum([len(r) for r in reads], out=offs[1:])
    return toks, offs


EDGE_CLASS_CASES = ((1, 3, 700, 5), (2, 2, 300, 5), (3, 12, 2500, 3), (4, 40, 3000, 5), (5, 6, 300, 3))  # seed, V, reads, k
