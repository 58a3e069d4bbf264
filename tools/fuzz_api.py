"""Differential fuzzing of the reference-compatible Python layer (amira_amd.GeneMerGraph & co.
over the HIP engine) against the oracle: the golden-generating procedures (tests/golden/
procedures.py: whole sweep through the class API, planted-allele clustering) on random
parameters, product vs oracle.  Run under PYTHONHASHSEED=0 (clustering of the reference depends
on set order).  usage: PYTHONHASHSEED=0 fuzz_api.py SECONDS [SEED] [--wide-k]
--wide-k (or FUZZ_WIDE_K=1): gene-mer sizes up to 15 for bubble popping and up to 11 for the sweep and clustering, on
reads of at least 2k + 20 genes; one line per procedure and a tally per procedure and k at the end.  Without it the
draws are what they always were (tests/test_gpu_fuzz.py runs a seeded leg of them)."""
import json, os, sys, time, traceback, types
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)
import numpy as np
import procedures as P


def impls():
    import amira_amd
    from amira_amd.graph_utils import choose_kmer_size, get_overall_mean_node_coverages
    prod = types.SimpleNamespace(GeneMerGraph=amira_amd.GeneMerGraph, Gene=amira_amd.Gene, GeneMer=amira_amd.GeneMer,
                                 choose_kmer_size=choose_kmer_size,
                                 get_overall_mean_node_coverages=get_overall_mean_node_coverages)
    import amira_oracle
    from amira_oracle import driver
    orc = types.SimpleNamespace(GeneMerGraph=amira_oracle.GeneMerGraph, Gene=amira_oracle.Gene,
                                GeneMer=amira_oracle.GeneMer, choose_kmer_size=driver.choose_kmer_size,
                                get_overall_mean_node_coverages=driver.get_overall_mean_node_coverages)
    return prod, orc


def draw_wide(rng):
    """(procedure, arguments) with the wide choice of k: bubble popping from {3, 5, 7, 9, 11, 15}, the sweep and
    clustering from {3, 5, 7, 9, 11}, reads of 2k + 20 genes and more"""
    u = rng.random()
    only = os.environ.get("FUZZ_ONLY")
    u = {"bubbles": 0.0, "planted": 0.99}.get(only, u)
    seed = int(rng.integers(1, 1 << 30))
    if u < 0.35:
        k = int(rng.choice([3, 5, 7, 9, 11, 15]))
        return P.p_bubbles_random, (seed, int(rng.integers(80, 220)), int(rng.integers(2 * k + 20, 2 * k + 36)),
                                    int(rng.choice([80, 120, 400])), k, float(rng.choice([0.02, 0.04, 0.06])))
    k = int(rng.choice([3, 5, 7, 9, 11]))
    if u < 0.70:
        return P.p_sweep, (seed, int(rng.integers(100, 400)), int(rng.integers(2 * k + 20, 2 * k + 40)),
                           int(rng.choice([120, 400, 1500])), k, float(rng.choice([0.0, 0.03, 0.07])))
    return P.p_planted, (seed, int(rng.integers(150, 300)), int(rng.integers(2 * k + 20, 2 * k + 40)),
                         int(rng.choice([300, 1000])), k)


def run_wide(budget, seed):
    """the wide mode's loop: a palindromic gene-mer (an even k; none of the k drawn here) that BOTH sides refuse counts
    as refused, anything else that differs as a failure"""
    assert os.environ.get("PYTHONHASHSEED") == "0", "run with PYTHONHASHSEED=0"
    prod, orc = impls()
    rng = np.random.default_rng(seed)
    t_end = time.time() + budget
    tally, n_fail, n_refused = {}, 0, 0
    while time.time() < t_end and n_fail < 3:
        proc, args = draw_wide(rng)
        k = args[4]
        t = time.time()
        got = []
        for impl in (prod, orc):
            try:
                got.append(json.loads(json.dumps(proc(impl, *args))))
            except AssertionError as refusal:
                got.append(("refused", type(refusal).__name__))
            except Exception:  # noqa: BLE001
                traceback.print_exc()
                got.append(("raised", len(got)))
        if got[0] == got[1] and isinstance(got[0], tuple):
            verdict = "refused"
            n_refused += 1
        elif got[0] == got[1]:
            verdict = "equal"
            tally[(proc.__name__, k)] = tally.get((proc.__name__, k), 0) + 1
        else:
            verdict = "MISMATCH"
            n_fail += 1
        print(f"{verdict}: {proc.__name__} {args} {time.time() - t:.1f}s", flush=True)
    for (name, k), n in sorted(tally.items()):
        print(f"fuzz_api wide: {name} k={k}: {n} equal")
    print(f"fuzz_api wide: {sum(tally.values())} procedures equal (product vs oracle), {n_fail} failures, "
          f"{n_refused} refused on both sides (seed {seed})")
    return sum(tally.values()), n_fail


def run(budget, seed, max_cases=None):
    assert os.environ.get("PYTHONHASHSEED") == "0", "run with PYTHONHASHSEED=0"
    prod, orc = impls()
    rng = np.random.default_rng(seed)
    t_end = time.time() + budget
    n_ok = n_fail = 0
    while time.time() < t_end and (max_cases is None or n_ok + n_fail < max_cases):
        k = int(rng.choice([3, 5, 7]))
        u = rng.random()
        only = os.environ.get("FUZZ_ONLY")   # e.g. FUZZ_ONLY=bubbles
        if only == "bubbles":
            u = 0.0
        elif only == "planted":   # read-path clustering (assign_reads_to_genes) on planted multi-copy genes
            u = 0.99
        if u < 0.15:   # bubble popping, device MinHash against the oracle's pure-Python sketch
            k = int(rng.choice([3, 5]))
            args = (int(rng.integers(1, 1 << 30)), int(rng.integers(80, 220)), int(rng.integers(k + 8, 36)),
                    int(rng.choice([40, 120, 400])), k, float(rng.choice([0.02, 0.05, 0.08])))
            proc = P.p_bubbles_random
        elif u < 0.75:
            args = (int(rng.integers(1, 1 << 30)), int(rng.integers(100, 500)), int(rng.integers(k + 6, 45)),
                    int(rng.choice([40, 120, 400, 1500])), k, float(rng.choice([0.0, 0.02, 0.05])))
            proc = P.p_sweep
        else:
            args = (int(rng.integers(1, 1 << 30)), int(rng.integers(150, 400)), int(rng.integers(25, 45)),
                    int(rng.choice([300, 1000])), k)
            proc = P.p_planted
        try:
            a = json.loads(json.dumps(proc(prod, *args)))
            b = json.loads(json.dumps(proc(orc, *args)))
            assert a == b
            n_ok += 1
        except Exception:  # noqa: BLE001
            print("MISMATCH:", proc.__name__, args, flush=True); traceback.print_exc(); n_fail += 1
            if n_fail >= 3:
                break
    print(f"fuzz_api: {n_ok} procedures equal (product vs oracle), {n_fail} failures (seed {seed})")
    return n_ok, n_fail


if __name__ == "__main__":
    wide = "--wide-k" in sys.argv or os.environ.get("FUZZ_WIDE_K", "0") not in ("", "0")
    argv = [a for a in sys.argv[1:] if a != "--wide-k"]
    budget = float(argv[0]) if len(argv) > 0 else 60.0
    seed = int(argv[1]) if len(argv) > 1 else 271828
    sys.exit(1 if (run_wide if wide else run)(budget, seed)[1] else 0)
