#!/usr/bin/env python3
"""The overlap stage's device pass beside the per-pair Python restatement of the reference (tests/test_overlap_cuts.py:
restated_cut), on N pairs of synthetic overlapping contig ends at two sizes.  Both must give the same cuts: the tool asserts it.

    python tools/overlap_bench.py [--pairs 2000] [--sizes 60,600] [--repeat 5] [--device 0]

Per size one JSON line: pairs, minimizers per slice, best-of-`repeat` seconds of Device.overlap_cuts on a resident sketch (upload of
the pair records, the kernels, download of the cut records: what merge_overlapping_pathfile waits for), seconds of the restatement
over the same pairs (once), and the two as pairs per second.  The restatement builds dicts and adjacency sets as the reference does
but no igraph graph, so it is a lower bound of the reference's time, not a measurement of it."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_overlap_cuts as cases  # noqa: E402  (the restatement and the pair generator)
from ntlink_amd import capi  # noqa: E402


def run(dev, n_pairs, size, repeat, seed=5):
    rng = np.random.default_rng(seed)
    c = cases.Cases()
    for _ in range(n_pairs):  # contig ends that share most of their minimizers, a few rearranged blocks
        cases.random_pair(c, rng, size, size, int(size * rng.uniform(0.6, 1.0)), int(rng.integers(0, 4)))
    off, h, q, s, pairs = c.arrays()
    with dev.sketch_from_arrays(off, h, q, s) as sk:
        got = dev.overlap_cuts(sk, pairs)  # (first call: module load)
        best = float("inf")
        for _ in range(repeat):
            dev.sync()
            t0 = time.perf_counter()
            got = dev.overlap_cuts(sk, pairs)
            best = min(best, time.perf_counter() - t0)
    t0 = time.perf_counter()
    want = np.array([cases.restated_cut(c.lists, p) for p in c.pairs], capi.OVERLAP_CUT_DT)
    t_py = time.perf_counter() - t0
    assert (got == want).all(), f"{int((got != want).sum())} of {n_pairs} pairs differ from the restatement"
    return {"pairs": n_pairs, "minimizers_per_slice": size, "device_s_best": round(best, 6), "repeat": repeat, "restated_python_s": round(t_py, 3),
            "device_pairs_per_s": round(n_pairs / best), "python_pairs_per_s": round(n_pairs / t_py), "device": dev.name,
            "cuts_found": int((got["status"] & capi.NTL_OVERLAP_CUT != 0).sum()), "global_path": int((got["status"] & capi.NTL_OVERLAP_GLOBAL != 0).sum())}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--pairs", type=int, default=2000)
    ap.add_argument("--sizes", default="60,600")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    dev = capi.Device(a.device)
    try:
        for size in (int(x) for x in a.sizes.split(",")):
            print(json.dumps(run(dev, a.pairs, size, a.repeat)), flush=True)
    finally:
        dev.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
