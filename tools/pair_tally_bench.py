#!/usr/bin/env python3
"""The pair tally of one mapped read batch, three ways, on the synthetic C3 workload (synth.DeviceWorkload: contigs and reads made on the
device, sketched, indexed and mapped once; the map result stays resident):

    python tools/pair_tally_bench.py [--read-bases 1000000000] [--repeat 5] [--device 0] [--append FILE]

One JSON line: the shape (reads, mappings, pair records), and per way the best-of-`repeat` milliseconds after a first call -- the three
ways alternate inside every repetition -- and the bytes it brings to the host:
  a_text_ends        MapResult.format + Text.download + PairTally.add_batch_ends             (the path as it stands, with text)
  b_text_pairs       the same format and download, the tally from Device.mapres_pairs + PairTally.add_pairs
  c_pairs_only       Device.mapres_pairs + PairTally.add_pairs alone                         (verbose=False paf=False)
  pairs_kernels_ms   the pair kernels alone (ntl_prof_get "pairs": events round the launches and the scan), per call
  host_tally_ms      add_batch_ends / add_pairs alone, per call
The three tallies must be equal: the tool asserts it."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ntlink_amd import capi, pairing, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--read-bases", type=int, default=1_000_000_000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--append", default=None, help="append the JSON line to this file too")
    a = ap.parse_args()
    dev = capi.Device(a.device)
    try:
        wl = synth.DeviceWorkload(dev, "C3", 1.0, read_bases=a.read_bases, batch_bases=3_950_000_000)
        W = wl.W
        k, w, f = W["k"], W["w"], 10
        rb, rl = wl.read_batches[0], np.ascontiguousarray(wl.read_lens[0], np.uint32)
        ctg_names, ctg_len = wl.plan["names"], wl.ctg_len
        read_names = [f"read{i}" for i in range(len(rl))]
        new_tally = lambda: pairing.PairTally(ctg_names, ctg_len, k, f)
        with dev.sketch(wl.contigs, k, w) as csk, dev.index(csk, ctg_len) as ix, dev.sketch(rb, k, w, index=ix, records=False) as rsk, \
                dev.map(ix, rsk, rl, k=k, z=1000) as res, dev.names(read_names, rl) as rn, dev.names(ctg_names, ctg_len) as cn, \
                dev.pair_table(new_tally()) as tab:
            n_maps, n_hits, _n_pafs = res.counts()
            seen = {}

            def text(t, from_pairs):
                with res.format(rn, cn, True, True) as txt:
                    d = txt.download()
                nbytes = len(d["verbose"]) + len(d["paf"]) + d["maps"].nbytes + d["ends"].nbytes
                try:
                    if from_pairs:
                        recs = dev.mapres_pairs(res, tab, rl)
                        nbytes += recs.nbytes
                        t0 = time.perf_counter()
                        t.add_pairs(recs)
                    else:
                        t0 = time.perf_counter()
                        t.add_batch_ends(d["maps"], d["ends"], rl)
                    seen["host_b" if from_pairs else "host_a"] = time.perf_counter() - t0
                finally:
                    dev.pinned_release(d["_pinned"])
                return nbytes

            def bare(t):
                recs = dev.mapres_pairs(res, tab, rl)
                t.add_pairs(recs)
                seen["records"] = len(recs)
                return recs.nbytes

            ways = {"a_text_ends": lambda t: text(t, False), "b_text_pairs": lambda t: text(t, True), "c_pairs_only": bare}
            best, nbytes, exports = {nm: float("inf") for nm in ways}, {}, {}
            host_ms = {"host_a": float("inf"), "host_b": float("inf")}
            for rep in range(a.repeat + 1):  # the first round: module load, page-locked buffers, the block cache
                for nm, fn in ways.items():
                    t = new_tally()
                    dev.sync()
                    t0 = time.perf_counter()
                    nbytes[nm] = fn(t)
                    dt = time.perf_counter() - t0
                    if rep:
                        best[nm] = min(best[nm], dt)
                        for key in host_ms:
                            host_ms[key] = min(host_ms[key], seen.get(key, float("inf")))
                    else:
                        exports[nm] = t.export()
            for nm in ("b_text_pairs", "c_pairs_only"):
                for x, y in zip(exports[nm], exports["a_text_ends"]):
                    assert np.array_equal(x, y), f"the tally of {nm} differs from the host path's"
            dev.prof_enable(True)
            dev.prof_reset()
            for _ in range(a.repeat):
                dev.mapres_pairs(res, tab, rl)
            ms, launches = dev.prof_get("pairs")
            dev.prof_enable(False)
            line = {"workload": "C3", "read_bases": int(rl.sum()), "reads": len(rl), "mappings": n_maps, "hits": n_hits,
                    "pair_records": seen["records"], "pairs": len(exports["a_text_ends"][0]), "repeat": a.repeat,
                    **{nm + "_ms": round(best[nm] * 1e3, 3) for nm in ways}, **{nm + "_bytes": int(nbytes[nm]) for nm in ways},
                    "pairs_kernels_ms": round(ms / max(launches, 1), 3), "host_add_batch_ends_ms": round(host_ms["host_a"] * 1e3, 3),
                    "host_add_pairs_ms": round(host_ms["host_b"] * 1e3, 3), "device": dev.name}
        wl.close()
    finally:
        dev.close()
    print(json.dumps(line), flush=True)
    if a.append:
        with open(a.append, "a") as fh:
            fh.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
