#!/usr/bin/env python3
"""The gap filler's re-mapping loop, grouped against per gap (not the flagship benchmark).

For G synthetic gaps (two scaffold ends of 300 .. 3000 bases, one read piece across them with 5 % errors, k20 w10), in one process:
  grouped   gapfill.map_gap_sequences: sketch, ONE ntl_map_run_grouped, records to Python objects
  per_gap   what the library offered before: one anchor.get_accepted_anchor_contigs per gap (a sketch upload, an index build, a second
            upload, a map and a download each) from the same sketches' arrays, over the first 2000 gaps, scaled to G
  kernel    group_probe_kernel alone (ntl_prof_get "probe") beside the bytes it moves: 16 B per contig record and per read record in,
            12 B per read record out
Prints one JSON line per G."""
import argparse
import json
import sys
import os
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ntlink_amd import anchor, capi, gapfill  # noqa: E402

ACGT = np.frombuffer(b"ACGT", np.uint8)
K, W = 20, 10


def make_gaps(n, seed=1):
    rng = np.random.default_rng(seed)
    scaffolds, reads = [], []
    for g in range(n):
        src, tgt = ACGT[rng.integers(0, 4, int(rng.integers(300, 3001)))], ACGT[rng.integers(0, 4, int(rng.integers(300, 3001)))]
        piece = np.concatenate([src[-int(rng.integers(250, 900)):], ACGT[rng.integers(0, 4, int(rng.integers(50, 400)))],
                                tgt[:int(rng.integers(250, 900))]])
        hit = rng.random(len(piece)) < 0.05
        piece[hit] = ACGT[rng.integers(0, 4, int(hit.sum()))]
        scaffolds += [(f"s{2 * g}+_source", b"N" * int(rng.integers(0, 500)) + src.tobytes()),
                      (f"s{2 * g + 1}+_target", tgt.tobytes() + b"N" * int(rng.integers(0, 500)))]
        reads.append((f"r{g}__s{2 * g}+__s{2 * g + 1}+", piece.tobytes()))
    return scaffolds, reads


def per_gap_loop(dev, scaffolds, reads, args, n):
    """the per-gap way over the first n gaps; the sketches are made once, as for the grouped pass, and are not timed"""
    with dev.batch([s for _i, s in scaffolds[:2 * n]]) as sb, dev.batch([s for _i, s in reads[:n]]) as rb, \
            dev.sketch(sb, K, W) as ssk, dev.sketch(rb, K, W) as rsk:
        soff, sh, sp, ss = ssk.download()
        roff, rh, rp, rs = rsk.download()
    names = [gapfill.default_name_of(i) for i, _s in scaffolds[:2 * n]]
    lens = {names[i]: gapfill._Length(len(scaffolds[i][1])) for i in range(2 * n)}
    two = 0
    t0 = time.perf_counter()
    for g in range(n):
        mx_info, dup = {}, set()
        for c in (2 * g, 2 * g + 1):
            for j in range(int(soff[c]), int(soff[c + 1])):
                key = str(int(sh[j]))
                if key in mx_info:
                    dup.add(key)
                else:
                    mx_info[key] = anchor.Minimizer(names[c], int(sp[j]), "+" if ss[j] else "-")
        for key in dup:
            del mx_info[key]
        mxs = [(str(int(rh[j])), int(rp[j]), "+" if rs[j] else "-") for j in range(int(roff[g]), int(roff[g + 1])) if str(int(rh[j])) in mx_info]
        accepted, _order = anchor.get_accepted_anchor_contigs(mxs, len(reads[g][1]), lens, mx_info, args, dev=dev)
        two += len(accepted) == 2
    return time.perf_counter() - t0, two


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaps", type=int, nargs="+", default=[2000, 20000])
    ap.add_argument("--per-gap", type=int, default=2000, help="gaps the per-gap loop runs over (scaled to G)")
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    args = argparse.Namespace(k=K, z=1000, x=0.0, sensitive=False)
    dev = capi.Device(0)
    for G in a.gaps:
        scaffolds, reads = make_gaps(G)
        list(gapfill.map_gap_sequences(scaffolds[:200], reads[:100], K, W, args, dev=dev))  # warm-up: code objects, pools
        times = []
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            two = sum(len(g.accepted) == 2 for g in gapfill.map_gap_sequences(scaffolds, reads, K, W, args, dev=dev))
            times.append(time.perf_counter() - t0)
        # the kernel alone: one stream, events round the lookup
        dev.set_pipeline(False)
        dev.prof_enable(True)
        dev.prof_reset()
        with dev.batch([s for _i, s in scaffolds]) as sb, dev.batch([s for _i, s in reads]) as rb, dev.sketch(sb, K, W) as ssk, dev.sketch(rb, K, W) as rsk:
            n_c, n_r = ssk.count, rsk.count
            clen = np.array([len(s) for _i, s in scaffolds], np.uint32); rlen = np.array([len(s) for _i, s in reads], np.uint32)
            for _ in range(a.repeat):
                with dev.map_grouped(ssk, clen, 2 * np.arange(G + 1, dtype=np.uint32), rsk, rlen, np.arange(G + 1, dtype=np.uint32), k=K) as res:
                    res.wait()
                    info = res.grouped_info
        probe_ms, launches = dev.prof_get("probe")
        dev.prof_enable(False)
        dev.set_pipeline(True)
        n_pg = min(a.per_gap, G)
        t_pg, two_pg = per_gap_loop(dev, scaffolds, reads, args, n_pg)
        kernel_ms = probe_ms / max(1, launches)
        moved = 16 * n_c + 16 * n_r + 12 * n_r
        print(json.dumps({"gaps": G, "grouped_s": min(times), "grouped_s_all": times, "per_gap_s_scaled": t_pg * G / n_pg, "per_gap_gaps_run": n_pg,
                          "ratio": t_pg * G / n_pg / min(times), "two_accepted": two, "two_accepted_per_gap": two_pg,
                          "probe_kernel_ms": kernel_ms, "probe_bytes": moved, "probe_GBps": moved / kernel_ms / 1e6,
                          "contig_records": n_c, "read_records": n_r, "grouped_info": info, "device": dev.name}), flush=True)
    dev.close()


if __name__ == "__main__":
    main()
