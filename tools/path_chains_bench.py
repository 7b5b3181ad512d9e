#!/usr/bin/env python3
"""Device.path_chains on synthetic symmetric chain graphs, beside the host's parsing and the plain restatement:

    python tools/path_chains_bench.py [--vertices 10000 1000000 4000000] [--repeat 5] [--device 0] [--lib FILE] [--no-restated] [--append FILE]

Per size one JSON line.  The input is made as files, as the stage reads them: a best path file of chains of 2 .. 40 contigs with
random signs, and one alternate file that joins the end of every second chain to the head of the next (new edges at end vertices,
all accepted), so that `vertices` oriented contigs stand in the graph.
  host_parse_group_ms  stitch_paths.read_paths + read_alternate_pathfiles on the two files, once
  paths_event_ms       the "paths" event of ntl_path_chains (upload, every launch, the two scans), best of `repeat` after a warm-up call
  wall_to_wait_ms      Device.path_chains from the call to its return (the one wait and the copies of the result), best of `repeat`
  restated_ms          tests/path_cases.restated_chains (dicts and walks, the reference's wording) on the same edge list, once;
                       its chains must equal the device's: the tool asserts it
--lib: another build of the C ABI (the tests' SIMT mock) to try the tool without a GPU; its times mean nothing."""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from ntlink_amd import capi, stitch_paths  # noqa: E402


def write_inputs(tmp, n_contigs, rng):
    "-> (best file, alternate file, chains in the best file)"
    lengths = []
    left = n_contigs
    while left:
        n = min(left, int(rng.integers(2, 41)))
        if left - n == 1:
            n += 1
        lengths.append(n)
        left -= n
    signs = rng.integers(0, 2, n_contigs)
    gaps = rng.integers(1, 2000, n_contigs)
    best, alt = os.path.join(tmp, "best.path"), os.path.join(tmp, "alt.path")
    at, ends = 0, []
    with open(best, "w") as fh:
        for i, n in enumerate(lengths):
            nodes = [f"c{c}{'+-'[signs[c]]}" for c in range(at, at + n)]
            fh.write(f"{i}\t" + " ".join(tok for c, node in enumerate(nodes) for tok in ((node, f"{gaps[at + c]}N") if c + 1 < n else (node,))) + "\n")
            ends.append((nodes[0], nodes[-1]))
            at += n
    with open(alt, "w") as fh:
        for i in range(0, len(ends) - 1, 2):
            fh.write(f"{i}\t{ends[i][1]} {gaps[i]}N {ends[i + 1][0]}\n")
    return best, alt, len(lengths)


def best_of(repeat, fn):
    times = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        times.append(1e3 * (time.perf_counter() - t0))
    return min(times), out


def measure(dev, n_vertices, repeat, restated, seed):
    rng = np.random.default_rng(seed)
    with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(io.StringIO()):
        best_file, alt_file, n_chains = write_inputs(tmp, n_vertices // 2, rng)
        t0 = time.perf_counter()
        names = stitch_paths._Names()
        best = stitch_paths.read_paths(best_file, names)
        s, t, d, n = stitch_paths.read_alternate_pathfiles([best_file, alt_file], best_file, names, best)
        host_ms = 1e3 * (time.perf_counter() - t0)
    edges = np.zeros(len(best[0]) + len(s), capi.PATH_EDGE_DT)
    edges["src"], edges["tgt"], edges["d"] = (np.concatenate([a, b]) for a, b in zip(best, (s, t, d)))
    edges["n"][len(best[0]):], edges["flags"][len(best[0]):] = n, capi.NTL_PATH_EDGE_NEW
    n_vertices = 2 * len(names.names)
    call = lambda: dev.path_chains(n_vertices, edges, None, capi.NTL_PATH_STITCH)
    call()  # the warm-up round: the block cache holds every buffer from here on
    dev.prof_enable(True)
    event = []
    for _ in range(repeat):
        dev.prof_reset()
        call()
        event.append(dev.prof_get("paths")[0])
    dev.prof_enable(False)
    wall_ms, (off, vertex, gap, counts) = best_of(repeat, call)
    line = {"tool": "path_chains_bench", "device": dev.name, "vertices": n_vertices, "edges": len(edges), "new_edges": len(s), "chains_in_best_file": n_chains,
            "chains_out": int(counts["n_chains"]), "chain_vertices_out": int(counts["n_chain_vertices"]), "repeat": repeat,
            "host_parse_group_ms": round(host_ms, 3), "paths_event_ms": round(min(event), 3), "wall_to_wait_ms": round(wall_ms, 3)}
    if restated:
        import path_cases
        t0 = time.perf_counter()
        paths, *_ = path_cases.restated_chains(n_vertices, edges.tolist(), [], capi.NTL_PATH_STITCH)
        line["restated_ms"] = round(1e3 * (time.perf_counter() - t0), 3)
        off = off.tolist()
        assert len(paths) == len(off) - 1 and all(vertex[a:b].tolist() == p[0] and gap[a:b - 1].tolist() == p[1] for a, b, p in zip(off, off[1:], paths)), \
            "the device's chains differ from the restated reference's"
    return line


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--vertices", type=int, nargs="+", default=[10_000, 1_000_000, 4_000_000])
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--lib", default=None, help="another build of the C ABI (the tests' SIMT mock)")
    ap.add_argument("--no-restated", action="store_true", help="skip the plain-Python restatement (minutes at 4 000 000 vertices)")
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--append", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    dev = capi.Device(a.device, lib_path=a.lib) if a.lib else capi.Device(a.device)
    try:
        for n_vertices in a.vertices:
            text = json.dumps(measure(dev, n_vertices, a.repeat, not a.no_restated, a.seed))
            print(text, flush=True)
            if a.append:
                with open(a.append, "a") as fh:
                    fh.write(text + "\n")
    finally:
        dev.close()


if __name__ == "__main__":
    main()
