#!/usr/bin/env python3
"""indexlr's TSV of one resident sketch, two ways, written to a file on tmpfs:

    python tools/sketch_text_bench.py [--read-bases 1000000000] [--contig-bases 100000000] [--repeat 5] [--device 0] [--append FILE]

Two JSON lines, one per input:
  reads    one read batch of the synthetic C3 workload (synth.DeviceWorkload) at its k and w (k32 w250), `--pos --strand --len`
  contigs  a batch of synthetic contigs at k15 w5 in the `H:pos` form of the overlap stage (ntLink:244,249)
and per line the best-of-`repeat` milliseconds after a first round -- the two ways alternate inside every repetition, each timed with
time.perf_counter from a drained device to the closed file -- and the bytes each brings to the host:
  a_host_ms    Sketch.download + formats.write_indexlr          (the path as it stands: records cross PCIe, the host formats)
  b_device_ms  Device.names + Sketch.text + formats.write_blob  (NTL_INDEXLR_DEVICE_TEXT=1: the text crosses PCIe)
  text_kernels_ms  the length pass, the scans and the fill pass alone (ntl_prof_get "sketch_text"), per sketch
The two files must be equal: the tool asserts it."""
import argparse
import filecmp
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ntlink_amd import capi, formats, seqio, synth  # noqa: E402


def measure(dev, label, sk, names, lengths, with_len, with_strand, repeat, tmpdir):
    names = seqio.Names.of(names)
    lengths = np.ascontiguousarray(lengths, np.uint32)
    paths = {nm: os.path.join(tmpdir, f"sketch_text_bench.{os.getpid()}.{nm}.tsv") for nm in ("a_host", "b_device")}
    moved = {}

    def host(path):
        off, h, p, s = sk.download()
        moved["a_host"] = off.nbytes // 2 + len(h) * 16  # 32-bit offsets and 16-byte records cross PCIe
        with open(path, "w") as fh:
            formats.write_indexlr(fh, names, lengths, off, h, p, s, with_len, with_strand)

    def device(path):
        moved["b_device"] = 0
        with open(path, "w") as fh, dev.names(names, lengths) as tab:
            for piece in sk.text(tab, with_len, with_strand):
                moved["b_device"] += len(piece)
                try:
                    formats.write_blob(fh, piece)
                finally:
                    dev.pinned_release(piece)

    ways = {"a_host": host, "b_device": device}
    best = {nm: float("inf") for nm in ways}
    times = {nm: [] for nm in ways}
    try:
        for rep in range(repeat + 1):  # the first round: module load, page-locked buffers, the block cache, the page cache
            for nm, fn in ways.items():
                dev.sync()
                t0 = time.perf_counter()
                fn(paths[nm])
                dt = time.perf_counter() - t0
                if rep:
                    best[nm] = min(best[nm], dt)
                    times[nm].append(round(dt * 1e3, 3))
                elif nm == "b_device":
                    assert filecmp.cmp(paths["a_host"], paths["b_device"], shallow=False), "the device text differs from the host emitter's"
        text_bytes = os.path.getsize(paths["b_device"])
        dev.prof_enable(True)
        dev.prof_reset()
        with dev.names(names, lengths) as tab:
            for piece in sk.text(tab, with_len, with_strand):
                dev.pinned_release(piece)
        dev.sync()
        ms, launches = dev.prof_get("sketch_text")
        dev.prof_enable(False)
    finally:
        for p in paths.values():
            if os.path.exists(p):
                os.remove(p)
    return {"input": label, "sequences": len(names), "minimizers": sk.count, "text_bytes": text_bytes, "repeat": repeat,
            **{nm + "_ms": round(best[nm] * 1e3, 3) for nm in ways}, **{nm + "_all_ms": times[nm] for nm in ways},
            **{nm + "_pcie_bytes": int(moved[nm]) for nm in ways}, "text_kernels_ms": round(ms, 3), "text_calls": launches, "device": dev.name}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--read-bases", type=int, default=1_000_000_000)
    ap.add_argument("--contig-bases", type=int, default=100_000_000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--tmpdir", default="/dev/shm")
    ap.add_argument("--append", default=None, help="append the JSON lines to this file too")
    a = ap.parse_args()
    dev = capi.Device(a.device)
    lines = []
    try:
        wl = synth.DeviceWorkload(dev, "C3", 1.0, read_bases=a.read_bases, batch_bases=3_950_000_000)
        k, w = wl.W["k"], wl.W["w"]
        rl = np.ascontiguousarray(wl.read_lens[0], np.uint32)
        with dev.sketch(wl.read_batches[0], k, w) as sk:
            lines.append({"workload": "C3", "k": k, "w": w, "form": "H:pos:strand with --len",
                          **measure(dev, "reads", sk, [f"read{i}" for i in range(len(rl))], rl, True, True, a.repeat, a.tmpdir)})
        wl.close()
        n_ctg = max(1, a.contig_bases // 100_000)
        cl = np.full(n_ctg, 100_000, np.uint32)
        with dev.synth_genome(7, cl) as cb, dev.sketch(cb, 15, 5) as sk:
            lines.append({"workload": "synthetic contigs", "k": 15, "w": 5, "form": "H:pos",
                          **measure(dev, "contigs", sk, [f"ctg{i}" for i in range(n_ctg)], cl, False, False, a.repeat, a.tmpdir)})
    finally:
        dev.close()
    for line in lines:
        print(json.dumps(line), flush=True)
    if a.append:
        with open(a.append, "a") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
