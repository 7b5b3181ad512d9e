#!/usr/bin/env python3
"""The gap filler's output stage on a synthetic assembly (the sizes of gapmap_bench.py's mask leg: G + 1 scaffolds of --scaffold-len
bases, G gaps, a read per gap), one JSON line:

  stitch    stitch_kernel alone (ntl_prof_get "stitch", per call) over the whole output, its GB/s counting one read and one write per
            output byte, and in the same process a device-to-device copy of the same number of bytes (hipMemcpy, HIP events): the copy is
            what the kernel is measured against
  stage     gapfill.print_gap_filled_sequences end to end (plan given: segments, stitch, copies into page-locked memory, the file),
            the one-off upload of the assembly's bytes (Device.ascii: the second H2D of the assembly beside Device.batch's), and the
            reference's loop in plain Python -- slicing, translate, concatenation, one write per record -- on the same input; both
            files must be equal

Warm-up run first, then --repeat timed runs of each, alternating; the minimum and every sample are reported."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ntlink_amd import capi, gapfill  # noqa: E402

ACGT = np.frombuffer(b"ACGT", np.uint8)
TABLE = bytes.maketrans(b"ACGTUNMRWSYKVHDBacgtunmrwsykvhdb", b"TGCAANKYWSRMBDHVtgcaankywsrmbdhv")


def make(G, scaffold_len, per_line, seed=1):
    rng = np.random.default_rng(seed)
    blob = ACGT[rng.integers(0, 4, (G + 1) * scaffold_len, dtype=np.uint8)].tobytes()
    seqs = {f"c{i}": blob[i * scaffold_len:(i + 1) * scaffold_len] for i in range(G + 1)}
    reads, pairs, sequences, lines = {}, {}, {}, []
    signs = ["+-"[int(b)] for b in rng.integers(0, 2, G + 1)]
    for name in seqs:
        s = sequences[name] = gapfill.ScaffoldGaps(length=scaffold_len)
        s.five_prime_cut, s.three_prime_cut = int(rng.integers(0, 3000)), scaffold_len - int(rng.integers(0, 3000))
    for g in range(G):
        n = int(rng.integers(1500, 6000))
        reads[f"r{g}"] = ACGT[rng.integers(0, 4, n, dtype=np.uint8)].tobytes()
        a, b = sorted(rng.integers(0, n, 2).tolist())
        p = pairs[(f"c{g}{signs[g]}", f"c{g + 1}{signs[g + 1]}")] = gapfill.PairInfo(100)
        p.chosen_read, p.chosen_reversed = f"r{g}", bool(g & 1)
        p.source_read_cut, p.target_read_cut = (b, a) if g & 1 else (a, b)
    for first in range(0, G + 1, per_line):
        nodes = [f"c{i}{signs[i]}" for i in range(first, min(G + 1, first + per_line))]
        lines.append(f"ntLink_{len(lines)}\t" + " 101N ".join(nodes) + "\n")
    return seqs, reads, pairs, sequences, "".join(lines)


def python_loop(path, out, pairs, sequences, seqs, reads, soft_mask):
    """print_gap_filled_sequences of the reference over bytes, for paths whose gaps are all in `pairs` with both cuts"""
    with open(path) as fin, open(out, "wb") as fout:
        for line in fin:
            ctg_id, nodes = line.strip().split("\t")
            nodes = nodes.split(" ")
            sequence = b""
            for idx, node in enumerate(nodes):
                if node.endswith("N"):
                    p = pairs[(nodes[idx - 1], nodes[idx + 1])]
                    if p.chosen_reversed:
                        piece = reads[p.chosen_read][p.target_read_cut:p.source_read_cut][::-1].translate(TABLE)
                    else:
                        piece = reads[p.chosen_read][p.source_read_cut:p.target_read_cut]
                    sequence += piece.lower() if soft_mask else piece
                else:
                    lo, hi = sequences[node[:-1]].get_cut_coordinates()
                    piece = seqs[node[:-1]][lo:hi]
                    sequence += piece[::-1].translate(TABLE) if node[-1] == "-" else piece
            fout.write(b">" + ctg_id.encode() + b"\n" + sequence + b"\n")


def d2d_copy_ms(nbytes, repeat):
    """hipMemcpy device to device of nbytes between two fresh blocks, timed by HIP events on the null stream -- through the HIP runtime
    the library itself is linked against (already loaded: one runtime per process)"""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")
    vp = C.c_void_p

    def chk(rc):
        if rc != 0:
            raise RuntimeError(f"HIP error {rc}")

    a, b, e0, e1 = vp(), vp(), vp(), vp()
    chk(hip.hipMalloc(C.byref(a), C.c_size_t(nbytes))); chk(hip.hipMalloc(C.byref(b), C.c_size_t(nbytes)))
    chk(hip.hipMemset(a, 65, C.c_size_t(nbytes)))
    chk(hip.hipEventCreate(C.byref(e0))); chk(hip.hipEventCreate(C.byref(e1)))
    out = []
    for i in range(repeat + 1):  # the first is the warm-up
        chk(hip.hipEventRecord(e0, None))
        chk(hip.hipMemcpyAsync(b, a, C.c_size_t(nbytes), 3, None))  # hipMemcpyDeviceToDevice
        chk(hip.hipEventRecord(e1, None))
        chk(hip.hipEventSynchronize(e1))
        ms = C.c_float()
        chk(hip.hipEventElapsedTime(C.byref(ms), e0, e1))
        if i:
            out.append(ms.value)
    for e in (e0, e1):
        hip.hipEventDestroy(e)
    hip.hipFree(a); hip.hipFree(b)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaps", type=int, default=2000)
    ap.add_argument("--scaffold-len", type=int, default=50000)
    ap.add_argument("--per-line", type=int, default=10, help="scaffolds per path line")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--soft-mask", action="store_true")
    a = ap.parse_args()
    seqs, reads, pairs, sequences, path_text = make(a.gaps, a.scaffold_len, a.per_line)
    dev = capi.Device(0)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "b.path")
        with open(path, "w") as fh:
            fh.write(path_text)
        args = argparse.Namespace(o=os.path.join(tmp, "dev.fa"), path=path, min_gap=21, soft_mask=a.soft_mask)
        res_s = gapfill.resident_scaffolds(seqs.items(), dev=dev)
        res_r = gapfill.resident_scaffolds(reads.items(), dev=dev, stitchable=True)
        buf = np.frombuffer(b"".join(seqs.values()), np.uint8)
        off = np.arange(len(seqs) + 1, dtype=np.uint64) * np.uint64(a.scaffold_len)
        t_upload = []
        for _ in range(a.repeat + 1):  # the first is the warm-up (the block cache's first allocation)
            if res_s.ascii is not None:
                res_s.ascii.close()
            dev.sync()
            t0 = time.perf_counter()
            res_s.ascii = dev.ascii(buf, off)
            t_upload.append(time.perf_counter() - t0)
        plan = gapfill.output_plan(path, pairs, sequences, args)
        quiet = open(os.devnull, "w")
        run = lambda: gapfill.print_gap_filled_sequences(pairs, sequences, res_s, res_r, args, dev=dev, plan=plan, stats_file=quiet)
        run()  # warm-up
        python_loop(path, os.path.join(tmp, "py.fa"), pairs, sequences, seqs, reads, a.soft_mask)
        with open(args.o, "rb") as f1, open(os.path.join(tmp, "py.fa"), "rb") as f2:
            assert f1.read() == f2.read(), "the device's file and the Python loop's differ"
        out_bytes = os.path.getsize(args.o)
        t_dev, t_py = [], []
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            run()
            t_dev.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            python_loop(path, os.path.join(tmp, "py.fa"), pairs, sequences, seqs, reads, a.soft_mask)
            t_py.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        gapfill.output_plan(path, pairs, sequences, args)
        t_plan = time.perf_counter() - t0
        dev.prof_enable(True)
        dev.prof_reset()
        for _ in range(a.repeat):
            run()
        dev.sync()
        ms, launches = dev.prof_get("stitch")
        dev.prof_enable(False)
        copy_ms = d2d_copy_ms(out_bytes, a.repeat)
        res_s.close(); res_r.close()
    kernel_ms = ms / max(launches, 1)
    print(json.dumps({"leg": "stitch", "gaps": a.gaps, "scaffold_len": a.scaffold_len, "soft_mask": a.soft_mask, "output_bytes": out_bytes,
                      "segments": sum(len(p) for _i, p in plan.records) + 2 * len(plan.records),
                      "stitch_kernel_ms": kernel_ms, "stitch_launches": launches, "stitch_GBps": 2 * out_bytes / (kernel_ms * 1e-3) / 1e9,
                      "d2d_copy_ms": min(copy_ms), "d2d_copy_ms_all": copy_ms, "d2d_copy_GBps": 2 * out_bytes / (min(copy_ms) * 1e-3) / 1e9,
                      "print_gap_filled_sequences_s": min(t_dev), "print_gap_filled_sequences_s_all": t_dev, "output_plan_s": t_plan,
                      "python_loop_s": min(t_py), "python_loop_s_all": t_py, "python_over_device": min(t_py) / min(t_dev),
                      "ascii_upload_s": min(t_upload[1:]), "ascii_upload_s_all": t_upload, "ascii_upload_bytes": int(len(buf)),
                      "device": dev.name}), flush=True)
    dev.close()


if __name__ == "__main__":
    main()
