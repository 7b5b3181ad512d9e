#!/usr/bin/env python3
"""Benchmark of the `ntLink pair` hot path on MI355X (BASELINE.json metric: read Gbases/s mapped, paf=True).

Workload (default C3 = BASELINE.json configs[2], the configuration north_star's target is stated on):
3 Gbp assembly in 5000 contigs + 30x ONT-like 15 kb reads (90 Gbases), k=32 w=250.  Everything is
generated ON THE DEVICE (ntl_synth_*, include/ntlink_amd.h) and is resident in HBM as packed 2-bit
batches before the timed region: the whole 90-Gbases read set as 23 distinct sub-batches (a batch is
bounded by 32-bit base indices), 23 GB of the 288.

  contig stage (once, reported as contig_stage_ms): sketch the contigs, build the index.
  one STEP = one pass of the hot path over the rank's whole read set: for each of its sub-batches
             sketch -> index lookup -> map (accepted contigs + PAF blocks) -> compacted records in HBM.
             The calls only queue device work (include/ntlink_amd.h "Asynchrony"): the window stage of
             sub-batch i+1 runs on its own stream beside the lookup / map kernels of sub-batch i.
  value    = read bases of all ranks x steps / max-over-ranks wall time of the K timed steps.

A plain run sets up, warms up, times the steps and prints the line (--dump-outputs DIR: and writes the outputs of
one more step of the same path).  --full adds the rest: behind the timed region the same context runs a few steps with the second
stream off (per-kernel durations of kernels running alone, what `roofline.kernels_alone` quotes and what the rocprofv3
summaries in profiles/ hold), the clock and power of the GPU during the timed steps, the CPU baseline, the end-to-end
(file to file) leg and the other workloads.

N > 1: one process per GPU (the driver launches `python -m torch.distributed.run ... bench.py --gpus N`;
a bare `python bench.py --gpus N` starts those N ranks itself as a child process).  Reads shard, the contig
index is rebuilt on every GPU, no data-path collective; RCCL carries the barrier and the max.  Default for N > 1:
STRONG scaling, BASELINE.json configs[3] -- the same 90 Gbases split N ways, a rank's share in at least --min-batches (4)
sub-batches; --weak gives every rank a whole read set of its own instead.

Prints ONE JSON line on rank 0.
"""
import argparse
import contextlib
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8 TB/s
N_SIMD = 1024
STAGES = ("sketch_meta", "sketch_mask", "sketch_wave", "sketch_redo", "sketch_emit", "probe", "map", "compact")  # sketch_wave: the window kernel alone, inside sketch_mask


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=14)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--workload", default="C3", help="C3 (default: 3 Gbp + 90 Gbases ONT, k32 w250), C2, C5")
    ap.add_argument("--strong", action="store_true", help="strong scaling: the workload's read set is split over the ranks (configs[3]; the default for --gpus N > 1)")
    ap.add_argument("--weak", action="store_true", help="weak scaling: every rank maps a whole read set of its own (N > 1 only; reported as \"scaling\": \"weak\")")
    ap.add_argument("--emulate-world", type=int, default=0, help="debugging: this ONE rank takes the share (and the sub-batch size) it would have in a world of that size; reported in config")
    ap.add_argument("--min-batches", type=int, default=4, help="strong scaling: a rank's share is cut into at least this many sub-batches (the two-stream pipeline needs a few; "
                    "more and smaller ones cost more than they hide: profiles/r04_strong_share_sweep.txt)")
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the workload (debugging only; reported)")
    ap.add_argument("--batch-bases", type=float, default=3.95e9, help="read bases per device batch")
    ap.add_argument("--full", action="store_true", help="besides the headline: the kernels-alone pass, the clock / power of the GPU during the timed steps, "
                    "the CPU baseline, the end-to-end leg and the other workloads (a plain run sets up, warms up, times the steps and prints the line)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, one more step of the same path whose outputs are written as DIR/<name>.npy "
                    "(float64; a fixed, seeded sample of the reads' mappings, hits and PAF records + every sub-batch's counts; rank 0's share); "
                    "the run fails if its counts are not those the line reports")
    ap.add_argument("--serial-steps", type=int, default=None, help="steps of the kernels-alone pass behind the timed region (0 = none; default 2 with --full, else 0)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--no-e2e", action="store_true", help="--full without the end-to-end leg")
    ap.add_argument("--no-others", action="store_true", help="--full without the other single-GPU configs (other_workloads)")
    ap.add_argument("--e2e-bases", type=float, default=32e9, help="read bases of the end-to-end (file to file) leg")
    ap.add_argument("--lib", default=None, help="C-ABI library to load (tests point this at the SIMT-mock build)")
    ap.add_argument("--spawn-check", action="store_true", help="ranks only report the world size (CPU test of the launcher)")
    args = ap.parse_args(argv)
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.serial_steps is None:
        args.serial_steps = 2 if args.full else 0
    return args


def spawn_ranks(args):
    """`python bench.py --gpus N` without a launcher: start the N ranks as a CHILD process (never exec: this
    process has not touched the GPU, and must not replace itself either way), relay rank 0's JSON line."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    line = None
    for ln in p.stdout.splitlines():
        if ln.startswith("{") and ('"metric"' in ln or '"spawn_check"' in ln):
            line = ln
    if line:
        print(line, flush=True)
    return p.returncode if p.returncode else (0 if line else 1)


class stdout_to_stderr:
    """file descriptor 1 -> 2 for a block (native code and child threads included)"""

    def __enter__(self):
        sys.stdout.flush()
        self.saved = os.dup(1)
        os.dup2(2, 1)

    def __exit__(self, *exc):
        sys.stdout.flush()
        os.dup2(self.saved, 1)
        os.close(self.saved)
        return False


def kernel_signature():
    """Identifies the kernel sources a PMC pass was taken on (profiles/traffic.json is stale after an edit of the code; comments
    and white space do not count)."""
    import re
    h = hashlib.sha1()
    d = os.path.join(ROOT, "ntlink_amd", "csrc")
    for f in ("sketch_kernels.h", "sketch2_kernels.h", "dev_common.h", "dev_intrin.h", "map_kernels.h", "index_common.h"):
        p = os.path.join(d, f)
        if os.path.exists(p):
            text = open(p, "r", errors="replace").read()
            text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)   # block comments
            text = re.sub(r"(?m)(^|[^:\"'])//[^\n]*", r"\1", text)  # line comments (not `://` inside a string)
            h.update(" ".join(text.split()).encode())
    return h.hexdigest()[:12]


class DeviceStatePoller:
    """Shader clock, socket power and junction temperature of this rank's GPU, sampled from the amdgpu hwmon files while the timed
    steps run (a thread that reads three small sysfs files every 100 ms; nothing here can fail the bench: no hwmon, no field).
    Why: the C3 step is instruction-bound and follows the shader clock, and the boxes differ in the clock they sustain under it --
    on some the socket sits at a power limit through the steps (profiles/r07x_clocks_power_during_bench.txt: 2.13 GHz at 1.2 kW against
    2.37 GHz in the lighter phases) -- so the line says which clock its number was measured at."""

    def __init__(self, local_rank=0, period=0.1):
        import glob
        self.period, self.samples, self.thread, self.stop = period, [], None, False
        dirs = []
        for h in sorted(glob.glob("/sys/class/drm/card*/device/hwmon/hwmon*")):
            try:
                if open(os.path.join(h, "freq1_label")).read().strip() == "sclk":
                    dirs.append(h)
            except OSError:
                pass
        # which of the node's cards is this process's GPU: the one at the PCI address the runtime reports; failing that, the card that
        # draws the most power while the steps run (summary)
        self.dirs, self.dir, self.which = dirs, None, None
        try:
            import torch
            pr = torch.cuda.get_device_properties(torch.cuda.current_device())
            addr = f"{getattr(pr, 'pci_domain_id', 0):04x}:{pr.pci_bus_id:02x}:{getattr(pr, 'pci_device_id', 0):02x}."
            for h in dirs:
                if os.path.basename(os.path.realpath(os.path.join(h, "..", ".."))).startswith(addr):
                    self.dir, self.which = h, "the card at this device's PCI address " + addr + "0"
        except Exception:
            pass

    def _read(self, name, scale, d=None):
        try:
            return int(open(os.path.join(d or self.dir, name)).read()) * scale
        except (OSError, ValueError, TypeError):
            return None

    def sample(self):
        out = []
        for d in ([self.dir] if self.dir else self.dirs):
            out.append((self._read("freq1_input", 1e-6, d), self._read("power1_input", 1e-6, d) or self._read("power1_average", 1e-6, d),
                        self._read("temp2_input", 1e-3, d)))
        return out

    def _run(self):
        while not self.stop:
            self.samples.append(self.sample())
            time.sleep(self.period)

    def __enter__(self):
        if self.dir or self.dirs:
            import threading
            self.idle = self.sample()
            self.thread = threading.Thread(target=self._run, daemon=True)
            self.thread.start()
        return self

    def __exit__(self, *exc):
        self.stop = True
        if self.thread:
            self.thread.join(timeout=1.0)
        return False

    def summary(self):
        if not self.samples or not self.samples[0]:
            return None
        import statistics
        cards = [self.dir] if self.dir else self.dirs
        j, which = 0, self.which
        if not self.dir:  # the busiest card
            power = [statistics.median([x[i][1] or 0.0 for x in self.samples]) for i in range(len(cards))]
            j = max(range(len(cards)), key=lambda i: power[i])
            which = f"the card that drew the most power of the node's {len(cards)} (no PCI address from the runtime)"

        def col(i):
            v = [x[j][i] for x in self.samples if x[j][i] is not None]
            return {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)} if v else None
        return {"what": "this rank's GPU while the timed steps ran (amdgpu hwmon, one sample per 100 ms): the step is instruction-bound and follows "
                        "the shader clock; where the socket power sits at a limit through the steps the clock is that limit's",
                "samples": len(self.samples), "sclk_mhz": col(0), "socket_power_w": col(1), "junction_c": col(2),
                "before_the_steps": {"sclk_mhz": self.idle[j][0], "socket_power_w": self.idle[j][1], "junction_c": self.idle[j][2]},
                "power_cap_w": self._read("power1_cap", 1e-6, cards[j]), "source": cards[j], "picked": which}


class Comm:
    """barrier / max / sum / gather over the ranks (RCCL on GPUs, gloo under the SIMT mock); a single process needs none"""

    def __init__(self, use_cuda, local_rank):
        self.dist, self.use_cuda, self.local_rank = None, use_cuda, local_rank
        if "RANK" not in os.environ:
            return
        import torch
        import torch.distributed as dist
        sys.stdout.flush()
        saved = os.dup(1)
        os.dup2(2, 1)  # RCCL prints a version banner on stdout: keep stdout for the one JSON line
        try:
            if use_cuda:
                dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
                warm = torch.zeros(1, device="cuda")
                dist.all_reduce(warm)
                torch.cuda.synchronize()
            else:
                dist.init_process_group("gloo")
        finally:
            sys.stdout.flush()
            os.dup2(saved, 1)
            os.close(saved)
        self.dist = dist

    def barrier(self, devs):
        if self.dist is not None:
            if self.use_cuda:
                self.dist.barrier(device_ids=[self.local_rank])
            else:
                self.dist.barrier()
        if self.use_cuda:
            import torch
            torch.cuda.synchronize()
        for d in devs:
            d.sync()

    def _t(self, v):
        import torch
        return torch.tensor([float(v)], dtype=torch.float64, device="cuda" if self.use_cuda else "cpu")

    def max(self, v):
        if self.dist is None:
            return float(v)
        t = self._t(v)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return float(t.item())

    def sum(self, v):
        if self.dist is None:
            return float(v)
        t = self._t(v)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM)
        return float(t.item())

    def gather(self, v):
        if self.dist is None:
            return [float(v)]
        import torch
        t = self._t(v)
        out = [torch.zeros_like(t) for _ in range(self.dist.get_world_size())]
        self.dist.all_gather(out, t)
        return [float(x.item()) for x in out]

    def gather_obj(self, obj):
        if self.dist is None:
            return [obj]
        out = [None] * self.dist.get_world_size()
        self.dist.all_gather_object(out, obj)
        return out

    def close(self):
        if self.dist is not None:
            self.dist.destroy_process_group()


def run_workload(dev, comm, name, args, steps, warmup, rank, world, serial_steps, dump=False):
    """Generates workload `name` on the device, runs the contig stage once, `warmup` + `steps` timed pipelined steps and
    `serial_steps` steps with the second stream off; dump: the outputs of one more step of the same path in R["outputs"] (OutputSampler).
    Returns the measurements; the workload stays open in R["wl"]."""
    import numpy as np
    from ntlink_amd import synth
    W = synth.workload(name, args.scale)
    k, w = W["k"], W["w"]
    total_read_bases = W["read_bases"]
    share_of = args.emulate_world if (args.emulate_world > 1 and world == 1) else world
    my_bases = total_read_bases // share_of if args.strong else total_read_bases
    batch_bases = int(args.batch_bases)
    if args.strong and share_of > 1:  # a rank's share of configs[3] is 3 sub-batches of the N = 1 size: too few for window(i+1) beside emit(i)
        batch_bases = max(1, min(batch_bases, -(-my_bases // max(1, args.min_batches))))
    t0 = time.perf_counter()
    wl = synth.DeviceWorkload(dev, name, args.scale, read_bases=my_bases, batch_bases=batch_bases,
                              read_seed=(2 + rank) if not args.strong else (2, rank))
    dev.sync()
    gen_s = time.perf_counter() - t0
    params = dict(k=k, z=1000, x=0.0, sensitive=W["sensitive"], repeat_filter=False)
    stats = dict(read_mx=0, index_hits=0, counts=[0, 0, 0])

    # ---- contig stage: once (a 30x read set amortises it; timed on its own)
    dev.prof_enable(True)
    dev.prof_reset()
    dev.sync()
    t0 = time.perf_counter()
    csk = dev.sketch(wl.contigs, k, w)
    ix = dev.index(csk, wl.ctg_len)
    index_size = len(ix)
    dev.sync()
    contig_stage_ms = (time.perf_counter() - t0) * 1e3
    contig_prof = {nm: dev.prof_get(nm) for nm in ("sketch_meta", "sketch_mask", "sketch_redo", "sketch_emit", "index")}
    contig_mx = csk.count

    # NTL_BENCH_STREAMS > 1 (experiments only): that many worker threads, each with its own context, take the sub-batches in turn
    n_streams = max(1, int(os.environ.get("NTL_BENCH_STREAMS", "1")))
    devs = [dev] + [dev.clone() for _ in range(n_streams - 1)]
    for d in devs[1:]:
        d.prof_enable(True)

    def run_batches(d, items, collect, acc, sink=None):
        held = []

        def take(n_keep):  # counts are asked for two sub-batches late: the device never waits for the host's question
            while len(held) > n_keep:
                j, rsk, res = held.pop(0)
                if collect:
                    acc["read_mx"] += rsk.count
                    acc["strips"] = acc.get("strips", 0) + rsk.strips
                    acc["index_hits"] += res.n_index_hits
                    acc["counts"] = [a + b for a, b in zip(acc["counts"], res.counts())]
                if not (sink and sink(j, rsk, res)):  # a sink that returns True keeps the result open (and closes it itself)
                    res.close()
                rsk.close()

        trace = os.environ.get("NTL_BENCH_TRACE")
        for j, (rb, rl) in items:
            t_a = time.perf_counter()
            # as pipeline.run_pair makes it: looked up in the index while emitted (no separate probe pass), and for this map only (no records)
            rsk = d.sketch(rb, k, w, index=ix, records=os.environ.get("NTL_BENCH_RECORDS", "0") == "1")
            t_b = time.perf_counter()
            res = d.map(ix, rsk, rl, **params)  # queued behind it; nothing waits
            if trace:
                print(f"bench trace: sketch call {1e3 * (t_b - t_a):.3f} ms, map call {1e3 * (time.perf_counter() - t_b):.3f} ms", file=sys.stderr)
            if collect or sink:
                held.append((j, rsk, res))
                take(2)
            else:
                res.close()
                rsk.close()
        take(0)

    def step(collect=False, sink=None):
        """sink(sub-batch, sketch, result): every sub-batch's result, taken two sub-batches late as collect takes its counts; a sink must
        not download there (ntl_mapres_download drains the main stream, which would serialise the sub-batches)"""
        if collect:
            stats.update(read_mx=0, index_hits=0, counts=[0, 0, 0], strips=0)
        items = list(enumerate(zip(wl.read_batches, wl.read_lens)))
        if n_streams == 1:
            run_batches(dev, items, collect, stats, sink)
            return
        import threading
        accs = [dict(read_mx=0, index_hits=0, counts=[0, 0, 0]) for _ in devs]
        ths = [threading.Thread(target=run_batches, args=(d, items[i::n_streams], collect, accs[i], sink)) for i, d in enumerate(devs)]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        if collect:
            for a in accs:
                stats["read_mx"] += a["read_mx"]; stats["index_hits"] += a["index_hits"]
                stats["counts"] = [x + y for x, y in zip(stats["counts"], a["counts"])]

    for i in range(warmup):
        step(collect=(i == 0))
    if warmup == 0:
        stats["read_mx"] = None
    for d in devs:
        d.prof_reset()
    comm.barrier(devs)
    poller = DeviceStatePoller(int(os.environ.get("LOCAL_RANK", "0"))) if args.full else None
    with poller or contextlib.nullcontext():
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        comm.barrier(devs)  # ntl_ctx_sync: also where a failure of queued work nobody looked at is raised
        elapsed = time.perf_counter() - t0
    device_state = poller.summary() if poller else None
    prof = {nm: tuple(sum(x) for x in zip(*[d.prof_get(nm) for d in devs])) for nm in STAGES}
    if stats["read_mx"] is None:
        step(collect=True)
        comm.barrier(devs)
    # ---- what the timed steps computed: one more step of the same path after the clock stops -- the same calls queued in the same
    # order, the window stage of sub-batch i + 1 on its own stream beside the lookup / map of sub-batch i.  Inside the step the sink only
    # asks for counts, two sub-batches late as the collect step does (each waits on its own result's event, not on the stream), and
    # keeps the results of up to DUMP_BATCHES sub-batches spread over the step open; they are downloaded and sampled when the step is
    # over (a download waits for everything queued on the stream).  Its counts must be those of the collect step: a step that does
    # not compute the same thing every time fails the run instead of dumping one of its answers.
    outputs = None
    if dump:
        sampler = OutputSampler([len(rl) for rl in wl.read_lens])
        step(sink=sampler.add)
        dev.sync()  # rank 0 only: no collective here
        if comm.use_cuda:
            import torch
            free, total = torch.cuda.mem_get_info()
            print(f"bench: --dump-outputs holds the results of {len(sampler.open)} of {len(wl.read_lens)} sub-batches; device memory in use "
                  f"{(total - free) / 1e9:.1f} GB of {total / 1e9:.1f}", file=sys.stderr)
        sampler.finish()
        outputs = sampler.arrays()
        c = outputs["counts"].sum(axis=0)
        seen = [int(x) for x in c[1:]]
        want = [stats["read_mx"], stats["index_hits"], *stats["counts"]]
        if seen != want:
            raise RuntimeError(f"--dump-outputs: the step's read minimizers, index hits, mappings, hits and PAF records {seen} differ from "
                               f"those of the collect step {want}: the path does not compute the same thing from step to step")
    # ---- kernels alone: the same steps with the window stage back on the one stream
    serial = None
    pipelined = dev.pipelined
    if serial_steps > 0:
        for d in devs:
            if d.pipelined:
                d.set_pipeline(False)
        step()  # untimed: the one-stream order asks the block cache for its arrays in another sequence than the pipelined steps did
        comm.barrier(devs)
        for d in devs:
            d.prof_reset()
        t0 = time.perf_counter()
        for _ in range(serial_steps):
            step()
        comm.barrier(devs)
        s_elapsed = time.perf_counter() - t0
        serial = {"steps": serial_steps, "ms_per_step": s_elapsed / serial_steps * 1e3,
                  "prof": {nm: tuple(sum(x) for x in zip(*[d.prof_get(nm) for d in devs])) for nm in STAGES}}
        if pipelined:
            for d in devs:
                d.set_pipeline(True)
    for d in devs:
        d.prof_enable(False)
    for d in devs[1:]:
        d.close()
    per_rank_ms = [x / steps * 1e3 for x in comm.gather(elapsed)]
    ranks_seen = int(round(comm.sum(1)))
    ranks = comm.gather_obj({"rank": rank, "local_rank": int(os.environ.get("LOCAL_RANK", "0")), "device": dev.name,
                             "backend": ("rccl" if comm.use_cuda else "gloo") if comm.dist is not None else None})
    per_rank_bases = comm.gather(wl.read_bases)
    elapsed_max = comm.max(elapsed)
    total_bases = comm.sum(wl.read_bases)
    return dict(name=name, W=W, wl=wl, ix=ix, csk=csk, params=params, stats=stats, gen_s=gen_s, contig_stage_ms=contig_stage_ms,
                contig_prof=contig_prof, contig_mx=contig_mx, index_size=index_size, elapsed=elapsed_max, total_bases=total_bases,
                prof=prof, serial=serial, pipelined=pipelined, per_rank_ms=per_rank_ms, per_rank_bases=per_rank_bases, steps=steps,
                n_streams=n_streams, ranks_seen=ranks_seen, ranks=ranks, batch_bases=batch_bases, device_state=device_state,
                outputs=outputs)


DUMP_SEED = 20240607          # which reads --dump-outputs samples: fixed, so that two builds are compared on the same reads
DUMP_BATCHES = 8              # sub-batches whose results are held to the end of the dump step (C3: 65 GB of device memory in use with 8 held)
DUMP_READS = 8192             # reads sampled from those sub-batches (C3: about 8 k mappings and 130 k hits)
DUMP_MAX_BYTES = 64 << 20


class OutputSampler:
    """The outputs of one step for --dump-outputs.  add(j, sketch, result) is the step's sink: it takes sub-batch j's counts and keeps
    the result open if j is one of the DUMP_BATCHES sub-batches spread evenly over the step (the first and the last among them);
    finish() downloads those after the step, one at a time, and samples each as it arrives (take).  arrays() -> {name: float64 array}:
      counts  per sub-batch: reads, read minimizers, index hits, mappings, hits, PAF records (the whole step, exact);
      maps    read, contig, hits of the mappings of DUMP_READS reads drawn with DUMP_SEED from the held sub-batches' reads (read = its
              index in the step, sub-batches in order), in the order the device hands them out;
      hits    read, contig, contig position, read position, contig strand, read strand of those mappings' hits, mapping by mapping
              (maps[].hit_off / n_hits into the sub-batch's hit array);
      pafs    read, contig, q_start, q_end, t_start, t_end, hits, strand of their PAF records.
    Every field is a u32 or smaller: float64 holds it exactly.  At most DUMP_MAX_BYTES in all (hits cut at the end beyond that)."""

    def __init__(self, reads_per_batch):
        import numpy as np
        n = np.asarray(reads_per_batch, np.int64)
        self.n, self.base = n, np.concatenate(([0], np.cumsum(n)[:-1]))
        self.held = sorted(set(np.linspace(0, len(n) - 1, min(len(n), DUMP_BATCHES)).round().astype(int).tolist()))
        pool = np.concatenate([np.arange(self.base[j], self.base[j] + n[j]) for j in self.held])
        self.pick = np.sort(np.random.default_rng(DUMP_SEED).choice(pool, size=min(len(pool), DUMP_READS), replace=False))
        self.counts = [None] * len(n)
        self.parts = {}
        self.open = {}

    def add(self, j, rsk, res):
        self.count(j, rsk.count, res.n_index_hits, res.counts())
        if j in self.held:
            self.open[j] = res
            return True
        return False

    def count(self, j, n_mx, n_ix, counts):
        self.counts[j] = [int(self.n[j]), n_mx, n_ix, *counts]

    def finish(self):
        for j in sorted(self.open):
            res = self.open.pop(j)
            try:
                self.take(j, res.download())
            finally:
                res.close()

    def take(self, j, r):
        import numpy as np
        m, h, p = r["maps"], r["hits"], r["pafs"]
        n, base = int(self.n[j]), int(self.base[j])
        mine = self.pick[(self.pick >= base) & (self.pick < base + n)] - base
        sm = m[np.isin(m["read"], mine)]
        sp = p[np.isin(p["read"], mine)]
        nh = sm["n_hits"].astype(np.int64)
        first = np.repeat(sm["hit_off"].astype(np.int64) - np.concatenate(([0], np.cumsum(nh)[:-1])), nh)
        sh = h[first + np.arange(int(nh.sum()), dtype=np.int64)]
        self.parts[j] = (np.stack([sm["read"] + float(base), sm["ctg"], sm["n_hits"]], axis=1),
                         np.stack([np.repeat(sm["read"] + float(base), nh), np.repeat(sm["ctg"], nh), sh["ctg_pos"], sh["read_pos"],
                                   sh["ctg_strand"], sh["read_strand"]], axis=1),
                         np.stack([sp["read"] + float(base), sp["ctg"], sp["q_start"], sp["q_end"], sp["t_start"], sp["t_end"], sp["n_hits"],
                                   sp["strand"]], axis=1))

    def arrays(self):
        import numpy as np
        if any(x is None for x in self.counts) or sorted(self.parts) != self.held:
            raise RuntimeError("--dump-outputs: a sub-batch's result was not taken")
        out = {"counts": np.array(self.counts, np.float64)}
        for i, nm in enumerate(("maps", "hits", "pafs")):
            out[nm] = np.concatenate([self.parts[j][i] for j in self.held]).astype(np.float64)
        room = DUMP_MAX_BYTES - sum(a.nbytes for nm, a in out.items() if nm != "hits")
        if out["hits"].nbytes > room:
            out["hits"] = out["hits"][:max(0, room // (8 * out["hits"].shape[1]))]
        return out


def write_outputs(outputs, path):
    import numpy as np
    os.makedirs(path, exist_ok=True)
    for nm, a in outputs.items():
        np.save(os.path.join(path, nm + ".npy"), a)
    print(f"bench: outputs of the step in {path}: " + ", ".join(f"{nm} {a.shape}" for nm, a in outputs.items()), file=sys.stderr)


def summarize(R, args, world, dev_name):
    """The JSON fields of one workload run (value, stage times, the two rooflines)."""
    W, wl, steps = R["W"], R["wl"], R["steps"]
    k, w = W["k"], W["w"]
    d = 2.0 / (w + 1)
    ms_per_step = R["elapsed"] / steps * 1e3
    value = R["total_bases"] * steps / R["elapsed"] / 1e9
    read_bases = wl.read_bases
    stats = R["stats"]
    hfrac = stats["index_hits"] / max(stats["read_mx"] or 1, 1)
    nb = len(wl.read_batches)

    def window(prof, nsteps):
        # the dominant kernel's own launches (round 6: a span around sketch_wave_kernel alone; "sketch_mask" also holds the block-minima
        # pass behind it, which is what rocprofv3's per-kernel average does not contain), or the window stage where that kernel does not run
        ms, n = prof.get("sketch_wave", (0.0, 0))
        if not n:
            ms, n = prof["sketch_mask"]
        per_step = n / max(nsteps, 1)
        avg = ms / max(n, 1)
        bpl = read_bases / max(per_step, 1)
        return avg, bpl, n

    avg_pipe, bases_per_launch, n_pipe = window(R["prof"], steps)
    if R["prof"].get("sketch_wave", (0.0, 0))[1]:
        wv_ms, wv_n = R["prof"]["sketch_wave"]
        mk_ms = R["prof"]["sketch_mask"][0]
        per_cycle = ms_per_step * steps / max(wv_n, 1)
        R["window_stream"] = {"what": "the window stream inside the timed steps, per sub-batch: a window kernel, then what stands between it and the next one "
                                      "(the block-minima pass over the strips it gave up, the exact pass, the next sketch's preparation, launch gaps)",
                              "cycle_ms": round(per_cycle, 4), "window_kernel_ms": round(wv_ms / max(wv_n, 1), 4),
                              "between_window_kernels_ms": round(per_cycle - wv_ms / max(wv_n, 1), 4),
                              "of_which_block_minima_pass_ms": round((mk_ms - wv_ms) / max(wv_n, 1), 4),
                              "note": "the gap is where the other stream's map kernels run at their stand-alone speed: closing it (the fallback passes on MAIN, "
                                      "profiles/HISTORY.md round 6) made every kernel shorter and the step longer"}
    if R["serial"]:
        avg_alone, _, n_alone = window(R["serial"]["prof"], R["serial"]["steps"])
    else:
        avg_alone, n_alone = avg_pipe, n_pipe
    bytes_per_launch = (0.25 + 16.0 * d) * bases_per_launch
    ach = lambda ms: bytes_per_launch / (ms * 1e-3) / 1e9 if ms > 0 else 0.0  # noqa: E731
    pm = pmc_summary(R["name"], args.scale, bases_per_launch)
    whole_b = 0.25 + d * (48.0 + 32.0 * hfrac)  # B = B_s + B_p + B_c with the measured hit fraction
    whole_gbs = whole_b * read_bases / (ms_per_step * 1e-3) / 1e9 if world == 1 else whole_b * R["total_bases"] / world / (ms_per_step * 1e-3) / 1e9
    mode = "two streams: window stage of sub-batch i+1 beside lookup/map of sub-batch i" if R["pipelined"] else "one stream (NTL_PIPELINE=0)"
    cfg = {"workload": f"{R['name']}: {len(wl.ctg_len)} contigs / {int(wl.ctg_len.sum())} bp assembly (sketched + indexed once: "
                       f"contig_stage_ms) + {read_bases} read bases per GPU per step ({int(sum(len(x) for x in wl.read_lens))} reads, mean {W['read_len']} bp, "
                       f"lognormal; generated on the device, {nb} distinct HBM-resident sub-batches), "
                       f"k={k} w={w} z=1000 x=0 sensitive={W['sensitive']} paf=True verbose=True",
           "scale": args.scale, "emulated_world": args.emulate_world or None, "hit_fraction": round(hfrac, 4),
           "read_minimizers_per_step": stats["read_mx"], "contig_minimizers": R["contig_mx"],
           "index_size": R["index_size"], "mappings_hits_pafs_per_step": list(stats["counts"]), "window_strips_per_step": stats.get("strips"),
           # k-mers of the reads / lane positions of their strips (a strip = one wavefront x 4096 positions): what the window kernel's lanes
           # roll that is a k-mer of a read -- the rest is the overlap of consecutive strips (w - 1 + 16 of 4096) and the empty end of a read's last strip
           "window_lane_utilisation": window_lane_utilisation(wl.read_lens, k, w),
           "device": dev_name, "gen_s": round(R["gen_s"], 2),
           "contig_stage_ms": round(R["contig_stage_ms"], 2),
           "contig_stage_kernels_ms": {nm: round(v[0], 3) for nm, v in R["contig_prof"].items() if v[1]},
           "value_incl_contig_stage_once": round(R["total_bases"] * steps / (R["elapsed"] + R["contig_stage_ms"] * 1e-3) / 1e9, 4),
           "timed_region_s": round(R["elapsed"], 3),
           "device_state_during_timed_steps": R.get("device_state"),
           "pipeline": {"value_measured_with": mode, "host_waits_per_step": 0,
                        "bench_streams": R["n_streams"]},
           "stage_ms_per_step": {nm: round(v[0] / steps, 3) for nm, v in R["prof"].items()},
           "stage_ms_note": "kernel spans inside the timed (pipelined) steps: they overlap each other, so they add up to more than ms_per_step; "
                            "kernels alone: serial_pass"}
    if R["serial"]:
        cfg["serial_pass"] = {"what": "the same steps on the same context with the second stream off, behind the timed region: one kernel at a time",
                              "steps": R["serial"]["steps"], "ms_per_step": round(R["serial"]["ms_per_step"], 3),
                              "Gbases_per_s": round(read_bases / (R["serial"]["ms_per_step"] * 1e-3) / 1e9, 2),
                              "stage_ms_per_step": {nm: round(v[0] / R["serial"]["steps"], 3) for nm, v in R["serial"]["prof"].items()}}
    # The headline figures (achieved, frac, avg_launch_ms) are those of the TIMED region -- the launches `value` is made of, where the kernel
    # shares the CUs with the previous sub-batch's lookup / map kernels on the other stream; `kernels_alone` holds the same kernel running
    # alone (the serial pass behind the timed region), which is what a rocprofv3 run with NTL_PIPELINE=0 sees.
    roof = {"bound": "valu", "bound_note": "what binds this kernel is VALU issue (integer rolling hash, no MFMA): `valu.frac` is the fraction of the SIMD cycles that "
                                           "the irreducible rolling work accounts for; `achieved` / `peak` / `frac` stay the HBM figures of the bench contract "
                                           "(algorithmic bytes / launch time / 8 TB/s), with `traffic` the counter bytes",
            "kernel": pm.get("kernel", "sketch window kernel (read batches)"),
            "achieved": round(ach(avg_pipe), 2), "peak": HBM_PEAK_GBS,
            "unit": "GB/s", "frac": round(ach(avg_pipe) / HBM_PEAK_GBS, 5), "traffic": pm.get("traffic"),
            "traffic_source": pm.get("traffic_source"),
            "bytes_per_base": round(0.25 + 16.0 * d, 4), "bases_per_launch": int(bases_per_launch),
            "avg_launch_ms": round(avg_pipe, 4), "launches": n_pipe,
            "measured_in": "timed region: HIP events on the window stream inside the pipelined steps (profiles/: the rocprofv3 kernel stats of this "
                           "same command); kernels_alone: the serial pass behind it (profiles/: the NTL_PIPELINE=0 runs)",
            "kernel_Gbases_per_s": round(bases_per_launch / (avg_pipe * 1e-3) / 1e9, 1) if avg_pipe > 0 else None,
            "kernels_alone": {"avg_launch_ms": round(avg_alone, 4), "launches": n_alone, "achieved": round(ach(avg_alone), 2),
                              "frac": round(ach(avg_alone) / HBM_PEAK_GBS, 5),
                              "kernel_Gbases_per_s": round(bases_per_launch / (avg_alone * 1e-3) / 1e9, 1) if avg_alone > 0 else None,
                              "measured_in": "serial pass behind the timed region" if R["serial"] else "timed region (no serial pass)"},
            "whole_path": {"bytes_per_base": round(whole_b, 4), "formula": "0.25 + d (48 + 32 h), SURVEY 8(d), h = measured hit fraction",
                           "achieved": round(whole_gbs, 1), "unit": "GB/s per GPU", "frac": round(whole_gbs / HBM_PEAK_GBS, 5)},
            "note": "integer/VALU-bound kernel (SURVEY 7): the 60 % HBM target of north_star is out of reach for a rolling hash (about 100 integer "
                    "operations per algorithmic byte); the roof that binds is VALU issue, in `valu`",
            "window_stream": R.get("window_stream"),
            "valu": valu_roofline(dict(pm, strips_per_launch=(stats.get("strips") or 0) / max(nb, 1) or None,
                                       scan_rounds_per_strip=float(-(-int(4096 * 10 / w) // 64))), avg_alone, bases_per_launch)}
    if roof["valu"]:
        roof["valu"]["measured_in"] = "kernels alone (the PMC passes run with NTL_PIPELINE=0)"
    return value, ms_per_step, cfg, roof


def main():
    args = parse_args()
    if args.strong and args.weak:
        sys.exit("--strong and --weak exclude each other")
    args.strong = not args.weak  # total work fixed at the workload's read set whatever N: configs[3]; at N = 1 the two are the same run
    if args.gpus > 1 and "RANK" not in os.environ:
        sys.exit(spawn_ranks(args))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
    if args.spawn_check:  # CPU-only: proves that --gpus N yields N communicating ranks
        import torch
        import torch.distributed as dist
        dist.init_process_group("gloo")
        t = torch.ones(1)
        dist.all_reduce(t)
        if dist.get_rank() == 0:
            print(json.dumps({"spawn_check": True, "n_gpus": int(t.item()), "world": dist.get_world_size()}), flush=True)
        dist.destroy_process_group()
        return
    sys.path.insert(0, ROOT)
    from ntlink_amd.dist_pair import pin_rank, LAST_PIN
    try:
        cores_mine = pin_rank(local_rank, local_world)
    except Exception as exc:  # pinning is an optimisation: an unexpected /sys layout must not cost the run
        print(f"bench: pin_rank failed ({type(exc).__name__}: {exc}); running unpinned", file=sys.stderr)
        cores_mine = None
    import torch
    from ntlink_amd import capi
    use_cuda = args.lib is None
    if use_cuda:
        torch.cuda.set_device(local_rank)
    comm = Comm(use_cuda, local_rank)
    dev = capi.Device(local_rank if use_cuda else 0, lib_path=args.lib)

    R = run_workload(dev, comm, args.workload, args, args.steps, args.warmup, rank, world, args.serial_steps, dump=bool(args.dump_outputs) and rank == 0)
    if R["outputs"] is not None:
        write_outputs(R["outputs"], args.dump_outputs)
    if rank == 0:
        value, ms_per_step, cfg, roof = summarize(R, args, world, dev.name)
        out = {
            "metric": "read Gbases/s mapped (ntLink pair, paf=True)",
            "value": round(value, 4), "unit": "Gbases/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3), "higher_is_better": True, "scaling": "strong" if args.strong else "weak",
            "vs_baseline": None, "dtype": "u64", "data": "synthetic",
            "config": cfg, "roofline": roof,
            "per_rank_ms_per_step": [round(x, 3) for x in R["per_rank_ms"]],
            "per_rank_bases_per_step": [int(x) for x in R["per_rank_bases"]],
            "world_size": world, "rccl_ranks_seen": R["ranks_seen"], "ranks": R["ranks"],
            "sub_batches_per_rank": len(R["wl"].read_batches), "batch_bases": R["batch_bases"],
            "scaling_note": ("this line is one of the driver's 1/2/4/8 runs" if world > 1 else
                             "N = 1.  No 1 -> 8 GPU curve has been measured on hardware by the builder (no multi-GPU box in reach): other_workloads.C3_one_rank_of_8 "
                             "is one rank's share on this GPU, profiles/r06_dist_host_scaling.json what 1 / 2 / 4 / 8 file-to-file ranks do to one host"),
        }
        if cores_mine:
            out["cores_per_rank"] = cores_mine
            out["pin_rank0"] = dict(LAST_PIN)
        if world == 1 and args.full and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(dev, R["wl"], R["W"], R["params"])
        if world == 1 and args.full and not args.no_e2e and use_cuda:
            for h in R["wl"].read_batches:
                h.close()
            R["wl"].read_batches = []
            with stdout_to_stderr():  # the driver logs its steps on stdout as the reference does (bin/ntlink_pair.py:540-606); stdout is the JSON line's
                out["end_to_end"] = end_to_end(dev, R["wl"], R["W"], args)
    R["ix"].close(); R["csk"].close(); R["wl"].close()
    if world == 1 and rank == 0 and args.full and not args.no_others and args.scale == 1.0:
        # the other single-GPU configurations of BASELINE.json under the same clock (fewer steps; same definitions)
        others = {}
        for name, st in (("C2", 200), ("C5", 3)):
            if name == args.workload:
                continue
            try:
                Ro = run_workload(dev, comm, name, args, st, 1, 0, 1, 1)
                v, ms, cfg_o, roof_o = summarize(Ro, args, 1, dev.name)
                others[name] = {"value": round(v, 3), "unit": "Gbases/s", "ms_per_step": round(ms, 3), "steps": st,
                                "workload": cfg_o["workload"], "hit_fraction": cfg_o["hit_fraction"],
                                "stage_ms_per_step": cfg_o["stage_ms_per_step"], "serial_pass": cfg_o.get("serial_pass"),
                                "window_kernel": {key: roof_o[key] for key in ("kernel", "avg_launch_ms", "bases_per_launch", "kernel_Gbases_per_s", "achieved", "frac", "kernels_alone", "traffic", "traffic_source")},
                                "whole_path": roof_o["whole_path"], "valu": roof_o["valu"]}
                Ro["ix"].close(); Ro["csk"].close(); Ro["wl"].close()
            except Exception as exc:  # the headline line must not be lost to a failure behind it: said, not hidden
                others[name] = {"error": f"{type(exc).__name__}: {exc}"}
        # BASELINE configs[3] seen from ONE rank of eight: this GPU takes the eighth of C3's reads (and the sub-batch size) that a rank of
        # `--gpus 8` takes -- what a rank does when its seven neighbours do not get in its way (they share the host, not the GPU).  The
        # driver's 1/2/4/8 curve is the measurement; this line is the per-rank rate to read it against.
        if args.workload == "C3":
            try:
                import copy
                a8 = copy.copy(args)
                a8.emulate_world, a8.strong = 8, True
                Re = run_workload(dev, comm, "C3", a8, 40, 3, 0, 1, 0)
                v, ms, cfg_e, _roof_e = summarize(Re, a8, 1, dev.name)
                others["C3_one_rank_of_8"] = {"value": round(v, 3), "unit": "Gbases/s per rank", "ms_per_step": round(ms, 3), "steps": 40,
                                              "read_bases_per_step": int(Re["total_bases"]), "sub_batches": len(Re["wl"].read_batches),
                                              "times_8": round(8 * v, 1),
                                              "note": "--emulate-world 8 on this one GPU; times_8 = eight such ranks if nothing but the host is shared"}
                Re["ix"].close(); Re["csk"].close(); Re["wl"].close()
            except Exception as exc:
                others["C3_one_rank_of_8"] = {"error": f"{type(exc).__name__}: {exc}"}
        # the dense sketches of the stages around `pair` (ntLink:243-251 k15 w5 on contig ends;
        # bin/ntlink_patch_gaps.py:417-441 k20 w10 on read pieces) on today's kernels, with the same two rooflines
        for name, (kk, ww) in (("f3_k15_w5", (15, 5)), ("f4_k20_w10", (20, 10))):
            try:
                others[name] = dense_sketch_line(dev, kk, ww)
            except Exception as exc:
                others[name] = {"error": f"{type(exc).__name__}: {exc}"}
        out["other_workloads"] = others
    if rank == 0:
        print(json.dumps(out), flush=True)
    dev.close()
    comm.close()


def pmc_summary(workload, scale, bases_per_launch):
    """HBM bytes and VALU instructions per launch of the dominant kernel from the rocprofv3 PMC passes of this
    same command (tools/gpu_round3.sh: FETCH_SIZE, WRITE_SIZE and the SQ counters in separate --pmc runs; PMC
    counters cannot be read from inside the process).  profiles/traffic.json records the kernel sources and the
    bases per launch it was taken on: anything else is reported as stale, not quoted."""
    path = os.path.join(ROOT, "profiles", "traffic.json")
    if scale != 1.0 or not os.path.exists(path):
        return {}
    t = json.load(open(path)).get(workload)
    if not t:
        return {}
    if t.get("kernel_signature") != kernel_signature() or abs(t.get("bases_per_launch", 0) - bases_per_launch) > 0.02 * bases_per_launch:
        return {"traffic": None, "traffic_source": "stale: profiles/traffic.json was taken on other kernel sources or launch sizes"}
    return {"traffic": t["bytes_per_launch"], "traffic_source": t["source"], "kernel": t.get("kernel"),
            "valu_wave_instr_per_launch": t.get("valu_wave_instr_per_launch"), "valu_source": t.get("valu_source"),
            "measured_cycles_per_wave_instr": t.get("measured_cycles_per_wave_instr"),
            "profiled_launch_ms": t.get("profiled_launch_ms"),
            "clock_ghz": t.get("clock_ghz"), "isa_mix": t.get("isa_mix")}


def dense_sketch_line(dev, k, w, bases=200_000_000, reps=5):
    """Sketch rate at the window sizes of the stages around `pair`: a minimizer every (w + 1) / 2 bases, so the records (16 B each) are most of
    the bytes and the windows are too small for the threshold-sparsified pass (every k-mer would be a candidate).  Round 6:
    sketch_small_kernel<W> (2 <= w <= 15: 16 k-mers per lane, the minima of a lane's windows in registers, exact 64-bit hashes; the
    round-1 form -- four k-mers per lane, NTL_SKETCH_SMALL=0 -- made 226-238 Gbases/s in its window pass) + emit_kernel.  These stages
    sketch contig ends and read pieces -- megabases, not the read set -- so the line is here for the record, not as a target."""
    import numpy as np
    b = dev.synth_genome(77, np.full(bases // 2_000_000, 2_000_000, np.uint32))
    try:
        with dev.sketch(b, k, w) as sk:
            n = sk.count
            from_lists = sk.from_lists
        dev.sync()
        dev.prof_enable(True)
        dev.prof_reset()
        t0 = time.perf_counter()
        for _ in range(reps):
            with dev.sketch(b, k, w) as sk:
                sk.wait()
        dev.sync()
        dt = (time.perf_counter() - t0) / reps
        prof = {nm: round(dev.prof_get(nm)[0] / reps, 4) for nm in ("sketch_meta", "sketch_mask", "sketch_redo", "sketch_emit")}
    finally:
        b.close()
    d = n / bases
    bpb = 0.25 + 16.0 * d
    win_ms = prof["sketch_mask"] + prof["sketch_redo"]
    return {"workload": f"{bases} bp of random sequence in 2-Mbp pieces, k={k} w={w}, one sketch call (records, no lookup)", "minimizers": int(n),
            "density": round(d, 4), "value": round(bases / dt / 1e9, 1), "unit": "Gbases/s", "ms_per_sketch": round(dt * 1e3, 3),
            "records_G_per_s": round(n / dt / 1e9, 2), "stage_ms": prof, "window_pass": "per-strip lists" if from_lists else ("bitmask (sketch_small_kernel, exact 64-bit pass, window minima in registers)"
                                                                if 2 <= w <= 15 and os.environ.get("NTL_SKETCH_SMALL", "1") != "0" and not os.environ.get("NTL_SKETCH_C")
                                                                else "bitmask (sketch_mask_kernel, exact 64-bit pass)"),
            "roofline": {"bound": "hbm", "bytes_per_base": round(bpb, 3), "formula": "0.25 + 16 d (packed bases in, 16-byte records out)",
                         "achieved": round(bpb * bases / (dt * 1e-0) / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": round(bpb * bases / dt / 1e9 / HBM_PEAK_GBS, 4),
                         "window_kernel": {"ms": round(win_ms, 4), "Gbases_per_s": round(bases / (win_ms * 1e-3) / 1e9, 1) if win_ms > 0 else None},
                         "emit_kernel": {"ms": prof["sketch_emit"],
                                         "GB_per_s_of_records": round(16.0 * n / (prof["sketch_emit"] * 1e-3) / 1e9, 1) if prof["sketch_emit"] > 0 else None}}}


VALU_FLOOR_PER_KMER = 9.0
# the floor's instructions by issue class (profiles/valu_cycles.json): the rolling step of skw_step in the shipped ISA + one address operation
VALU_FLOOR_CLASSES = (("v_alignbit_b32", 2), ("v_xor_b32", 2), ("v_lshrrev_b32", 1), ("v_add_u32", 2), ("vopc", 1), ("v_bfe_u32", 1))


def valu_class_cycles(cls):
    tab = getattr(valu_class_cycles, "tab", None)
    if tab is None:
        try:
            tab = json.load(open(os.path.join(ROOT, "profiles", "valu_cycles.json")))["cycles"]
        except (OSError, ValueError, KeyError):
            tab = {}
        valu_class_cycles.tab = tab
    return float(tab.get(cls, 4.2))


def window_lane_utilisation(read_lens, k, w):
    """k-mers of the reads / lane-steps the window kernel rolls for them.  The strip geometry of sketch_wave_kernel (ntl_hip.hip
    sketch_geometry, sketch2_kernels.h skw_per_lane): a read of M k-mers is cut into strips of 4096 elements that start NWO apart;
    a wavefront rolls 64 lanes x 64 steps over a strip, 64 x (16, 32 or 48) over a read's short last strip.  What is not a read's k-mer:
    the w - 1 + 16 elements consecutive strips share, and the unused end of the last strip's last sixteen-step block."""
    import numpy as np
    if not (94 <= w <= 255 and k <= 64):
        return None
    nwo = (256 - ((w - 16) // 16 + 2)) * 16 - 1
    M = np.concatenate([np.asarray(x, np.int64) for x in read_lens]) - (k - 1)
    M = M[M >= w]
    n = (M - w + nwo) // nwo  # strips of each read
    steps, i = 0, 0
    while True:
        m = M[n > i]
        if not len(m):
            break
        hi = np.minimum(4096, m - i * nwo + 1)
        steps += int(np.where(hi > 3072, 64, 16 * ((hi + 1023) // 1024)).sum()) * 64
        i += 1
    return round(float(M.sum()) / steps, 4) if steps else None


def valu_roofline(pm, avg_launch_ms, bases_per_launch):
    """The roof that binds the window kernel: VALU issue.
      measured  SIMD cycles per VALU wave-instruction of the profiled launches = 1024 SIMDs x (GRBM_GUI_ACTIVE / 8 XCDs) / SQ_INSTS_VALU
                (PMC pass of this same command, profiles/traffic.json) -- every cycle of every SIMD, busy or not, per instruction;
      priced    what the instructions would cost if each issued at its calibrated class cost (profiles/valu_cycles.json: 2.4 cycles for
                the plain two-operand integer ops, 4.0-4.4 for the rest) with the kernel's own mix: the compiler's assembly, basic blocks
                weighted by loop depth (tools/isa_mix.py: depth 1 = once per strip, depth 2 = the scan rounds of a strip, depth 3 = the
                scan steps, fitted so that the total is the instruction count the profiler saw);
      frac      = priced / measured: the share of the SIMD cycles that the kernel's own instruction stream accounts for.  No clamp.
      peak      = 1024 SIMDs x clock / priced (G wave-instr/s), achieved = instructions / launch time, both of the profiled launches
                (so that achieved / peak = frac); this run's unprofiled launch time beside them."""
    n = pm.get("valu_wave_instr_per_launch")
    meas = pm.get("measured_cycles_per_wave_instr")
    if not n or avg_launch_ms <= 0:
        return None
    t_prof = pm.get("profiled_launch_ms") or avg_launch_ms
    ach = n / (t_prof * 1e-3)  # of the PROFILED launches: their clock is the one that is known (GRBM_GUI_ACTIVE), so achieved / peak = frac
    lipb = n * 64.0 / bases_per_launch
    out = {"achieved": round(ach / 1e9, 2), "unit": "G wave-instr/s", "lane_instr_per_base": round(lipb, 2),
           # what ANY rolling implementation of this key pays per k-mer, counted in the shipped ISA of skw_step: two v_alignbit, two v_xor,
           # v_lshrrev, v_lshlrev, v_add (the key), v_cmp (the candidate test) + one instruction for the address of the step's seed pair;
           # useful_frac = floor / measured says how much of what the kernel issues is that work -- the rest is the first k-mer of a lane,
           # the seed addresses' bytes, the candidate lists, the scans, and the lanes that roll no k-mer of a read (window_lane_utilisation)
           "floor_lane_instr_per_base": VALU_FLOOR_PER_KMER, "useful_frac": round(VALU_FLOOR_PER_KMER / lipb, 3),
           "source": pm.get("valu_source"), "profiled_launch_ms": t_prof,
           "this_run": {"avg_launch_ms": round(avg_launch_ms, 4), "achieved": round(n / (avg_launch_ms * 1e-3) / 1e9, 2),
                        "note": "unprofiled launches of this run: the chip holds a higher clock without the profiler (MI355X_MICROARCH.md, DVFS), which this process cannot read"}}
    priced = priced_cycles(pm, n)
    if meas and priced:
        clock = pm.get("clock_ghz") or 0.0
        # frac (round 6): the FLOOR's instructions at their calibrated issue cost / the SIMD cycles the launch took.  The
        # floor per k-mer (VALU_FLOOR_CLASSES): what any rolling implementation of this key issues.  It can show waste; the figure that cannot
        # -- the kernel's OWN mix priced against its own cycles, 1.0 by construction when the VALU pipe never idles -- is kept as
        # `issue_slots_filled`, which only says that the pipe is full, not that it is full of useful work.
        floor_cycles = sum(n_i * valu_class_cycles(cls) for cls, n_i in VALU_FLOOR_CLASSES)
        useful = floor_cycles * (bases_per_launch / 64.0) / (meas * n)
        out.update({"measured_cycles_per_wave_instr": meas, "priced_cycles_per_wave_instr": priced["cycles"],
                    "frac": round(useful, 3),
                    "frac_is": "floor instructions (VALU_FLOOR_CLASSES: 2 v_alignbit + 2 v_xor + v_lshrrev + 2 v_add + v_cmp + 1 address op per k-mer) x their "
                               "calibrated issue cycles (profiles/valu_cycles.json) x k-mers per launch / 64, over the SIMD cycles of the launch "
                               "(1024 SIMDs x GRBM_GUI_ACTIVE / 8 = measured cycles per wave-instruction x SQ_INSTS_VALU)",
                    "floor_cycles_per_kmer_step": round(floor_cycles, 2),
                    "issue_slots_filled": round(priced["cycles"] / meas, 3),
                    "issue_slots_filled_is": "the kernel's own instruction mix at its calibrated cost / measured SIMD cycles per VALU wave-instruction: ~1 = the VALU "
                                             "pipe is never idle; says nothing about how useful the instructions are (that is `frac` / `useful_frac`)",
                    "peak": round(N_SIMD * clock / priced["cycles"], 1), "clock_ghz": clock,
                    "priced_from": priced["how"], "isa_mix": pm.get("isa_mix"),
                    "note": "SQ_ACTIVE_INST_VALU is not used: in these counter files it equals SQ_INSTS_VALU"})
    return out


def priced_cycles(pm, n_instr):
    """Class-priced cycles per wave-instruction of the profiled kernel from its loop-depth-weighted ISA mix (tools/isa_mix.py)."""
    path = pm.get("isa_mix")
    if not path or not os.path.exists(os.path.join(ROOT, path)):
        return None
    mix = json.load(open(os.path.join(ROOT, path)))["kernels"]
    kern = next((v for k, v in mix.items() if (pm.get("kernel") or "").replace("void ", "").strip() in k), None)
    if kern is None:
        return None
    d = {int(k): v for k, v in kern["by_depth"].items()}
    strips = pm.get("strips_per_launch")
    per_strip = n_instr * 64.0 / 64.0 / strips if strips else None  # wave-instructions per strip (one wavefront per strip)
    rounds = pm.get("scan_rounds_per_strip") or 3.0
    w = {0: 0.0, 1: 1.0, 2: rounds, 3: 0.0}
    fixed = sum(w[k] * d[k]["valu"] for k in d if k in w and k != 3)
    how = f"depth 1 x 1, depth 2 x {rounds} rounds"
    if 3 in d and d[3]["valu"]:
        fit = (per_strip - fixed) / d[3]["valu"] if per_strip else -1.0  # what is left of the counted instructions would be scan steps
        if fit > 0:
            w[3] = fit
            how += f", depth 3 x {w[3]:.1f} (fitted to {per_strip:.0f} VALU wave-instructions per strip)"
        else:  # the straight-line count already exceeds what was counted (blocks of other k, of a sequence's last strip ... are skipped)
            w[3] = rounds * 5.5
            how += f", depth 3 x {w[3]:.1f} (5.5 scan steps per round and side; the profiler counted {per_strip or 0:.0f} VALU wave-instructions per strip, fewer than the straight-line code holds: only the RATIO of the weights enters)"
    tot_i = sum(w.get(k, 0.0) * d[k]["valu"] for k in d)
    tot_c = sum(w.get(k, 0.0) * d[k]["priced_cycles"] for k in d)
    return {"cycles": round(tot_c / tot_i, 3), "how": how} if tot_i else None


def cpu_budget():
    """(CPUs this process may run on, CPU quota of its cgroup in cores or None): a container often sees every CPU of the host
    and is held to a fraction of them by cpu.max -- the GPU boxes of this project: 256 visible, 16 granted."""
    vis = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = float(q) / float(per)
    except (OSError, ValueError):
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                quota = q / per
        except (OSError, ValueError):
            pass
    return vis, quota


def cpu_baseline(dev, wl, W, params):
    """The oracle (C restatement of indexlr + the ntlink_pair mapping loop, parity-pinned) timed on this host,
    stage by stage, on a bounded sample of the same workload: all contigs + 1/30 of one coverage of reads.
    kind = "port": the literal reference cannot run here (btllib absent; its Python does not travel).
    Reference-faithful settings next to best-effort ones: indexlr runs with t=4 by default (ntLink:27) and
    ntlink_pair.py maps on one thread (bin/ntlink_pair.py:336-414)."""
    import numpy as np
    import oracle
    visible, quota = cpu_budget()
    # threads of the "all cores" legs: every visible CPU, or -- under a CPU quota -- twice the quota (more runnable threads than
    # granted cores only buy throttling: the 256-thread run of the scaling sweep below is the slowest of all)
    cores = visible if quota is None else max(1, min(visible, int(round(2 * quota))))
    k, w = W["k"], W["w"]
    T = {}

    def lap(name, t0):
        T[name] = max(round(time.perf_counter() - t0, 4), 1e-4)

    t0 = time.perf_counter()
    cbuf, coff = wl.contigs.download()
    sample_bases = max(int(wl.contigs.bases), 1)  # one coverage / 30 x 30 = as many read bases as the assembly has, capped
    sample_bases = min(sample_bases, 3_000_000_000)
    rb, rl = wl.make_reads(sample_bases, seed=(99, 0))
    rbuf, roff = rb.download()
    rb.close()
    lap("download_sample", t0)
    nreads = len(rl)
    small = max(1, nreads // 8)  # the slow reference-faithful settings run on 1/8 of the sample
    t0 = time.perf_counter()
    co, ch, cp, cs = oracle.sketch_batch(cbuf, coff, k, w, threads=cores)
    lap("contig_sketch_all_cores", t0)
    t0 = time.perf_counter()
    cid = np.repeat(np.arange(len(co) - 1, dtype=np.uint32), np.diff(co).astype(np.int64))
    ix = oracle.Index(ch, cid, cp, cs)
    lap("index_build_1_thread", t0)
    t0 = time.perf_counter()
    oracle.sketch_batch(rbuf[:int(roff[small])], roff[:small + 1], k, w, threads=4)
    lap("read_sketch_t4", t0)
    t4_bases = int(roff[small])
    # where the record-parallel sketch stops scaling on this host: the same 1/8 sample at 16 and 64 threads
    scaling = {"4": round(t4_bases / T["read_sketch_t4"] / 1e6, 1)}
    for nt in (16, 64, visible):
        if nt != cores and nt <= visible and str(nt) not in scaling:
            t0 = time.perf_counter()
            oracle.sketch_batch(rbuf[:int(roff[small])], roff[:small + 1], k, w, threads=nt)
            scaling[str(nt)] = round(t4_bases / max(time.perf_counter() - t0, 1e-4) / 1e6, 1)
    # the all-cores leg, twice: the first call also pays for creating the thread team and first-touching the output arrays
    t0 = time.perf_counter()
    ro, rh, rp, rs = oracle.sketch_batch(rbuf, roff, k, w, threads=cores)
    lap("read_sketch_all_cores_first_call", t0)
    t0 = time.perf_counter()
    ro, rh, rp, rs = oracle.sketch_batch(rbuf, roff, k, w, threads=cores)
    lap("read_sketch_all_cores", t0)
    kw = dict(k=params["k"], z=params["z"], x=params["x"], sensitive=params["sensitive"], repeat_filter=params["repeat_filter"])
    t0 = time.perf_counter()
    oracle.map_reads(ix, wl.ctg_len, ro[:small + 1], rl[:small], rh, rp, rs, threads=1, **kw)
    lap("map_1_thread", t0)
    t0 = time.perf_counter()
    res = oracle.map_reads(ix, wl.ctg_len, ro, rl, rh, rp, rs, threads=cores, **kw)
    lap("map_read_parallel", t0)
    bases = int(roff[-1])
    # whole-sample rates; the contig work is amortised over a 30x read set, so the read stages are what scales
    best = bases / (T["read_sketch_all_cores"] + T["map_read_parallel"]) / 1e9
    faithful = 1.0 / (T["read_sketch_t4"] / t4_bases + T["map_1_thread"] / t4_bases) / 1e9
    per_thread_t4 = t4_bases / T["read_sketch_t4"] / 4.0
    return {"value": round(best, 4), "unit": "Gbases/s", "cores": cores if quota is None else round(quota, 1), "kind": "port",
            "cpus_visible": visible, "cpu_quota_cores": quota, "threads_used": cores,
            "sample": f"all {len(wl.ctg_len)} contigs + {nreads} reads ({bases} bases, one coverage of the assembly) of the same generator; "
                      f"value = read sketch + read-parallel map on {cores} threads (second call: thread team and output pages warm); reference-faithful settings "
                      f"(indexlr t=4, map on 1 thread) timed on the first {small} reads ({t4_bases} bases)",
            "reference_faithful": {"value": round(faithful, 4), "unit": "Gbases/s", "cores": 4,
                                   "what": "indexlr -t 4 (ntLink:27) piped into a single-threaded map loop; the pipe overlaps them, "
                                           "so the true rate lies between this serial figure and the slower of the two stages"},
            "if_it_scaled": {"value": round(1.0 / (1.0 / (per_thread_t4 * (quota or cores)) + T["map_read_parallel"] / bases) / 1e9, 3), "unit": "Gbases/s",
                             "what": f"per-thread sketch rate at t=4 ({per_thread_t4 / 1e6:.1f} Mbases/s/thread) x {quota or cores:g} granted cores + the measured read-parallel map: "
                                     "the ceiling of the same code if it scaled perfectly over the cores this process is granted"},
            "stages_s": T,
            "read_sketch_scaling_Mbases_per_s": dict(scaling, **{str(cores): round(bases / T["read_sketch_all_cores"] / 1e6, 1)}),
            "stage_rates": {"read_sketch_t4_Mbases_per_s": round(t4_bases / T["read_sketch_t4"] / 1e6, 1),
                            "read_sketch_all_cores_Mbases_per_s": round(bases / T["read_sketch_all_cores"] / 1e6, 1),
                            "read_sketch_all_cores_first_call_Mbases_per_s": round(bases / T["read_sketch_all_cores_first_call"] / 1e6, 1),
                            "map_1_thread_Mbases_per_s": round(t4_bases / T["map_1_thread"] / 1e6, 1),
                            "map_read_parallel_Mbases_per_s": round(bases / T["map_read_parallel"] / 1e6, 1),
                            "contig_sketch_all_cores_Mbases_per_s": round(int(coff[-1]) / T["contig_sketch_all_cores"] / 1e6, 1)},
            "python_reference_calibration": "BASELINE.md section 2: the real ntlink_pair.py loop maps 0.9-2.3 M minimizers/s on one thread",
            "mappings": int(len(res["maps"]))}


def write_fasta(path, buf, off, prefix):
    with open(path, "wb", buffering=1 << 24) as f:
        mv = memoryview(buf)
        for i in range(len(off) - 1):
            f.write(b">%s%d\n" % (prefix, i))
            f.write(mv[int(off[i]):int(off[i + 1])])
            f.write(b"\n")


def end_to_end(dev, wl, W, args):
    """File to file on the same workload: FASTA in the page cache -> <target>.kK.wW.tsv, .verbose_mapping.tsv,
    .paf, .pairs.tsv, .scaffold.dot on disk (the five outputs of `ntLink pair ... paf=True`), through the pair
    driver (parser threads -> PCIe -> device -> text emitters).  Reported beside `value`, never as it."""
    import shutil
    import tempfile
    sys.path.insert(0, ROOT)
    from ntlink_amd import pipeline
    bases = int(min(args.e2e_bases, W["read_bases"]))
    base_dir = "/dev/shm" if os.path.isdir("/dev/shm") and shutil.disk_usage("/dev/shm").free > 4 * (bases + wl.contigs.bases) else None
    d = tempfile.mkdtemp(prefix="ntl_e2e_", dir=base_dir)
    try:
        t0 = time.perf_counter()
        cbuf, coff = wl.contigs.download()
        write_fasta(os.path.join(d, "asm.fa"), cbuf, coff, b"ctg")
        del cbuf
        files = []
        per = int(args.batch_bases)
        nb = max(1, -(-bases // per))
        for b in range(nb):
            rb, _ = wl.make_reads(bases // nb, seed=(77, b))
            rbuf, roff = rb.download()
            rb.close()
            p = os.path.join(d, f"reads_{b:02d}.fa")
            write_fasta(p, rbuf, roff, b"r%d_" % b)
            files.append(os.path.basename(p))
            del rbuf
        prep_s = time.perf_counter() - t0
        cwd = os.getcwd()
        os.chdir(d)
        try:
            # `value` = the FIRST pass of this process over all the read files: a real `ntLink pair` is one process and one pass
            # (ntLink:221-225).  Two more passes follow for the steady state (page-locked staging buffers, worker contexts and
            # thread pools exist by then): listed, not the headline.
            runs, stats_all = [], []
            for _ in range(3):
                for f in os.listdir(d):
                    if f.startswith("asm.fa."):
                        os.remove(os.path.join(d, f))
                pin0, mal0 = (dev.pin_alloc_s, dev.pin_alloc_bytes), dev.prof_get("hipMalloc")
                t0 = time.perf_counter()
                st_i = pipeline.run_pair(dev, "asm.fa", " ".join(files), k=W["k"], w=W["w"], paf=True, pairs_tsv=True,
                                         sensitive=W["sensitive"])
                runs.append(round(time.perf_counter() - t0, 3))
                mal1 = dev.prof_get("hipMalloc")
                st_i["one_time"] = {"page_lock_s": round(dev.pin_alloc_s - pin0[0], 3), "page_locked_MB": round((dev.pin_alloc_bytes - pin0[1]) / 1e6),
                                    "hipMalloc_s_main_context": round((mal1[0] - mal0[0]) / 1e3, 3), "hipMalloc_calls_main_context": int(mal1[1] - mal0[1])}
                stats_all.append(st_i)
            st, dt = stats_all[0], runs[0]
            best = min(range(3), key=lambda i: runs[i])
        finally:
            os.chdir(cwd)
        out_bytes = sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d) if f.startswith("asm.fa."))
        text_bytes = sum(os.path.getsize(os.path.join(d, f)) for f in files)
        try:
            rates = host_rates()
        except Exception as exc:
            rates = {"error": f"{type(exc).__name__}: {exc}"}
        gz = {}
        try:  # the forms reads really arrive in (ntLink:113-117,222: `gzip -cd -f FILES`): several .fq.gz files, one bgzip'd file
            gz = gz_forms(dev, d, files[0], W, cwd)
        except Exception as exc:
            gz = {"error": f"{type(exc).__name__}: {exc}"}
        def stage_times(x):
            return {"t_contig_stage": round(x["t_contigs"], 3), "t_wait_for_ingest": round(x["t_ingest"], 3), "t_device_incl_pack_pcie": round(x["t_device"], 3),
                    "t_handover": round(x["t_handover"], 3), "t_write": round(x.get("t_write", 0), 3), "t_tally": round(x.get("t_tally", 0), 3),
                    "t_drain_tail": round(x.get("t_drain_tail", 0), 3), "t_graph": round(x.get("t_graph", 0), 3)}
        return {"value": round(st["read_bases"] / dt / 1e9, 3), "unit": "Gbases/s", "seconds": round(dt, 3), "runs_s": runs,
                "runs_note": "value = the FIRST pass of the process over all read files (first call: page-locked staging buffers, worker contexts "
                             "and thread pools are made on the way; stage times below are that run's); steady_state = the faster of the two passes behind it",
                "steady_state": {"value": round(stats_all[best]["read_bases"] / runs[best] / 1e9, 3), "unit": "Gbases/s", "seconds": runs[best],
                                 "run": best, **stage_times(stats_all[best])},
                "one_time_costs_per_run": [x.get("one_time") for x in stats_all],
                "text_formatted_on": "device (ntl_mapres_format)" if os.environ.get("NTL_DEVICE_TEXT", "1") != "0" else "host (ntl_write_verbose / ntl_write_paf)",
                "compressed_inputs": gz,
                "host_rates": rates,
                "roofline": {"first_pass": e2e_roofline(rates, st["read_bases"], text_bytes, out_bytes, dt, cpu_budget()),
                             "steady_state": e2e_roofline(rates, stats_all[best]["read_bases"], text_bytes, out_bytes, runs[best], cpu_budget()),
                             "compressed": {nm: {"inflate_bound_s": round(2.0 * g["read_bases"] / (rates["inflate_GBps_per_core_zlib_of_sequence_text"] * 1e9 *
                                                                                                    max(1, int(cpu_budget()[1] or cpu_budget()[0]))), 4),
                                                 "measured_s": g["seconds"],
                                                 "note": "FASTQ text = 2 bytes per base through inflate on every granted core (zlib's rate; the reader uses libdeflate "
                                                         "where the box has it); one ordinary .gz member is ONE serial stream whatever inflates it"}
                                            for nm, g in gz.items() if isinstance(g, dict) and "read_bases" in g and rates.get("inflate_GBps_per_core_zlib_of_sequence_text")}},
                "host_cpu": dict(zip(("cpus_visible", "cpu_quota_cores"), cpu_budget())),
                "reader": st.get("reader"),
                "read_bases": st["read_bases"], "reads": st["reads"], "input": f"plain FASTA, {len(files)} read file(s), page cache ({d})",
                "output_bytes": out_bytes, "prepare_inputs_s": round(prep_s, 1),
                "t_contig_stage": round(st["t_contigs"], 3), "t_contig_stage_parts": st.get("t_contigs_parts"), "t_wait_for_ingest": round(st["t_ingest"], 3),
                "t_device_incl_pack_pcie": round(st["t_device"], 3), "t_device_parts": st.get("t_device_parts"), "t_handover": round(st["t_handover"], 3),
                "t_drain_tail": round(st.get("t_drain_tail", 0), 3), "t_graph": round(st.get("t_graph", 0), 3),
                "t_write": round(st.get("t_write", 0), 3), "t_tally": round(st.get("t_tally", 0), 3),
                "device_streams": int(os.environ.get("NTL_DEVICE_STREAMS", "2"))}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def host_rates():
    """What the file-to-file path is made of besides kernels, measured here on the cores this process is granted: PCIe both ways
    (1-GB page-locked torch tensors), the rate at which the granted cores move memory (numpy copies of 256-MB pieces on a thread per
    core: the parser reads every text byte once and writes a quarter of it packed), zlib inflate per core."""
    import threading
    import zlib
    import numpy as np
    import torch
    out = {}
    try:
        n = 1 << 30
        h = torch.empty(n, dtype=torch.uint8).pin_memory()
        g = torch.empty(n, dtype=torch.uint8, device="cuda")
        for name, (dst, src) in (("h2d_GBps", (g, h)), ("d2h_GBps", (h, g))):
            dst.copy_(src, non_blocking=True); torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                dst.copy_(src, non_blocking=True)
            torch.cuda.synchronize()
            out[name] = round(3 * n / (time.perf_counter() - t0) / 1e9, 1)
        del h, g
    except Exception as exc:  # a rate that cannot be measured is left out, not guessed
        out["pcie_error"] = f"{type(exc).__name__}: {exc}"
    vis, quota = cpu_budget()
    cores = max(1, int(quota or vis))
    cores = min(cores, 64)
    piece = 256 << 20
    src = [np.ones(piece, np.uint8) for _ in range(cores)]
    dst = [np.empty(piece, np.uint8) for _ in range(cores)]
    def work(i):
        for _ in range(4):
            np.copyto(dst[i], src[i])
    ths = [threading.Thread(target=work, args=(i,)) for i in range(cores)]
    t0 = time.perf_counter()
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    dt = time.perf_counter() - t0
    out["host_copy_GBps_read_plus_write"] = round(2 * 4 * piece * cores / dt / 1e9, 1)
    out["host_copy_threads"] = cores
    del src, dst
    text = (b"ACGTTGCA" * 8 + b"\n") * 200000
    comp = zlib.compress(text, 1)
    t0 = time.perf_counter()
    for _ in range(5):
        zlib.decompress(comp)
    out["inflate_GBps_per_core_zlib_of_sequence_text"] = round(5 * len(text) / (time.perf_counter() - t0) / 1e9, 2)
    return out


def e2e_roofline(rates, read_bases, text_bytes, out_bytes, seconds, cores):
    """Lower bounds of a file-to-file pass from the byte counts and the measured rates: which resource would bind if everything else were
    free, and how far the measured pass is from it."""
    b = {}
    if rates.get("host_copy_GBps_read_plus_write"):
        # the parser reads the text and writes 2 bits per base; the emitters write the output text once more into the page cache
        b["host_memory_s"] = round((text_bytes + 0.25 * read_bases + 2.0 * out_bytes) / (rates["host_copy_GBps_read_plus_write"] * 1e9), 4)
    if rates.get("h2d_GBps"):
        b["pcie_h2d_s"] = round(0.25 * read_bases / (rates["h2d_GBps"] * 1e9), 4)
    if rates.get("d2h_GBps"):
        b["pcie_d2h_s"] = round(out_bytes / (rates["d2h_GBps"] * 1e9), 4)
    if not b:
        return None
    binds = max(b, key=b.get)
    return {"bounds_s": b, "binds": binds, "measured_s": round(seconds, 3), "measured_over_bound": round(seconds / max(b[binds], 1e-9), 1),
            "bytes": {"text_in": int(text_bytes), "packed_over_pcie": int(0.25 * read_bases), "text_out": int(out_bytes)},
            "note": "host_memory_s prices every byte the host touches at the copy rate of the granted cores; the parser does more per byte than a copy "
                    "(newline and header scan, 2-bit pack with pext), which is the factor above it"}


def gz_forms(dev, d, fasta, W, cwd, max_bases=2_000_000_000):
    """The first reads file of the end-to-end leg again as (a) 16 gzip'd FASTQ files and (b) one BGZF (bgzip) FASTQ file, each mapped
    file to file against the same assembly.  The files are made here with zlib level 1 on a thread per file / per 16 blocks."""
    import struct
    import zlib
    from concurrent.futures import ThreadPoolExecutor
    from ntlink_amd import pipeline
    import numpy as np
    raw = np.fromfile(os.path.join(d, fasta), np.uint8, count=int(max_bases * 1.01))
    data = raw.tobytes()
    del raw
    recs = data.split(b">")[1:]
    if not data.endswith(b"\n"):
        recs = recs[:-1]
    nfiles = 16
    per = -(-len(recs) // nfiles)

    def fastq(rs):
        out = []
        for r in rs:
            nl = r.index(b"\n")
            seq = r[nl + 1:].rstrip(b"\n")
            out.append(b"@" + r[:nl] + b"\n" + seq + b"\n+\n" + b"I" * len(seq) + b"\n")
        return b"".join(out)

    def one_gz(i):
        txt = fastq(recs[i * per:(i + 1) * per])
        co = zlib.compressobj(1, zlib.DEFLATED, 31)
        with open(os.path.join(d, f"fq_{i:02d}.fq.gz"), "wb") as fh:
            fh.write(co.compress(txt) + co.flush())
        return txt

    t0 = time.perf_counter()
    with ThreadPoolExecutor(nfiles) as ex:
        texts = list(ex.map(one_gz, range(nfiles)))
    whole = b"".join(texts)
    del texts
    blocks = [whole[i:i + 0xFF00] for i in range(0, len(whole), 0xFF00)] + [b""]

    def bgzf_blocks(lo):
        out = []
        for ch in blocks[lo:lo + 64]:
            co = zlib.compressobj(1, zlib.DEFLATED, -15)
            body = co.compress(ch) + co.flush()
            out.append(b"\x1f\x8b\x08\x04" + b"\x00" * 4 + b"\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, 12 + 6 + len(body) + 8 - 1)
                       + body + struct.pack("<II", zlib.crc32(ch) & 0xFFFFFFFF, len(ch)))
        return b"".join(out)

    with ThreadPoolExecutor(32) as ex, open(os.path.join(d, "all.fq.bgz.gz"), "wb") as fh:
        for piece in ex.map(bgzf_blocks, range(0, len(blocks), 64)):
            fh.write(piece)
    del whole, blocks, recs, data
    prep_s = time.perf_counter() - t0
    out = {"prepare_s": round(prep_s, 1)}
    os.chdir(d)
    try:
        for name, reads in (("16_fq_gz_files", " ".join(f"fq_{i:02d}.fq.gz" for i in range(nfiles))), ("one_bgzf_fq_gz", "all.fq.bgz.gz")):
            runs, st, dt = [], None, None
            for _ in range(2):  # as in end_to_end: the faster of two runs, both listed (2 Gbases: 0.25 s of every run is the contig stage)
                for f in os.listdir(d):
                    if f.startswith("gzrun."):
                        os.remove(os.path.join(d, f))
                t0 = time.perf_counter()
                st_i = pipeline.run_pair(dev, "asm.fa", reads, prefix="gzrun", k=W["k"], w=W["w"], paf=True, pairs_tsv=True, sensitive=W["sensitive"],
                                         write_contig_tsv=False)
                dt_i = time.perf_counter() - t0
                runs.append(round(dt_i, 3))
                if dt is None or dt_i < dt:
                    st, dt = st_i, dt_i
            out[name] = {"value": round(st["read_bases"] / dt / 1e9, 3), "unit": "Gbases/s", "seconds": round(dt, 3), "runs_s": runs, "read_bases": st["read_bases"],
                         "t_contig_stage": round(st["t_contigs"], 3),
                         "value_behind_contig_stage": round(st["read_bases"] / max(dt - st["t_contigs"], 1e-9) / 1e9, 3),  # what a 90-Gbases input would see
                         "compressed_bytes": sum(os.path.getsize(os.path.join(d, x)) for x in reads.split())}
    finally:
        os.chdir(cwd)
    return out


if __name__ == "__main__":
    main()
