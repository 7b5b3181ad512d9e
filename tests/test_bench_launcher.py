"""bench.py --gpus N must run N ranks when it is started without a launcher (the driver's SCALE command shape
is `python bench.py --gpus N ...` as well as torch.distributed.run): CPU check of the spawn path with gloo."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gpus_2_spawns_two_ranks():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--spawn-check"], env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1  # one JSON line, from rank 0
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["world"] == 2


def test_bench_line_on_the_simt_mock(tmp_path):
    """The bench's own logic (device-side workload, contig stage once, steps over resident sub-batches, JSON contract)
    on the SIMT mock at a tiny scale; the numbers mean nothing here."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from sim import simlib
    lib = simlib.build()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--lib", lib, "--workload", "C2", "--scale", "0.0004",
                        "--steps", "1", "--warmup", "1", "--full", "--no-e2e", "--batch-bases", "100000"],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    out = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert out["config"]["workload"].startswith("C2:") and "2 distinct HBM-resident sub-batches" in out["config"]["workload"]
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "scaling", "dtype", "roofline", "cpu_baseline"):
        assert key in out
    assert out["n_gpus"] == 1 and out["cpu_baseline"]["kind"] == "port" and "stages_s" in out["cpu_baseline"]
    assert out["config"]["index_size"] > 0 and out["config"]["mappings_hits_pafs_per_step"][0] > 0
    # round 6: the roofline block says what binds, keeps the contract's HBM fields, and the line says that no scaling curve was measured
    roof = out["roofline"]
    assert roof["bound"] == "valu" and roof["unit"] == "GB/s" and roof["peak"] == 8000.0
    assert abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-4
    assert "scaling_note" in out and "No 1 -> 8 GPU curve" in out["scaling_note"]
    assert out["config"]["serial_pass"]["steps"] == 2  # --full: the kernels-alone pass behind the timed region


def test_plain_line_and_dumped_outputs_on_the_simt_mock(tmp_path):
    """A plain run does what the headline needs and nothing else (no kernels-alone pass, CPU baseline, end-to-end leg or other
    workloads); --steps is the number of timed steps; --dump-outputs writes the outputs of one more step of the same path as float
    arrays, whose counts are those of the line, and the same arrays from run to run."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from sim import simlib
    import numpy as np
    lib = simlib.build()
    lines = []
    for run in ("a", "b"):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--lib", lib, "--workload", "C2", "--scale", "0.0004",
                            "--steps", "2", "--warmup", "1", "--batch-bases", "100000", "--dump-outputs", str(tmp_path / run)],
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
        assert p.returncode == 0, p.stderr[-2000:]
        lines.append(json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]))
    out = lines[0]
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in out
    assert out["steps"] == 2 and abs(2 * out["ms_per_step"] - 1e3 * out["config"]["timed_region_s"]) < 2.0
    assert not {"cpu_baseline", "end_to_end", "other_workloads"} & set(out)
    assert "serial_pass" not in out["config"] and out["config"]["device_state_during_timed_steps"] is None
    got = {nm: np.load(tmp_path / "a" / f"{nm}.npy") for nm in ("counts", "maps", "hits", "pafs")}
    assert all(a.dtype == np.float64 for a in got.values()) and sum(a.nbytes for a in got.values()) <= 64 << 20
    counts = got["counts"]
    assert counts.shape == (out["sub_batches_per_rank"], 6)
    assert counts[:, 3:].sum(axis=0).tolist() == out["config"]["mappings_hits_pafs_per_step"]
    assert counts[:, 1].sum() == out["config"]["read_minimizers_per_step"]
    assert len(got["maps"]) > 0 and len(got["hits"]) == got["maps"][:, 2].sum()
    for nm, a in got.items():
        assert np.array_equal(a, np.load(tmp_path / "b" / f"{nm}.npy")), nm


def test_dumped_sample_follows_the_hit_offsets(monkeypatch):
    """OutputSampler: a sample of fewer reads than the step holds, reads numbered across the sub-batches; each sampled mapping with the
    hits its own hit_off / n_hits point to, in hit arrays whose per-read regions have gaps between them (as the device lays them out:
    read r's hits from its first minimizer on); the counts of every sub-batch."""
    sys.path.insert(0, ROOT)
    import bench
    import numpy as np
    from ntlink_amd.capi import MAPPING_DT, HIT_DT, PAF_DT
    monkeypatch.setattr(bench, "DUMP_READS", 4)
    sizes = (6, 5)
    sampler = bench.OutputSampler(sizes)
    assert len(sampler.pick) == 4 and len(set(sampler.pick.tolist())) == 4 and sampler.pick.max() < sum(sizes)
    want_maps, want_hits = [], []
    for b, reads in enumerate(sizes):
        base = sum(sizes[:b])
        rows = [(r, c) for r in range(reads) for c in range(1 + r % 2)]  # odd reads map to two contigs
        maps = np.zeros(len(rows), MAPPING_DT)
        maps["read"] = [r for r, _ in rows]
        maps["ctg"] = [10 * b + c for _, c in rows]
        maps["n_hits"] = [1 + (r + c) % 3 for r, c in rows]
        maps["hit_off"] = [16 * r + 4 * c + 1 for r, c in rows]  # gaps before, between and after the regions
        hits = np.zeros(16 * reads, HIT_DT)
        hits["ctg_pos"] = 99_999_999  # what no sampled mapping may carry
        for m in maps:
            o, n = int(m["hit_off"]), int(m["n_hits"])
            hits["ctg_pos"][o:o + n] = 1000 * b + 100 * int(m["read"]) + 10 * int(m["ctg"]) + np.arange(n)
            hits["read_pos"][o:o + n] = int(m["read"])
            hits["read_strand"][o:o + n] = 1
        pafs = np.zeros(len(rows), PAF_DT)
        pafs["read"], pafs["ctg"], pafs["q_end"] = maps["read"], maps["ctg"], 4_000_000_000
        sampler.count(b, 11 * reads, 5 * reads, (len(maps), len(hits), len(pafs)))
        sampler.take(b, {"maps": maps, "hits": hits, "pafs": pafs})
        for m in maps:
            if base + int(m["read"]) in sampler.pick:
                want_maps.append([base + int(m["read"]), int(m["ctg"]), int(m["n_hits"])])
                for hh in hits[int(m["hit_off"]):int(m["hit_off"]) + int(m["n_hits"])]:
                    want_hits.append([base + int(m["read"]), int(m["ctg"]), int(hh["ctg_pos"]), int(hh["read_pos"]), 0, 1])
    out = sampler.arrays()
    assert out["counts"].tolist() == [[6, 66, 30, 9, 96, 9], [5, 55, 25, 7, 80, 7]]
    assert sorted(set(out["maps"][:, 0].tolist())) == sorted(sampler.pick.tolist())
    assert out["maps"].tolist() == want_maps and out["hits"].tolist() == want_hits
    assert 99_999_999 not in out["hits"][:, 2] and len(out["hits"]) == out["maps"][:, 2].sum()
    assert out["pafs"][:, 0].tolist() == [x[0] for x in want_maps] and set(out["pafs"][:, 3].tolist()) == {4e9}  # u32 exact in float64


def test_dump_step_downloads_only_after_the_step(monkeypatch):
    """OutputSampler as the dump step's sink: inside the step it asks only for counts (a download drains the main stream and would
    serialise the sub-batches) and keeps the results of DUMP_BATCHES sub-batches spread over the step open -- the first and the last
    among them; the others are closed at once.  finish() downloads the held ones after the step and closes them; the sample is drawn
    from the held sub-batches' reads."""
    sys.path.insert(0, ROOT)
    import bench
    import numpy as np
    from ntlink_amd.capi import MAPPING_DT, HIT_DT, PAF_DT
    monkeypatch.setattr(bench, "DUMP_BATCHES", 4)
    log = []

    class Sketch:
        count = 40

    class Result:
        def __init__(self, j):
            self.j = j
        n_index_hits = 9

        def counts(self):
            log.append(("counts", self.j))
            return (2, 3, 2)

        def download(self):
            log.append(("download", self.j))
            maps = np.zeros(2, MAPPING_DT)
            maps["read"], maps["n_hits"], maps["hit_off"] = [0, 1], [1, 2], [0, 1]
            return {"maps": maps, "hits": np.zeros(3, HIT_DT), "pafs": np.zeros(0, PAF_DT)}

        def close(self):
            log.append(("close", self.j))

    sampler = bench.OutputSampler([2] * 10)
    assert sampler.held == [0, 3, 6, 9]
    assert set((sampler.pick // 2).tolist()) <= set(sampler.held) and len(sampler.pick) == 8
    for j in range(10):
        res = Result(j)
        if not sampler.add(j, Sketch(), res):
            res.close()
    assert not [e for e in log if e[0] == "download"] and sorted(sampler.open) == [0, 3, 6, 9]
    assert [e[1] for e in log if e[0] == "close"] == [1, 2, 4, 5, 7, 8]
    log.clear()
    sampler.finish()
    assert log == [(what, j) for j in (0, 3, 6, 9) for what in ("download", "close")] and not sampler.open
    out = sampler.arrays()
    assert out["counts"].tolist() == [[2, 40, 9, 2, 3, 2]] * 10
    assert out["maps"][:, 0].tolist() == [0, 1, 6, 7, 12, 13, 18, 19] and len(out["hits"]) == 12


def test_valu_roofline_fraction_is_priced_on_the_floor(monkeypatch):
    """roofline.valu.frac = the floor's instructions at their calibrated issue cost / the SIMD cycles of the launch -- it must fall when
    the kernel issues more instructions for the same bases, which the kernel's own mix priced against its own cycles
    (issue_slots_filled) cannot show."""
    sys.path.insert(0, ROOT)
    import bench
    floor = sum(n * bench.valu_class_cycles(c) for c, n in bench.VALU_FLOOR_CLASSES)
    assert 27.0 < floor < 31.0 and sum(n for _, n in bench.VALU_FLOOR_CLASSES) == bench.VALU_FLOOR_PER_KMER
    monkeypatch.setattr(bench, "priced_cycles", lambda pm, n: {"cycles": 3.3, "how": "test"})
    bases = 3_900_000_000
    lean = bench.valu_roofline({"valu_wave_instr_per_launch": 1.2e9, "measured_cycles_per_wave_instr": 3.3, "clock_ghz": 2.1}, 1.8, bases)
    fat = bench.valu_roofline({"valu_wave_instr_per_launch": 2.4e9, "measured_cycles_per_wave_instr": 3.3, "clock_ghz": 2.1}, 3.6, bases)
    assert abs(lean["frac"] - floor * (bases / 64) / (3.3 * 1.2e9)) < 1e-3
    assert abs(fat["frac"] - lean["frac"] / 2) < 1e-3                      # twice the instructions for the same bases: half the fraction
    assert lean["issue_slots_filled"] == fat["issue_slots_filled"] == 1.0  # ... which the self-priced figure does not see
    assert abs(lean["useful_frac"] - 9.0 / (1.2e9 * 64 / bases)) < 1e-3


def test_device_state_poller_reads_the_busiest_card(tmp_path, monkeypatch):
    """config.device_state_during_timed_steps: shader clock / socket power / junction temperature from the amdgpu hwmon files while the
    timed steps run (the step follows the clock, and the boxes differ in the clock they sustain).  No hwmon: no field, never an error;
    no PCI address from the runtime: the card that draws the most power."""
    import glob
    import time
    sys.path.insert(0, ROOT)
    import bench
    with bench.DeviceStatePoller(0) as p:
        pass
    assert p.summary() is None or "sclk_mhz" in p.summary()  # (None here: no amdgpu hwmon in the CPU container)
    dirs = []
    for i, (mhz, watt) in enumerate(((2400, 290), (2130, 1190))):
        d = tmp_path / f"card{i}" / "device" / "hwmon" / "hwmon0"
        d.mkdir(parents=True)
        for name, v in (("freq1_label", "sclk"), ("freq1_input", mhz * 10**6), ("power1_input", watt * 10**6), ("temp2_input", 58000), ("power1_cap", 1400 * 10**6)):
            (d / name).write_text(f"{v}\n")
        dirs.append(str(d))
    monkeypatch.setattr(glob, "glob", lambda pat: dirs)
    with bench.DeviceStatePoller(0, period=0.01) as p:
        time.sleep(0.08)
    st = p.summary()
    assert st["samples"] >= 2 and st["source"] == dirs[1] and "most power" in st["picked"]
    assert st["sclk_mhz"]["median"] == 2130.0 and st["socket_power_w"]["max"] == 1190.0 and st["junction_c"]["min"] == 58.0 and st["power_cap_w"] == 1400.0


def test_two_ranks_strong_scaling_line_on_the_simt_mock():
    """`bench.py --gpus 2` (strong scaling is the default for N > 1: BASELINE.json configs[3]) end to end on CPU: the launcher starts two gloo ranks, each maps its half of the read
    set on the SIMT mock, rank 0 prints one line with n_gpus = 2, the max-over-ranks time and the summed bases."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from sim import simlib
    lib = simlib.build()
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    base = [sys.executable, os.path.join(ROOT, "bench.py"), "--lib", lib, "--workload", "C2", "--scale", "0.0004", "--steps", "1",
            "--warmup", "1", "--full", "--no-e2e", "--no-cpu-baseline", "--batch-bases", "100000"]
    p = subprocess.run(base + ["--gpus", "2", "--min-batches", "2"], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)  # bare --gpus N = configs[3]
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    two = json.loads(lines[0])
    assert two["n_gpus"] == 2 and two["scaling"] == "strong"
    assert two["world_size"] == 2 and two["rccl_ranks_seen"] == 2
    assert [(r["rank"], r["local_rank"], r["backend"]) for r in two["ranks"]] == [(0, 0, "gloo"), (1, 1, "gloo")] and all(r["device"] for r in two["ranks"])
    per_rank = int(two["config"]["workload"].split(" read bases per GPU")[0].split("+ ")[-1])
    assert abs(2 * per_rank - 200_000) < 40_000  # C2 at scale 0.0004 is 200 kbases of reads: split two ways (a few 10-kb reads each)
    assert two["ms_per_step"] > 0 and two["config"]["index_size"] > 0 and two["config"]["mappings_hits_pafs_per_step"][0] > 0
    assert two["config"]["serial_pass"]["steps"] == 2  # --full: the kernels-alone pass and its barriers at world 2


def test_eight_ranks_strong_scaling_line_on_the_simt_mock():
    """configs[3]'s shape: a bare `bench.py --gpus 8` -- eight gloo ranks, each with an eighth of the read set; the line
    carries every rank's time and bases so that an imbalance would show."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from sim import simlib
    lib = simlib.build()
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--lib", lib, "--workload", "C2", "--scale", "0.0008", "--steps", "1",
                        "--warmup", "1", "--no-e2e", "--no-cpu-baseline", "--batch-bases", "100000", "--serial-steps", "0", "--gpus", "8", "--min-batches", "4"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=1500)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["n_gpus"] == 8 and out["scaling"] == "strong" and out["world_size"] == 8 and out["rccl_ranks_seen"] == 8
    assert [r["local_rank"] for r in out["ranks"]] == list(range(8))
    assert out["sub_batches_per_rank"] >= 4  # a rank's share is cut into sub-batches of its own (--min-batches), not the N = 1 size
    assert len(out["per_rank_ms_per_step"]) == 8 and len(out["per_rank_bases_per_step"]) == 8
    # C2 at scale 0.0008: 400 kbases of reads over all ranks; a sub-batch of 12.5 kbases is rounded up to two whole 10-kb reads
    assert 400_000 <= sum(out["per_rank_bases_per_step"]) <= 700_000
    assert max(out["per_rank_ms_per_step"]) == pytest_approx(out["ms_per_step"])


def pytest_approx(v):
    import pytest
    return pytest.approx(v, rel=1e-3, abs=1e-3)
