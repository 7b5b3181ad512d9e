"""The gap filler's output: gapfill.output_plan / print_gap_filled_sequences / print_agp / print_filling_stats / patch_gaps and
bin/ntlink_patch_gaps.py -- under the SIMT mock and on the GPU, the same checks.
  a. crafted: FASTA, AGP and summary against what the reference's own print_gap_filled_sequences, print_agp and print_filling_stats
     wrote for the same pairs, scaffolds and reads (tests/golden/gen/gapout_cases.json.gz, made by tests/golden/gen_goldens_gapout.py,
     which asserts what the case contains), without and with --soft_mask, with the default max_bytes and with one so small that every
     path line is a stitch call of its own and one exceeds it
  b. shipped: patch_gaps with the arguments of the reference's test_5 writes the FASTA the reference ships
     (tests/golden/ref/expected_outputs/...gap_fill.fa), the three AGP rows and the summary of the reference's main(); the same with the
     reads in two files (test_8) and with --soft_mask; on the GPU bin/ntlink_patch_gaps.py as a child process, and no temporary file
  c. PairInfo.chosen_reversed of choose_gap_reads == what choose_gap_reads_restated sets, for every pair of the gap-select fixtures"""
import argparse
import contextlib
import functools
import glob
import gzip
import io
import json
import os
import subprocess
import sys

import pytest

from ntlink_amd import capi, gapfill

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.path.join(HERE, "golden", "ref")
PREFIX = os.path.join(REF, "expected_outputs", "scaffolds_1.fa.k32.w250.z1000.")
READ_ID = "42601c42-926c-46c1-a103-f84988cb196e_Basecall_1D_template"
AGP_ROWS = ["ntLink_0\t1\t33470\t1\tW\t188266\t1\t33470\t+", f"ntLink_0\t33471\t39162\t2\tP\t{READ_ID}\t6398\t12089\t+",
            "ntLink_0\t39163\t87420\t3\tW\t189231\t1\t48258\t-"]


@functools.lru_cache(maxsize=None)
def golden():
    with gzip.open(os.path.join(HERE, "golden", "gen", "gapout_cases.json.gz"), "rt") as fh:
        return json.load(fh)


@functools.lru_cache(maxsize=None)
def shipped_fasta():
    with open(PREFIX + "ntLink.scaffolds.gap_fill.fa", "rb") as fh:
        return fh.read()


# ---------------------------------------------------------------- a. crafted

def check_crafted(dev, tmp_path, max_bytes):
    doc = golden()
    path = str(tmp_path / "c.path")
    with open(path, "w") as fh:
        fh.write(doc["path"])
    with gapfill.resident_scaffolds(doc["scaffolds"], dev=dev, stitchable=True) as scaffolds, \
            gapfill._resident(dev, [r[0] for r in doc["reads"]], [r[1].encode() for r in doc["reads"]], False, True) as reads:
        for which, soft in (("plain", False), ("soft_mask", True)):
            pairs = {}
            for source, target, gap, read, sc, sr, tc, tr, old, reversed_ in doc["pairs"]:
                p = pairs[(source, target)] = gapfill.PairInfo(gap)
                p.chosen_read, p.source_ctg_cut, p.source_read_cut, p.target_ctg_cut, p.target_read_cut = read, sc, sr, tc, tr
                p.old_anchor_used, p.chosen_reversed = old, reversed_ if read is not None else None
            sequences = {name: gapfill.ScaffoldGaps(length=len(seq)) for name, seq in doc["scaffolds"]}
            for name, (c5, c3, t5, t3) in doc["state"].items():
                s = sequences[name]
                s.five_prime_cut, s.three_prime_cut, s.five_prime_trim, s.three_prime_trim = c5, c3, t5, t3
            args = argparse.Namespace(o=str(tmp_path / f"{which}.{max_bytes}.fa"), path=path, min_gap=doc["min_gap"], soft_mask=soft)
            stats = io.StringIO()
            plan = gapfill.print_gap_filled_sequences(pairs, sequences, scaffolds, reads, args, dev=dev, max_bytes=max_bytes, stats_file=stats)
            gapfill.print_agp(pairs, sequences, args, plan=plan)
            want = doc[which]
            with open(args.o, "rb") as fh:
                got = fh.read().decode()
            assert got.split("\n") == want["fasta"].split("\n"), which
            with open(args.o + ".agp") as fh:
                assert fh.read().split("\n") == want["agp"].split("\n"), which
            assert stats.getvalue() == want["stats"]
            assert plan.printed == set("ABCDEFGHIJKLMNOPQ") and plan.unassigned == ["U1", "U2"]
            sizes = [size for _h, _s, size in gapfill._record_segments(plan, sequences, scaffolds, reads)]
            if max_bytes < gapfill.STITCH_BYTES:  # every record a call of its own, and one larger than the bound
                assert min(a + b for a, b in zip(sizes, sizes[1:])) > max_bytes and max(sizes) > max_bytes > min(sizes)
                assert len(list(gapfill._stitch_calls(gapfill._record_segments(plan, sequences, scaffolds, reads), max_bytes))) == len(sizes)
            else:
                assert len(list(gapfill._stitch_calls(gapfill._record_segments(plan, sequences, scaffolds, reads), max_bytes))) == 1
    dev.sync()


# ---------------------------------------------------------------- b. the reference's shipped golden

def _args(tmp_path, name, reads, **kw):
    a = argparse.Namespace(path=PREFIX + "trimmed_scafs.path", mappings=PREFIX + "verbose_mapping.tsv", trims=PREFIX + "trimmed_scafs.tsv",
                           s=os.path.join(REF, "scaffolds_1.fa"), reads=reads, z=1000, k=35, w=10, t=4, large_k=32, x=0, min_gap=1,
                           o=str(tmp_path / name), stringent=False, soft_mask=False, sensitive=False, verbose=False)
    vars(a).update(kw)
    return a


def _split_reads(tmp_path):
    """long_reads_1.fa in two files, cut between two records (the reference's test_8)"""
    with open(os.path.join(REF, "long_reads_1.fa"), "rb") as fh:
        raw = fh.read()
    cut = raw.index(b"\n>", len(raw) // 2) + 1
    parts = [str(tmp_path / "reads_a.fa"), str(tmp_path / "reads_b.fa")]
    for p, piece in zip(parts, (raw[:cut], raw[cut:])):
        with open(p, "wb") as fh:
            fh.write(piece)
    assert raw[cut:cut + 1] == b">" and cut < len(raw)
    return parts


def soft_masked(fasta):
    """the shipped golden with output bases [33470, 39162) of ntLink_0 lower-cased, nothing else changed"""
    head, _, rest = fasta.partition(b"\n")
    assert head == b">ntLink_0"
    return head + b"\n" + rest[:33470] + rest[33470:39162].lower() + rest[39162:]


def check_shipped(dev, tmp_path, variant):
    reads = _split_reads(tmp_path) if variant == "two_files" else [os.path.join(REF, "long_reads_1.fa")]
    args = _args(tmp_path, variant + ".gap_fill.fa", reads, soft_mask=variant == "soft_mask")
    log = io.StringIO()
    with contextlib.redirect_stdout(log):
        pairs, _sequences, plan = gapfill.patch_gaps(args, dev)
    assert args.min_gap == 1, "the caller's namespace is left alone"
    with open(args.o, "rb") as fh:
        got = fh.read()
    want = soft_masked(shipped_fasta()) if variant == "soft_mask" else shipped_fasta()
    assert len(got) == len(want) and got == want, "the reference's shipped .gap_fill.fa"
    assert want != shipped_fasta() or variant != "soft_mask"
    with open(args.o + ".agp") as fh:
        agp = fh.read()
    assert agp == golden()["shipped"]["agp"] and agp.splitlines() == AGP_ROWS
    assert [plan.counters[c] for c in gapfill._COUNTERS] == [1, 0, 0, 1, 1, 1, 0]
    assert golden()["shipped"]["stats"] in log.getvalue() and "DONE!" in log.getvalue()
    assert [p.chosen_read for p in pairs.values()] == [READ_ID]
    assert not glob.glob(str(tmp_path / "*masked_temp*"))
    dev.sync()


# ---------------------------------------------------------------- c. chosen_reversed

def check_chosen_reversed(dev, tmp_path):
    import types
    with gzip.open(os.path.join(HERE, "golden", "gen", "gapsel_cases.json.gz"), "rt") as fh:
        doc = json.load(fh)
    vp, pp = str(tmp_path / "g.verbose_mapping.tsv"), str(tmp_path / "g.path")
    for p, text in ((vp, doc["verbose"]), (pp, doc["path"])):
        with open(p, "w") as fh:
            fh.write(text)
    sequences = {name: types.SimpleNamespace(length=length) for name, length in doc["lengths"].items()}
    args = argparse.Namespace(large_k=doc["large_k"])
    mine, theirs = gapfill.read_path_file_pairs(pp, doc["min_gap"]), gapfill.read_path_file_pairs(pp, doc["min_gap"])
    gapfill.choose_gap_reads(mine, vp, sequences, args, dev=dev)
    gapfill.choose_gap_reads_restated(theirs, vp, sequences, args)
    got = {key: (p.chosen_read, p.chosen_reversed) for key, p in mine.items()}
    assert got == {key: (p.chosen_read, p.chosen_reversed) for key, p in theirs.items()}
    flags = {rev for read, rev in got.values() if read is not None}
    assert flags == {True, False} and all(rev is None for read, rev in got.values() if read is None)
    dev.sync()


# ---------------------------------------------------------------- under the SIMT mock

@pytest.fixture(scope="module")
def sim_dev():
    from sim import simlib
    dev = simlib.device()
    yield dev
    dev.close()


@pytest.mark.parametrize("max_bytes", [gapfill.STITCH_BYTES, 140])
def test_sim_crafted(sim_dev, tmp_path, max_bytes):
    check_crafted(sim_dev, tmp_path, max_bytes)


@pytest.mark.parametrize("variant", ["one_file", "two_files", "soft_mask"])
def test_sim_shipped(sim_dev, tmp_path, variant):
    check_shipped(sim_dev, tmp_path, variant)


def test_sim_chosen_reversed(sim_dev, tmp_path):
    check_chosen_reversed(sim_dev, tmp_path)


# ---------------------------------------------------------------- on the GPU

@pytest.fixture(scope="module")
def gpu_dev():
    dev = capi.Device(0)
    yield dev
    dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("max_bytes", [gapfill.STITCH_BYTES, 140])
def test_gpu_crafted(gpu_dev, tmp_path, max_bytes):
    check_crafted(gpu_dev, tmp_path, max_bytes)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["one_file", "two_files", "soft_mask"])
def test_gpu_shipped(gpu_dev, tmp_path, variant):
    check_shipped(gpu_dev, tmp_path, variant)


@pytest.mark.gpu
def test_gpu_chosen_reversed(gpu_dev, tmp_path):
    check_chosen_reversed(gpu_dev, tmp_path)


@pytest.mark.gpu
def test_gpu_command(tmp_path):
    """bin/ntlink_patch_gaps.py as a child process: the shipped FASTA, the parameter block, and no temporary file left behind"""
    out = str(tmp_path / "cli.gap_fill.fa")
    cmd = [sys.executable, os.path.join(os.path.dirname(HERE), "bin", "ntlink_patch_gaps.py"), "--path", PREFIX + "trimmed_scafs.path",
           "--mappings", PREFIX + "verbose_mapping.tsv", "--trims", PREFIX + "trimmed_scafs.tsv", "-s", os.path.join(REF, "scaffolds_1.fa"),
           "--reads", os.path.join(REF, "long_reads_1.fa"), "--large_k", "32", "--min_gap", "1", "-k", "35", "-w", "10", "-t", "2", "-o", out]
    done = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stderr[-2000:]
    with open(out, "rb") as fh:
        assert fh.read() == shipped_fasta()
    with open(out + ".agp") as fh:
        assert fh.read().splitlines() == AGP_ROWS
    assert done.stdout.startswith("Running ntLink gap-filling...\n\nParameters:\n\t--path ") and "\t--min_gap 1\n" in done.stdout
    assert golden()["shipped"]["stats"] in done.stdout
    assert sorted(os.listdir(tmp_path)) == ["cli.gap_fill.fa", "cli.gap_fill.fa.agp"] and not glob.glob(str(tmp_path / "*.masked_temp.fa"))
