"""The overlap stage behind the filter (ntlink_amd.overlap: merge_overlapping_pathfile, the four writers, overlap_sequences) and its
drop-in CLI (bin/ntlink_overlap_sequences.py) -- under the SIMT mock and on the GPU, the same checks.
  a. the reference's four fixtures (tests/golden/ref: <target>.stitch.path, .n1.scaffold.dot -> .trimmed_scafs.{path,tsv,agp,fa} as the
     reference's own run left them; only fixture 4 has real overlaps), fused form; fixture 4 also through the CLI as a child process
  b. the fused form and the `-m FILE` form against each other: fixture 4 with a whole-file k15 w5 TSV made by this project's indexlr
  c. the cases of tests/golden/gen_goldens_overlapcuts.py against the end state the reference left (every ScaffoldCut, the new paths,
     the four files), through the recorded minimizer stream with its LAST marker lines and through the fused form
  d. the refusals, each a ValueError that names the pair; the assertions of ScaffoldCut; the lone N of an empty slice
  e. no output file is left after a failure"""
import argparse
import functools
import gzip
import json
import os
import subprocess
import sys

import pytest

from ntlink_amd import capi, gapfill, overlap, pipeline

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.path.join(HERE, "golden", "ref")
FIXTURES = {1: "scaffolds_1.fa.k32.w250.z1000", 2: "scaffolds_2.fa.k32.w100.z1000", 3: "scaffolds_3.fa.k24.w250.z1000", 4: "scaffolds_4.fa.k40.w100.z1000"}
SUFFIXES = ("path", "tsv", "agp", "fa")


def fixture_args(n, prefix, m=None):
    base = os.path.join(REF, "expected_outputs", FIXTURES[n])
    return argparse.Namespace(m=m, f=0.5, path=base + ".stitch.path", fasta=os.path.join(REF, f"scaffolds_{n}.fa"), k=15, d=base + ".n1.scaffold.dot",
                              g=20, outgap=0, p=prefix, v=False, trim_info=True)  # ntLink:246-251 with its defaults (merge_gap=0)


def texts(prefix):
    return {s: open(f"{prefix}.trimmed_scafs.{s}", "rb").read() for s in SUFFIXES}


def expected_fixture(n):
    """the reference's four files; its .trimmed_scafs.fa is kept gzip-compressed among the fixtures, the same bytes"""
    base = os.path.join(REF, "expected_outputs", FIXTURES[n]) + ".trimmed_scafs."
    return {s: (gzip.open(base + "fa.gz") if s == "fa" else open(base + s, "rb")).read() for s in SUFFIXES}


# ---------------------------------------------------------------- a, b. fixtures

def check_fixture(dev, tmp_path, n):
    prefix = str(tmp_path / "out")
    scaffolds, _paths = overlap.overlap_sequences(fixture_args(n, prefix), dev)
    got, want = texts(prefix), expected_fixture(n)
    for s in SUFFIXES:
        assert got[s] == want[s], f"fixture {n}: .trimmed_scafs.{s} differs"
    if n == 4:  # scaf3- 1N scaf4+ and scaf1+ 1N scaf2+, trims 57 / 40 / 46
        assert b"scaf3- 1N scaf4+" in got["path"] and got["tsv"] == b"scaf1\t0\t8913\nscaf2\t46\t30523\nscaf3\t57\t15069\nscaf4\t40\t8463\n"
        assert scaffolds["scaf3"].ori == "-" and scaffolds["scaf3"].source_cut == 57 - 15
    dev.sync()


def check_tsv_form(dev, tmp_path):
    tsv = str(tmp_path / "k15w5.tsv")
    with open(tsv, "w") as fh:
        pipeline.run_indexlr(dev, [os.path.join(REF, "scaffolds_4.fa")], 15, overlap.OVERLAP_W, fh, False, with_strand=False)
    prefix = str(tmp_path / "viatsv")
    overlap.overlap_sequences(fixture_args(4, prefix, m=tsv), dev)
    assert texts(prefix) == expected_fixture(4)
    dev.sync()


def check_cli(tmp_path, env):
    a = fixture_args(4, str(tmp_path / "cli"))
    cmd = [sys.executable, os.path.join(ROOT, "bin", "ntlink_overlap_sequences.py"), "-a", a.path, "-s", a.fasta, "-d", a.d, "-k", "15", "-g", "20",
           "--outgap", "0", "-p", a.p, "--trim_info"]
    done = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr
    assert "Parameters for overlap stage:" in done.stdout and "DONE!" in done.stdout
    assert texts(a.p) == expected_fixture(4)
    # -v is refused; a missing dot file fails: both exit non-zero and leave nothing
    for extra, prefix in ((["-v"], "verbose"), (["-d", str(tmp_path / "missing.dot")], "nodot")):
        bad = subprocess.run(cmd[:-3] + ["-p", str(tmp_path / prefix)] + extra, env=env, capture_output=True, text=True, timeout=300)
        assert bad.returncode != 0 and "ERROR" in bad.stderr, (bad.returncode, bad.stderr)
        assert not [f for f in os.listdir(tmp_path) if f.startswith(prefix)]


# ---------------------------------------------------------------- c. the generator's cases

@functools.lru_cache(maxsize=None)
def golden():
    with gzip.open(os.path.join(HERE, "golden", "gen", "overlapcut_cases.json.gz"), "rt") as fh:
        doc = json.load(fh)
    assert [c["name"] for c in doc["cases"]] == ["g20-outgap0", "g20-outgap2", "g4-f1"]
    return doc["cases"]


def golden_inputs(case, tmp_path, with_tsv):
    files = {}
    for key in ("fasta", "path", "dot") + (("tsv",) if with_tsv else ()):
        files[key] = str(tmp_path / f"in.{key}")
        with open(files[key], "w") as fh:
            fh.write(case[key])
    a = case["args"]
    return argparse.Namespace(m=files.get("tsv"), f=a["f"], path=files["path"], fasta=files["fasta"], k=a["k"], d=files["dot"], g=a["g"], outgap=a["outgap"],
                              p=str(tmp_path / ("tsv" if with_tsv else "fused")), v=False, trim_info=True)


def check_golden(dev, tmp_path, i, with_tsv):
    case = golden()[i]
    args = golden_inputs(case, tmp_path, with_tsv)
    scaffolds, paths = overlap.overlap_sequences(args, dev)
    got = {n: [s.ori, s.source_cut, s.target_cut, s.is_omitted_sequence()] for n, s in scaffolds.items()}
    assert list(got) == list(case["scaffolds"])  # FASTA order
    for name, want in case["scaffolds"].items():
        assert got[name] == want, f"{case['name']}: {name} ends as {got[name]}, the reference leaves {want}"
    assert paths == case["paths"]
    for s, text in texts(args.p).items():
        assert text.decode() == case["files"][s], f"{case['name']}: .trimmed_scafs.{s} differs"
    dev.sync()


def test_valid_regions_and_readers(tmp_path):
    """find_valid_mx_regions and the readers in front of it: no device"""
    case = golden()[0]
    args = golden_inputs(case, tmp_path, False)
    graph, scaf_num = overlap.read_scaffold_graph(args.d)
    assert scaf_num == 7 and overlap.has_estimated_overlap(graph, "zeta+", "mid-") and not overlap.has_estimated_overlap(graph, "b4+", "b5+")
    assert not overlap.has_estimated_overlap(graph, "b5+", "b6+") and not overlap.has_estimated_overlap(graph, "nobody+", "b6+")
    lines = case["fasta"].split("\n")
    scaffolds = {header.split()[0][1:]: overlap.ScaffoldCut(header.split()[0][1:], seq) for header, seq in zip(lines[0::2], lines[1::2])}
    valid = overlap.find_valid_mx_regions(args, overlap.GAP_RE, graph, scaffolds)
    assert {n: [list(r) for r in regs] for n, regs in valid.items()} == case["valid"]
    assert any(r[0] < 0 for regs in case["valid"].values() for r in regs), "a negative start, as the reference leaves it"
    assert overlap.normalize_path(["b+", "3N", "a-"], overlap.GAP_RE) == ["a+", "3N", "b-"]
    assert overlap.normalize_path(["a+", "3N", "b-"], overlap.GAP_RE) == ["a+", "3N", "b-"]


# ---------------------------------------------------------------- d, e. refusals, assertions, nothing left behind

def check_refusals(dev, tmp_path):
    case = golden()[0]

    def failing(change, match, exc=ValueError):
        sub = tmp_path / f"r{len(os.listdir(tmp_path))}"
        sub.mkdir()
        doc = dict(case)
        change(doc)
        args = golden_inputs(doc, sub, False)
        with pytest.raises(exc, match=match):
            overlap.overlap_sequences(args, dev)
        assert sorted(os.listdir(sub)) == ["in.dot", "in.fasta", "in.path"], "no output is left after a failure"

    def same_contig(doc):
        doc["path"] += "ntLink_9\tb4+ 21N b4-\n"
        doc["dot"] = doc["dot"].replace("}\n", '"b4+" -> "b4-" [d=-50 e=1 n=1]\n}\n')
    failing(same_contig, r"pair b4\+ b4-: source and target are the same contig")

    def absent(doc):
        doc["path"] += "ntLink_9\tb4+ 21N ghost+\n"
        doc["dot"] = doc["dot"].replace("}\n", '"b4+" -> "ghost+" [d=-50 e=1 n=1]\n}\n')
    failing(absent, r"pair b4\+ ghost\+: contig ghost is not in the FASTA file")

    def too_far(doc):
        doc["path"] += "ntLink_9\tb4- 21N b6+\n"
        doc["dot"] = doc["dot"].replace("}\n", '"b4-" -> "b6+" [d=-4000000000 e=1 n=1]\n}\n')
    failing(too_far, r"pair b4- b6\+: .* does not fit 32 bits")

    def cut_twice(doc):  # b2 is the target of b1- already: the reference's assertion, where the reference raises it
        doc["path"] += "ntLink_9\tb1- 21N b2+\n"
    failing(cut_twice, "Source cut is already set", AssertionError)

    def other_sign(doc):  # zeta is '-' in the first path (reversed by normalize_path); this one is kept as it is
        doc["path"] += "ntLink_9\talpha+ 300N zeta+ 21N mid-\n"
    failing(other_sign, "Ori is already set", AssertionError)

    def bad_dot(doc):
        doc["dot"] = doc["dot"].replace("}\n", "what is this\n}\n")
    failing(bad_dot, "unexpected line")

    # the TSV form: a contig of a pair without a line in the minimizer file
    sub = tmp_path / "notsv"
    sub.mkdir()
    doc = dict(case)
    doc["tsv"] = "".join(line + "\n" for line in case["tsv"].split("\n") if line and not line.startswith("b2\t"))
    with pytest.raises(ValueError, match=r"pair b1- b2\+: contig b2 has no line in the minimizer file"):
        overlap.overlap_sequences(golden_inputs(doc, sub, True), dev)
    assert sorted(os.listdir(sub)) == ["in.dot", "in.fasta", "in.path", "in.tsv"]
    with pytest.raises(ValueError, match="-v"):
        args = golden_inputs(case, sub, True)
        args.v = True
        overlap.overlap_sequences(args, dev)
    dev.sync()


def test_scaffold_cut():
    s = overlap.ScaffoldCut("c", "ACGTACGTAC")
    assert (s.ori, s.source_cut, s.target_cut, s.get_trim_coordinates(3), s.check_valid_trims(3)) == (None, None, None, (0, 10), True)
    s.ori = "+"
    assert (s.source_cut, s.target_cut) == (10, 0)
    s.ori = "+"
    with pytest.raises(AssertionError, match="Ori is already set"):
        s.ori = "-"
    with pytest.raises(ValueError, match="Orientation must be"):
        overlap.ScaffoldCut("d", "ACGT").ori = "?"
    s.source_cut = 7
    with pytest.raises(AssertionError, match="Source cut is already set"):
        s.source_cut = 8
    s.target_cut = 2
    with pytest.raises(AssertionError, match="Target cut is already set"):
        s.target_cut = 3
    assert s.get_trim_coordinates(3) == (2, 7) and s.check_valid_trims(3) and str(s) == "c+ 10 - s:7 t:2"
    m = overlap.ScaffoldCut("m", length=10)
    m.ori = "-"
    assert (m.source_cut, m.target_cut, m.get_trim_coordinates(3)) == (0, 10, (0, 10))
    m.source_cut = 4
    assert m.get_trim_coordinates(3) == (7, 10) and m.adjust_target_cut(3) == 10  # + k only for a cut that was set
    m.target_cut = 5
    assert m.get_trim_coordinates(3) == (7, 8) and m.check_valid_trims(3)
    m2 = overlap.ScaffoldCut("m2", length=10)
    m2.ori = "-"
    m2.source_cut, m2.target_cut = 6, 3
    assert not m2.check_valid_trims(3) and not m2.is_omitted_sequence()
    m2.omit_sequence()
    assert m2.is_omitted_sequence()


def check_writers(dev, tmp_path):
    """the lone N of an empty slice, `None-None`, omitted sequences left out of all three, 1N rows and the component numbers"""
    records = [("a", "ACGTACGTAC"), ("b", "GGGGGCCCCC"), ("c", "TTTTT"), ("gone", "AAAA"), ("e", "ACACACAC")]
    scaffolds = {name: overlap.ScaffoldCut(name, seq) for name, seq in records}
    scaffolds["a"].ori = "+"
    scaffolds["a"].source_cut = 6
    scaffolds["b"].ori = "-"
    scaffolds["b"].target_cut = 3
    scaffolds["b"].source_cut = 0    # a '-' node cut at 0 + k = 3 .. 3 + k = 6
    scaffolds["e"].ori = "+"
    scaffolds["e"].target_cut = 8    # nothing left of it: 8 .. 8
    scaffolds["gone"].omit_sequence()
    args = argparse.Namespace(p=str(tmp_path / "w"), k=3, fasta=None)
    with gapfill.resident_scaffolds(records, dev=dev, stitchable=True) as resident:
        overlap.print_trimmed_scaffolds(args, scaffolds, resident=resident, dev=dev)
    overlap.print_trim_coordinates(args, scaffolds)
    overlap.print_agp_file({"p1": ["a+", "1N", "b-", "4N", "e+"]}, scaffolds, args)
    got = {s: open(f"{args.p}.trimmed_scafs.{s}").read() for s in ("tsv", "agp", "fa")}
    assert got["fa"] == ">a 6-0\nACGTAC\n>b 0-3\nGGC\n>c None-None\nTTTTT\n>e 8-8\nN\n"
    assert got["tsv"] == "a\t0\t6\nb\t3\t6\nc\t0\t5\ne\t8\t8\n"
    assert got["agp"] == ("p1\t1\t6\t1\tW\ta\t1\t6\t+\n" "p1\t7\t9\t2\tW\tb\t4\t6\t-\n" "p1\t10\t12\t3\tN\t3\tscaffold\tyes\tpaired-ends\n"
                          "p1\t13\t12\t4\tW\te\t9\t8\t+\n" "c\t1\t5\t1\tW\tc\t1\t5\t+\n")
    dev.sync()


# ---------------------------------------------------------------- under the SIMT mock

@pytest.fixture(scope="module")
def sim_dev():
    from sim import simlib
    dev = simlib.device()
    yield dev
    dev.close()


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_sim_fixture(sim_dev, tmp_path, n):
    check_fixture(sim_dev, tmp_path, n)


def test_sim_tsv_form(sim_dev, tmp_path):
    check_tsv_form(sim_dev, tmp_path)


def test_sim_cli(tmp_path):
    from sim import simlib
    check_cli(tmp_path, dict(os.environ, NTLINK_AMD_LIB=simlib.build()))


@pytest.mark.parametrize("with_tsv", [False, True])
@pytest.mark.parametrize("i", [0, 1, 2])
def test_sim_golden(sim_dev, tmp_path, i, with_tsv):
    check_golden(sim_dev, tmp_path, i, with_tsv)


def test_sim_golden_in_batches(sim_dev, tmp_path):
    case = golden()[0]
    args = golden_inputs(case, tmp_path, False)
    overlap.overlap_sequences(args, sim_dev, batch_bases=1)  # a device pass per path line
    assert {s: t.decode() for s, t in texts(args.p).items()} == case["files"]


def test_sim_refusals(sim_dev, tmp_path):
    check_refusals(sim_dev, tmp_path)


def test_sim_writers(sim_dev, tmp_path):
    check_writers(sim_dev, tmp_path)


# ---------------------------------------------------------------- on the GPU

@pytest.fixture(scope="module")
def gpu_dev():
    dev = capi.Device(0)
    yield dev
    dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_gpu_fixture(gpu_dev, tmp_path, n):
    check_fixture(gpu_dev, tmp_path, n)


@pytest.mark.gpu
def test_gpu_tsv_form(gpu_dev, tmp_path):
    check_tsv_form(gpu_dev, tmp_path)


@pytest.mark.gpu
def test_gpu_cli(tmp_path):
    check_cli(tmp_path, dict(os.environ))


@pytest.mark.gpu
@pytest.mark.parametrize("with_tsv", [False, True])
@pytest.mark.parametrize("i", [0, 1, 2])
def test_gpu_golden(gpu_dev, tmp_path, i, with_tsv):
    check_golden(gpu_dev, tmp_path, i, with_tsv)


@pytest.mark.gpu
def test_gpu_refusals(gpu_dev, tmp_path):
    check_refusals(gpu_dev, tmp_path)


@pytest.mark.gpu
def test_gpu_writers(gpu_dev, tmp_path):
    check_writers(gpu_dev, tmp_path)
