"""The filter in front of the overlap stage's sketch (ntlink_amd/filter_sequences.py, bin/ntlink_filter_sequences.py) -- under the SIMT
mock and on the GPU, the same checks.
  a. the reference's four scaffolds_N.fa with their shipped .stitch.path and .n1.scaffold.dot: the output equal to a restatement of
     filter_sequences (bin/ntlink_filter_sequences.py:17-31) over seqio records
  b. a crafted case: a contig with two valid regions that occurs on two path lines, printed once per occurrence; a path without an
     overlap, which gives its LAST record only; a contig that is missing from the FASTA file -- exit status 1 and NOTHING on standard
     output: every contig of the path file is looked up before the first byte is written
  c. on the GPU, in child processes: bin/ntlink_filter_sequences.py | bin/indexlr --long --pos -k 15 -w 5 - |
     bin/ntlink_overlap_sequences.py -m - (ntLink:247-251) leaves the shipped .trimmed_scafs.path, .agp and .tsv"""
import argparse
import os
import re
import subprocess
import sys

import pytest

from ntlink_amd import capi, filter_sequences, overlap, seqio

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.path.join(HERE, "golden", "ref")
BIN = os.path.join(ROOT, "bin")
FIXTURES = {1: "scaffolds_1.fa.k32.w250.z1000", 2: "scaffolds_2.fa.k32.w100.z1000", 3: "scaffolds_3.fa.k24.w250.z1000", 4: "scaffolds_4.fa.k40.w100.z1000"}
GAP_RE = re.compile(r"^(\d+)N$")


def fixture_args(n):
    base = os.path.join(REF, "expected_outputs", FIXTURES[n])
    return argparse.Namespace(fasta=os.path.join(REF, f"scaffolds_{n}.fa"), dot=base + ".n1.scaffold.dot", path=base + ".stitch.path", k=15, f=0.5, g=20, t=4)


def restated(args):
    "filter_sequences of the reference, :17-31, over the records as seqio reads them"
    ss = seqio.load_all([args.fasta])
    off = ss.offsets.tolist()
    sequences = {name: bytes(ss.buf[off[i]:off[i + 1]]).decode() for i, name in enumerate(ss.names.tolist())}
    scaffolds = {name: overlap.ScaffoldCut(name, length=len(seq)) for name, seq in sequences.items()}
    graph, _ = overlap.read_scaffold_graph(args.dot)
    valid_mx_regions = overlap.find_valid_mx_regions(args, GAP_RE, graph, scaffolds)
    out = []
    with open(args.path) as path_fin:
        for path in path_fin:
            path_name, path_seq = path.strip().split("\t")
            path_seq = overlap.normalize_path(path_seq.split(" "), GAP_RE)
            for node in path_seq:
                if re.search(GAP_RE, node):
                    continue
                node_name = node.strip("+-")
                if node_name in valid_mx_regions:
                    out.append(">{}\n{}\n".format(node_name, sequences[node_name]))
            out.append(">LAST{}\nN\n".format(path_name))
    return "".join(out), valid_mx_regions


def run(dev, args, tmp_path, max_bytes=None):
    out = str(tmp_path / "filtered.fa")
    filter_sequences.filter_sequences(args, out, dev, max_bytes=max_bytes)
    with open(out) as fh:
        return fh.read()


def check_fixtures(dev, tmp_path):
    printed = 0
    for n in FIXTURES:
        want, regions = restated(fixture_args(n))
        assert run(dev, fixture_args(n), tmp_path) == want, f"fixture {n}"
        printed += len(regions)
    assert printed >= 4  # fixture 4 has the real overlaps: scaf1 .. scaf4
    assert run(dev, fixture_args(4), tmp_path, max_bytes=10000) == restated(fixture_args(4))[0]  # a stitch call per record
    dev.sync()


def crafted(tmp_path, missing=False):
    seqs = {"A": "ACGTTGCA" * 40, "B": "GGATCcnAT" * 50, "C": "TTGACA" * 70, "D": "CATG" * 90, "E": "AAGT" * 30, "F": "CCTG" * 30}
    with open(tmp_path / "in.fa", "w") as fh:
        for name, seq in seqs.items():
            if not (missing and name == "F"):
                fh.write(f">{name} a comment\n{seq}\n")
    flip = lambda v: v[:-1] + ("-" if v[-1] == "+" else "+")
    edges = [("A+", "B+", -30), ("B+", "C-", -25), ("D+", "B-", -40), ("E+", "F+", 120)]
    with open(tmp_path / "in.dot", "w") as fh:
        fh.write("digraph G {\n" + "".join(f'"{n}{o}" [l={len(s)}]\n' for n, s in seqs.items() for o in "+-"))
        for s, t, d in edges:
            fh.write(f'"{s}" -> "{t}" [d={d} e=0 n=3]\n"{flip(t)}" -> "{flip(s)}" [d={d} e=0 n=3]\n')
        fh.write("graph [scaf_num=5]\n}\n")
    with open(tmp_path / "in.path", "w") as fh:
        fh.write("ntLink_6\tA+ 1N B+ 1N C-\n")   # B: the target of one pair and the source of the next
        fh.write("ntLink_7\tD+ 1N B-\n")         # B again, on another line
        fh.write("ntLink_8\tE+ 121N F+\n")       # no overlap
    return argparse.Namespace(fasta=str(tmp_path / "in.fa"), dot=str(tmp_path / "in.dot"), path=str(tmp_path / "in.path"), k=15, f=0.5, g=20, t=4)


def check_crafted(dev, tmp_path):
    args = crafted(tmp_path)
    want, regions = restated(args)
    assert len(regions["B"]) == 3 and want.count(">B\n") == 2 and want.endswith(">LASTntLink_7\nN\n>LASTntLink_8\nN\n") and ">E" not in want
    assert "GGATCcnAT" in want  # the bytes as they are in the file
    assert run(dev, args, tmp_path) == want
    args = crafted(tmp_path, missing=True)
    out = str(tmp_path / "nothing.fa")
    with open(out, "w") as fh:
        with pytest.raises(ValueError, match="contig F is not in the FASTA file"):
            filter_sequences.filter_sequences(args, fh.fileno(), dev)
    assert os.path.getsize(out) == 0
    dev.sync()


def cli(args, env):
    return subprocess.run([sys.executable, os.path.join(BIN, "ntlink_filter_sequences.py"), "--fasta", args.fasta, "--dot", args.dot, "--path", args.path,
                           "-k", "15", "-g", "20", "-t", "4"], env=env, capture_output=True, text=True, timeout=120)


def check_cli(tmp_path, env):
    args = crafted(tmp_path)
    done = cli(args, env)
    assert done.returncode == 0 and done.stdout == restated(args)[0], done.stderr
    bad = cli(crafted(tmp_path, missing=True), env)
    assert bad.returncode == 1 and bad.stdout == "" and "ERROR" in bad.stderr and "contig F" in bad.stderr


# ---------------------------------------------------------------- under the SIMT mock

@pytest.fixture(scope="module")
def sim_dev():
    from sim import simlib
    dev = simlib.device()
    yield dev
    dev.close()


def test_sim_fixtures(sim_dev, tmp_path):
    check_fixtures(sim_dev, tmp_path)


def test_sim_crafted(sim_dev, tmp_path):
    check_crafted(sim_dev, tmp_path)


def test_sim_cli(sim_dev, tmp_path):
    from sim import simlib
    check_cli(tmp_path, dict(os.environ, NTLINK_AMD_LIB=simlib.build()))


# ---------------------------------------------------------------- on the GPU

@pytest.fixture(scope="module")
def gpu_dev():
    dev = capi.Device(0)
    yield dev
    dev.close()


@pytest.mark.gpu
def test_gpu_fixtures(gpu_dev, tmp_path):
    check_fixtures(gpu_dev, tmp_path)


@pytest.mark.gpu
def test_gpu_crafted(gpu_dev, tmp_path):
    check_crafted(gpu_dev, tmp_path)


@pytest.mark.gpu
def test_gpu_cli(tmp_path):
    check_cli(tmp_path, dict(os.environ))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 4])
def test_gpu_makefile_pipe(tmp_path, n):
    """ntLink:247-251 with its defaults, three child processes joined by pipes (fixture 1 as the issue names it; fixture 4 has the overlaps)"""
    a = fixture_args(n)
    prefix = str(tmp_path / "out")
    py = sys.executable
    pipe = (f"set -o pipefail; '{py}' '{BIN}/ntlink_filter_sequences.py' --fasta '{a.fasta}' --dot '{a.dot}' --path '{a.path}' -k 15 -g 20 -t 4 | "
            f"'{py}' '{BIN}/indexlr' --long --pos -k 15 -w 5 -t 4 - | "
            f"'{py}' '{BIN}/ntlink_overlap_sequences.py' -m - --path '{a.path}' -s '{a.fasta}' -d '{a.dot}' -p '{prefix}' -g 20 -k 15 --outgap 0 --trim_info")
    done = subprocess.run(["bash", "-c", pipe], capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr
    base = os.path.join(REF, "expected_outputs", FIXTURES[n]) + ".trimmed_scafs."
    for suffix in ("path", "agp", "tsv"):
        with open(f"{prefix}.trimmed_scafs.{suffix}") as got, open(base + suffix) as want:
            assert got.read() == want.read(), suffix
