"""The merge stage and the count kernel on the device (merge.merge_contigs -> ntl_stitch, ntl_stitched_base_counts,
csrc/count_kernels.h; bin/MergeContigs), under the SIMT mock and on the GPU, the same checks.
  a. the reference's four cases byte for byte through merge_contigs, with the counts of every record and their abyss-fac line, and
     through bin/MergeContigs as a child process (standard output, -o, --stats; -k 3 and a bad path exit non-zero, no file left)
  b. the resident form behind the overlap stage (merge.merge_after_overlap: the store the stage holds, trimmed coordinates mapped onto
     the untrimmed records) gives the bytes of the file form, for the four cases
  c. max_bytes so small that every record is a stitch call of its own and one exceeds it; unpathed contigs with comments first
  d. the count kernel against numpy on one crafted text cut many ways (merge_cases.count_cases): records of 0, 1, 15, 16, 17 bytes, a
     record ending on a tile boundary, one over three tiles, 200 one-byte records in one tile, N n U newline > and IUPAC codes, a
     total that is no multiple of 16; n_rec = 0; NTL_EINVAL for offsets that descend or run past the end"""
import os
import subprocess
import sys

import numpy as np
import pytest

import merge_cases as mc
from ntlink_amd import capi, merge
from test_overlap_stage import fixture_args

ROOT = mc.ROOT


def check_case(dev, tmp_path, n):
    out = str(tmp_path / "merged.fa")
    got = merge.merge_contigs(mc.trimmed_fasta(n), mc.case_file(n, ".trimmed_scafs.path"), out, dev)
    with open(out, "rb") as fh:
        assert fh.read() == mc.golden(n)
    assert got.counts.dtype == np.uint64 and np.array_equal(got.counts, mc.counts_of_fasta(mc.golden(n)))
    with open(mc.case_file(n, ".ntLink.scaffolds.fa.abyssfac.tsv")) as fh:
        assert merge.fac_text(merge.fac_stats(got.counts), mc.CASES[n] + ".ntLink.scaffolds.fa") == fh.read()
    dev.sync()


def check_after_overlap(dev, tmp_path, n):
    """the overlap stage from the untrimmed scaffolds_n.fa, the merge from its store: the bytes the file form makes of the files the
    stage wrote, which are the reference's (test_overlap_stage.check_fixture), so both equal the reference's merge output"""
    args = fixture_args(n, str(tmp_path / "ov"))
    out = str(tmp_path / "resident.fa")
    _scaffolds, _paths, got = merge.merge_after_overlap(args, out, dev)
    via_file = str(tmp_path / "file.fa")
    again = merge.merge_contigs(args.p + ".trimmed_scafs.fa", args.p + ".trimmed_scafs.path", via_file, dev)
    with open(out, "rb") as a, open(via_file, "rb") as b:
        text = a.read()
        assert text == b.read() and text == mc.golden(n)
    assert np.array_equal(got.counts, again.counts) and np.array_equal(got.counts, mc.counts_of_fasta(text))
    assert got.plan.headers == again.plan.headers
    dev.sync()


def check_small_calls(dev, tmp_path):
    rng = np.random.default_rng(3)
    seqs = {f"c{i}": mc.ALPHABET[rng.integers(0, 20, n)].tobytes() for i, n in enumerate((300, 1, 77, 40000, 16, 5, 123))}
    fasta, path = tmp_path / "in.fa", tmp_path / "in.path"
    fasta.write_bytes(b"".join(b">" + name.encode() + (b" 3-9 note" if name == "c4" else b"") + b"\n" + seq + b"\n" for name, seq in seqs.items()))
    path.write_text("s1\tc3- 1N c0+ 20N c2-\ns2\tc6+ 1N c1-\n")
    S = seqs
    rc = lambda s: s[::-1].translate(mc.TABLE)
    low = lambda s: s[:1].lower() + s[1:]
    want = b">c4 3-9 note\n" + S["c4"] + b"\n>c5\n" + S["c5"] + b"\n" + \
           b">s1 40396 0 c3-,...,c2-\n" + rc(S["c3"]) + low(S["c0"]) + b"N" * 19 + rc(S["c2"]) + b"\n" + \
           b">s2 124 0 c6+,1N,c1-\n" + S["c6"] + low(rc(S["c1"])) + b"\n"
    for max_bytes in (None, 200):  # 200: every record alone, s1 larger than the bound
        out = str(tmp_path / f"out{max_bytes}.fa")
        got = merge.merge_contigs(str(fasta), str(path), out, dev, max_bytes=max_bytes)
        with open(out, "rb") as fh:
            assert fh.read() == want
        assert np.array_equal(got.counts, mc.counts_of_fasta(want)) and got.plan.n_unpathed == 2
    # a contig of the path that the FASTA does not have: ValueError before anything is written
    path.write_text("s1\tc3- 1N c9+\n")
    with pytest.raises(ValueError, match="in.path:1: node 'c9\\+'"):
        merge.merge_contigs(str(fasta), str(path), str(tmp_path / "never.fa"), dev)
    assert not os.path.exists(tmp_path / "never.fa")
    dev.sync()


def check_cli(tmp_path, env):
    exe = [sys.executable, os.path.join(ROOT, "bin", "MergeContigs")]
    for n in (1, 2, 3, 4):
        fa, path = mc.trimmed_fasta(n), mc.case_file(n, ".trimmed_scafs.path")
        if n % 2:  # standard output
            done = subprocess.run(exe + ["-k2", fa, path], env=env, capture_output=True, timeout=300)
            assert done.returncode == 0, done.stderr
            assert done.stdout == mc.golden(n)
        else:      # -o and --stats
            out, stats = tmp_path / f"m{n}.fa", tmp_path / f"m{n}.tsv"
            done = subprocess.run(exe + ["-k", "2", "-o", str(out), "--stats", str(stats), fa, path], env=env, capture_output=True, timeout=300)
            assert done.returncode == 0 and done.stdout == b"", done.stderr
            assert out.read_bytes() == mc.golden(n)
            with open(mc.case_file(n, ".ntLink.scaffolds.fa.abyssfac.tsv")) as fh:
                assert stats.read_text() == fh.read().replace(mc.CASES[n] + ".ntLink.scaffolds.fa", str(out))
    fa, path = mc.trimmed_fasta(4), mc.case_file(4, ".trimmed_scafs.path")
    bad = subprocess.run(exe + ["-k", "3", fa, path], env=env, capture_output=True, timeout=300)
    assert bad.returncode == 2 and b"-k2" in bad.stderr and bad.stdout == b""
    broken = tmp_path / "broken.path"
    broken.write_text("s\tscaf1+ scaf2+\n")
    bad = subprocess.run(exe + ["-o", str(tmp_path / "bad.fa"), fa, str(broken)], env=env, capture_output=True, timeout=300)
    assert bad.returncode == 1 and b"ERROR: ValueError" in bad.stderr and b"broken.path:1: node 'scaf2+'" in bad.stderr
    assert not os.path.exists(tmp_path / "bad.fa")


def check_counts(dev):
    text, cases = mc.count_cases()
    want = mc.count_reference()
    assert want["whole"][0] == mc.called(text).sum() and 0 < want["whole"][0] < len(text)
    assert want["one_byte_records"][:200].max() == 1 and want["three_tiles_aligned"][0] > 8000
    with dev.ascii([text]) as store, dev.stitch([store], [(0, 0, 0, len(text), 0)]) as st:
        assert st.nbytes == len(text)
        for name, off in cases.items():
            got = st.base_counts(off)
            assert got.dtype == np.uint64 and len(got) == len(off) - 1, name
            assert np.array_equal(got, want[name]), (name, np.flatnonzero(got != want[name])[:5])
        # no record at all: nothing is asked of the device
        assert len(st.base_counts([])) == 0 and len(st.base_counts([17])) == 0
        # refusals
        for off, why in (([0, 10, 9], "descends at record 1"), ([5, 4], "descends at record 0"), ([0, len(text) + 1], "beyond the result's"),
                         ([len(text) + 1, len(text) + 2], "beyond the result's")):
            with pytest.raises(capi.NtlError) as e:
                st.base_counts(off)
            assert e.value.code == capi.NTL_EINVAL and why in str(e.value), str(e.value)
        assert np.array_equal(st.base_counts(cases["halves"]), want["halves"])  # the handle is as good as before
        with dev.stitch([store], []) as empty:  # an empty text
            assert empty.base_counts([0, 0, 0]).tolist() == [0, 0]
            with pytest.raises(capi.NtlError):
                empty.base_counts([0, 1])
    dev.sync()


# ---------------------------------------------------------------- under the SIMT mock

@pytest.fixture(scope="module")
def sim_dev():
    from sim import simlib
    dev = simlib.device()
    yield dev
    dev.close()


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_sim_case(sim_dev, tmp_path, n):
    check_case(sim_dev, tmp_path, n)


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_sim_after_overlap(sim_dev, tmp_path, n):
    check_after_overlap(sim_dev, tmp_path, n)


def test_sim_small_calls(sim_dev, tmp_path):
    check_small_calls(sim_dev, tmp_path)


def test_sim_cli(tmp_path):
    from sim import simlib
    check_cli(tmp_path, dict(os.environ, NTLINK_AMD_LIB=simlib.build()))


def test_sim_counts(sim_dev):
    check_counts(sim_dev)


# ---------------------------------------------------------------- on the GPU

@pytest.fixture(scope="module")
def gpu_dev():
    dev = capi.Device(0)
    yield dev
    dev.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_gpu_case(gpu_dev, tmp_path, n):
    check_case(gpu_dev, tmp_path, n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_gpu_after_overlap(gpu_dev, tmp_path, n):
    check_after_overlap(gpu_dev, tmp_path, n)


@pytest.mark.gpu
def test_gpu_small_calls(gpu_dev, tmp_path):
    check_small_calls(gpu_dev, tmp_path)


@pytest.mark.gpu
def test_gpu_cli(tmp_path):
    check_cli(tmp_path, dict(os.environ))


@pytest.mark.gpu
def test_gpu_counts(gpu_dev):
    check_counts(gpu_dev)
