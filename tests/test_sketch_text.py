"""ntl_sketch_format (csrc/sketch_text_kernels.h), capi.Sketch.text and the NTL_INDEXLR_DEVICE_TEXT switch of the drivers -- under the SIMT
mock and on the GPU, the same checks.

Every device check holds the concatenated pieces of Sketch.text BYTE FOR BYTE against formats.write_indexlr on the downloaded records
of the same sketch (the host emitter: the parent's behaviour, pinned to the reference's goldens by the existing tests).  Crafted
sketches come through ntl_sketch_from_host, so no sequence has to hash to an awkward value.

  digits       hashes 0, 9, 10^n - 1 and 10^n up to n = 19, 2^64 - 1; positions and lengths on both sides of every digit count up to
               2^32 - 1; both strands; the three column forms
  empty lines  a sequence without minimizers first, last, in the middle, two in a row; none anywhere; nseq = 0; an empty range; a name
               of zero bytes; a name of 300 bytes
  shapes       1, 63 .. 65, 255 .. 257 minimizers; one sequence of 70 000; 1 000 sequences of one; totals and sequence counts around a
               workgroup multiple
  pieces       a cut at every sequence boundary in turn (NTL_SKETCH_TEXT_MAX_BYTES); a range given to the call directly; one sequence
               above the limit refused with its message, and the context still good
  refusals     a sketch without records, a short name table, bad ranges
  goldens      the four contig TSVs the reference ships, from their FASTA files; the H:pos form of the overlap stage's stream
  drivers      run_indexlr with the switch on and off; bin/indexlr to a pipe and to a file; bin/ntLink pair's contig TSV
  random       200 seeded sketches, zeros included, random column form"""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

from helpers import FIXTURES, REF, read_text
from ntlink_amd import capi, filter_sequences, formats, pipeline, seqio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "bin")
FORMS = ((False, True), (True, True), (False, False))  # (with_len, with_strand): pos+strand, pos+strand+len, pos only
U64 = [0, 9] + [v for n in range(1, 20) for v in (10 ** n - 1, 10 ** n)] + [2 ** 64 - 1]
U32 = [0] + [v for n in range(1, 10) for v in (10 ** n - 1, 10 ** n)] + [2 ** 32 - 1]
WORKGROUP = 256  # SKTEXT_NT


def host_text(names, lengths, cols, with_len, with_strand):
    "formats.write_indexlr on the downloaded columns"
    fh = io.StringIO()
    formats.write_indexlr(fh, list(names), lengths, *cols, with_len, with_strand)
    return fh.getvalue().encode()


def device_text(dev, sk, tab, with_len, with_strand, **kw):
    out = []
    for piece in sk.text(tab, with_len, with_strand, **kw):
        out.append(bytes(piece))
        dev.pinned_release(piece)
    return out


def make(counts, seed=0, names=None, lengths=None):
    "a crafted sketch's arrays: counts[i] minimizers for sequence i, values of every digit count"
    rng = np.random.default_rng(seed)
    counts = np.asarray(counts, np.int64)
    n = int(counts.sum())
    off = np.zeros(len(counts) + 1, np.uint64)
    np.cumsum(counts, out=off[1:])
    h = rng.integers(0, 2 ** 64, n, dtype=np.uint64) >> rng.integers(0, 64, n).astype(np.uint64)
    p = (rng.integers(0, 2 ** 32, n, dtype=np.uint64) >> rng.integers(0, 32, n).astype(np.uint64)).astype(np.uint32)
    s = rng.integers(0, 2, n).astype(np.uint8)
    if names is None:
        names = [f"seq{i}" + "x" * int(rng.integers(0, 9)) for i in range(len(counts))]
    if lengths is None:
        lengths = (rng.integers(0, 2 ** 32, len(counts), dtype=np.uint64) >> rng.integers(0, 32, len(counts)).astype(np.uint64)).astype(np.uint32)
    return names, np.asarray(lengths, np.uint32), (off, h, p, s)


def check_sketch(dev, names, lengths, cols, label, forms=FORMS, **kw):
    "the device text of the arrays, in every column form, against the host emitter on what the sketch gives back"
    with dev.sketch_from_arrays(*cols) as sk, dev.names(names, lengths) as tab:
        down = sk.download()
        for a, b in zip(down, cols):
            assert np.array_equal(a, b), label
        for with_len, with_strand in forms:
            want = host_text(names, lengths, down, with_len, with_strand)
            got = b"".join(device_text(dev, sk, tab, with_len, with_strand, **kw))
            assert got == want, f"{label}: len={with_len} strand={with_strand}"
    return want


# ---------------------------------------------------------------- the checks (the same for the mock and the GPU)

def check_digits(dev):
    # sequence i: every hash at position U32[i], its length U32[i]; strands alternate, and once the other way round
    for flip in (0, 1):
        nseq = len(U32)
        off = np.arange(nseq + 1, dtype=np.uint64) * np.uint64(len(U64))
        h = np.tile(np.array(U64, np.uint64), nseq)
        p = np.repeat(np.array(U32, np.uint32), len(U64))
        s = ((np.arange(len(h)) + flip) & 1).astype(np.uint8)
        text = check_sketch(dev, [f"s{i}" for i in range(nseq)], np.array(U32, np.uint32), (off, h, p, s), "digits")
    assert b"\t0:0 9:0 " in text and text.endswith(b" 18446744073709551615:4294967295\n")  # (the last form: pos only)


def check_empty_lines(dev):
    for counts in ([0, 2, 1], [2, 1, 0], [1, 0, 2], [1, 0, 0, 2], [0, 0, 3, 0, 0], [0], [0, 0, 0], []):
        names, lengths, cols = make(counts, seed=len(counts))
        text = check_sketch(dev, names, lengths, cols, f"counts {counts}")
        assert text.count(b"\n") == len(counts)
    names, lengths, cols = make([2, 0, 3], names=["a", "", "b" * 300])
    text = check_sketch(dev, names, lengths, cols, "a name of zero bytes, a name of 300")
    assert b"\n\t" in text and b"b" * 300 + b"\t" in text
    # an empty range, at either end and in the middle, and on a sketch without sequences
    with dev.sketch_from_arrays(*cols) as sk, dev.names(names, lengths) as tab:
        for at in (0, 1, 3):
            with sk.format(tab, True, True, at, at) as t:
                assert t.nbytes == 0 and len(t.download()) == 0
    with dev.sketch_from_arrays(np.zeros(1, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint8)) as sk, \
            dev.names([], []) as tab:
        with sk.format(tab, True, True) as t:
            assert t.nbytes == 0


def check_shapes(dev):
    one = FORMS[1:2]
    check_sketch(dev, *make([1, 63, 64, 65, 255, 256, 257], seed=1), "around a wavefront and a workgroup")
    check_sketch(dev, *make([70000], seed=2), "one sequence of 70 000", forms=one)  # the search crosses 274 workgroups
    check_sketch(dev, *make([1] * 1000, seed=3), "1 000 sequences of one", forms=one)
    for total in (WORKGROUP - 1, WORKGROUP, WORKGROUP + 1, 2 * WORKGROUP - 1, 2 * WORKGROUP, 2 * WORKGROUP + 1):
        check_sketch(dev, *make([100, 0, total - 100], seed=total), f"{total} minimizers", forms=one)
        check_sketch(dev, *make([1, 0] * (total // 2) + [2] * (total % 2), seed=total), f"{total} sequences", forms=one)  # more lines than tokens in the last block


PIECE_COUNTS = [9, 7, 7, 5, 3, 3, 1, 0]  # no sequence's bound above the first one's: every cut below leaves pieces that fit


def check_pieces(dev, monkeypatch):
    names, lengths, cols = make(PIECE_COUNTS, seed=5, names=[f"n{i}" for i in range(len(PIECE_COUNTS))])
    with dev.sketch_from_arrays(*cols) as sk, dev.names(names, lengths) as tab:
        whole = b"".join(device_text(dev, sk, tab, True, True))
        assert whole == host_text(names, lengths, cols, True, True)
        lines = whole.splitlines(keepends=True)
        per_seq, per_mx = int(dev.L.ntl_sketch_text_bound(tab.ptr, 1, 0)), int(dev.L.ntl_sketch_text_bound(tab.ptr, 0, 1))
        assert (per_seq, per_mx) == (2 + 13, 34)
        for cut in range(1, len(PIECE_COUNTS)):  # the largest limit that still cuts behind sequence cut - 1
            limit = per_mx * sum(PIECE_COUNTS[:cut]) + per_seq * cut + 1
            monkeypatch.setenv("NTL_SKETCH_TEXT_MAX_BYTES", str(limit))
            ranges = sk.text_ranges(tab)
            assert ranges[0] == (0, cut) and ranges[-1][1] == len(PIECE_COUNTS) and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
            pieces = device_text(dev, sk, tab, True, True)
            assert len(pieces) == len(ranges) >= 2 and pieces[0] == b"".join(lines[:cut]) and b"".join(pieces) == whole, cut
            monkeypatch.delenv("NTL_SKETCH_TEXT_MAX_BYTES")
            assert sk.text_ranges(tab, piece_bytes=limit) == ranges  # the Python-side piece size cuts by the same rule
        assert sk.text_ranges(tab) == [(0, len(PIECE_COUNTS))]
        # a range given to the call directly is the matching slice
        for lo, hi in ((0, 1), (2, 5), (6, 8), (7, 8), (0, 8)):
            with sk.format(tab, True, True, lo, hi) as t:
                piece = t.download()
                assert bytes(piece) == b"".join(lines[lo:hi]) and t.nbytes == len(piece), (lo, hi)
                dev.pinned_release(piece)
        # one sequence above the limit: refused, not split -- and the next call on the same context works
        monkeypatch.setenv("NTL_SKETCH_TEXT_MAX_BYTES", str(per_mx * PIECE_COUNTS[0] + per_seq))
        assert sk.text_ranges(tab)[0] == (0, 1)
        with pytest.raises(capi.NtlError, match=r"sequences \[0, 1\) may take 321 bytes, one call makes fewer than 321") as ei:
            device_text(dev, sk, tab, True, True)
        assert ei.value.code == capi.NTL_ERANGE
        with sk.format(tab, True, True, 1, 2) as t:  # (the second sequence fits)
            assert bytes(t.download()) == lines[1]
        monkeypatch.delenv("NTL_SKETCH_TEXT_MAX_BYTES")
        assert b"".join(device_text(dev, sk, tab, True, True)) == whole
    dev.sync()


def check_refusals(dev):
    names, lengths, cols = make([2, 1], seed=7)

    def refused(sk, tab, message, *args):
        with pytest.raises(capi.NtlError, match=message) as ei:
            sk.format(tab, True, True, *args)
        assert ei.value.code == capi.NTL_EINVAL, message
    with dev.sketch_from_arrays(*cols) as sk, dev.names(names, lengths) as tab, dev.names(names[:1], lengths[:1]) as short:
        refused(sk, short, "the name table holds fewer names than the sketch has sequences")
        refused(sk, tab, r"the range \[2, 1\) is not one of the sketch's 2 sequences", 2, 1)
        refused(sk, tab, r"the range \[0, 3\) is not one of the sketch's 2 sequences", 0, 3)
        refused(sk, tab, r"the range \[3, 3\) is not one of the sketch's 2 sequences", 3, 3)
        with pytest.raises(capi.NtlError, match="unknown flag bits"):
            p = capi.C.c_void_p()
            dev._chk(dev.L.ntl_sketch_format(sk.ptr, tab.ptr, 4, 0, 2, capi.C.byref(p)))
        assert b"".join(device_text(dev, sk, tab, True, True)) == host_text(names, lengths, cols, True, True)  # ... and the sketch is still good
    # a sketch made only to be mapped holds no records
    seq = np.random.default_rng(3).choice(np.frombuffer(b"ACGT", np.uint8), 3000).tobytes()
    with dev.batch([seq, seq[500:]]) as b, dev.sketch(b, 15, 5) as csk, dev.index(csk, [3000, 2500]) as ix, \
            dev.sketch(b, 15, 5, index=ix, records=False) as fm, dev.names(["a", "b"], [3000, 2500]) as tab:
        assert not fm.has_records
        refused(fm, tab, "a sketch made by ntl_sketch_run_for_map holds no records")
        assert b"".join(device_text(dev, csk, tab, True, True)) == host_text(["a", "b"], [3000, 2500], csk.download(), True, True)
    dev.sync()


def _file_sketch_text(dev, path, k, w, with_len, with_strand):
    "(device text, host text) of one FASTA file sketched on the device"
    ss = seqio.load_all([path])
    with dev.batch(ss.buf, ss.offsets) as b, dev.sketch(b, k, w) as sk, dev.names(ss.names, ss.lengths) as tab:
        got = b"".join(device_text(dev, sk, tab, with_len, with_strand))
        return got, host_text(ss.names.tolist(), ss.lengths, sk.download(), with_len, with_strand)


def check_goldens(dev, tmp_path):
    for _tag, target, _reads, k, w, gold in FIXTURES[:4]:
        got, host = _file_sketch_text(dev, os.path.join(REF, target), k, w, False, True)
        with open(os.path.join(REF, "expected_outputs", gold + ".tsv"), "rb") as fh:
            assert got == fh.read() == host, gold
    # the H:pos form, of the stream tests/test_filter_sequences.py feeds the overlap stage (ntLink:244,249)
    import test_filter_sequences as tf
    filtered = str(tmp_path / "filtered.fa")
    filter_sequences.filter_sequences(tf.fixture_args(4), filtered, dev)
    got, host = _file_sketch_text(dev, filtered, 15, 5, False, False)
    assert got == host and got.count(b"\n") >= 4 and b":+" not in got and b":-" not in got and len(got) > 20000


def check_driver(dev, tmp_path, monkeypatch):
    "run_indexlr: the switch, its default, and what runs behind it"
    rng = np.random.default_rng(11)
    paths = [str(tmp_path / "in.fa")]
    with open(paths[0], "w") as fh:  # six records, one without a k-mer, one of N: lines without tokens among the others
        for i, n in enumerate((2500, 3100, 20, 1800, 2200, 2900)):
            seq = "N" * n if i == 3 else "".join(rng.choice(list("ACGT"), n))
            fh.write(f">r{i} comment\n{seq}\n")
    dev.prof_enable(True)
    try:
        outs = {}
        for label, env, arg in (("unset", None, None), ("env 1", "1", None), ("arg on", "0", True), ("arg off", "1", False)):
            if env is None:
                monkeypatch.delenv("NTL_INDEXLR_DEVICE_TEXT", raising=False)
            else:
                monkeypatch.setenv("NTL_INDEXLR_DEVICE_TEXT", env)
            dev.prof_reset()
            with open(tmp_path / "out.tsv", "w") as fh:
                pipeline.run_indexlr(dev, paths, 32, 20, fh, True, batch_bases=5000, device_text=arg)  # (several batches)
            dev.sync()
            outs[label] = (tmp_path / "out.tsv").read_bytes()
            assert (dev.prof_get("sketch_text")[1] >= 1) == (label in ("env 1", "arg on")), label  # (off: nothing is formatted on the device)
    finally:
        dev.prof_enable(False)
    assert len(set(outs.values())) == 1 and outs["unset"].count(b"\n") == 6 and b"r2\t20\t\n" in outs["unset"] and len(outs["unset"]) > 10000


def _run_all(cmds):
    "the child processes side by side; -> their (return code, stdout bytes)"
    procs = [subprocess.Popen(cmd, env=env, stdout=out, stderr=subprocess.PIPE) for cmd, env, out in cmds]
    done = []
    for p in procs:
        stdout, stderr = p.communicate(timeout=300)
        assert p.returncode == 0, stderr.decode()
        done.append(stdout)
    return done


CLI_INPUTS = {"fasta": ["scaffolds_1.fa"], "fq.gz": ["long_reads_2.fq.gz"], "two files": ["scaffolds_1.fa", "scaffolds_4.fa"]}


def check_cli(tmp_path, env, which, fastq_records=None):
    """bin/indexlr with the switch on and off, to a pipe and to a file: the same bytes.  fastq_records (the mock, which sketches a
    base in microseconds): the first so many records of the .fq.gz fixture, gzipped again, instead of all of it"""
    files = [os.path.join(REF, n) for n in CLI_INPUTS[which]]
    if fastq_records and which == "fq.gz":
        import gzip
        ss = seqio.load_all(files)
        off = ss.offsets.tolist()
        files = [str(tmp_path / "head.fq.gz")]
        with gzip.open(files[0], "wb") as fh:
            for i, name in enumerate(ss.names.tolist()[:fastq_records]):
                seq = bytes(ss.buf[off[i]:off[i + 1]])
                fh.write(b"@" + name.encode() + b"\n" + seq + b"\n+\n" + b"I" * len(seq) + b"\n")
    cmd = [sys.executable, os.path.join(BIN, "indexlr"), "--long", "--pos", "--strand", "--len", "-k", "32", "-w", "100", "-t", "4"] + files
    on, off = dict(env, NTL_INDEXLR_DEVICE_TEXT="1"), {k: v for k, v in env.items() if k != "NTL_INDEXLR_DEVICE_TEXT"}
    with open(tmp_path / "on.tsv", "wb") as f_on, open(tmp_path / "off.tsv", "wb") as f_off:
        pipe_on, pipe_off, _a, _b = _run_all([(cmd, on, subprocess.PIPE), (cmd, off, subprocess.PIPE), (cmd, on, f_on), (cmd, off, f_off)])
    assert pipe_on == pipe_off == (tmp_path / "on.tsv").read_bytes() == (tmp_path / "off.tsv").read_bytes()
    assert pipe_on.count(b"\n") >= 2 and len(pipe_on) > 10000


def check_pair_cli(tmp_path, env):
    "bin/ntLink pair with the switch on leaves the <target>.k<k>.w<w>.tsv the reference ships"
    import shutil
    for n in ("scaffolds_4.fa", "long_reads_4_top5.fa"):
        shutil.copy(os.path.join(REF, n), tmp_path / n)
    cmd = [sys.executable, os.path.join(BIN, "ntLink"), "pair", "-B", "target=scaffolds_4.fa", "reads=long_reads_4_top5.fa", "k=40", "w=100"]
    done = subprocess.run(cmd, cwd=tmp_path, env=dict(env, NTL_INDEXLR_DEVICE_TEXT="1"), capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr
    assert read_text(str(tmp_path / "scaffolds_4.fa.k40.w100.tsv")) == read_text(os.path.join(REF, "expected_outputs", "scaffolds_4.fa.k40.w100.tsv"))


RANDOM_PARTS = 4  # 200 seeded sketches, fifty a test case (a launch of the mock takes milliseconds)


def check_random(dev, part):
    rng = np.random.default_rng(20240 + part)
    zeros = 0
    for i in range(200 // RANDOM_PARTS):
        nseq = int(rng.integers(0, 13))
        counts = np.where(rng.random(nseq) < 0.3, 0, rng.integers(1, 200, nseq) >> rng.integers(0, 8, nseq))
        zeros += int((counts == 0).sum())
        check_sketch(dev, *make(counts, seed=1000 * part + i), f"random {part}.{i}", forms=[FORMS[int(rng.integers(0, 3))]])
    assert zeros >= 50


def test_the_cases_cover_the_issue():
    assert len(U64) == 41 and sorted({len(str(v)) for v in U64}) == list(range(1, 21))
    assert len(U32) == 20 and sorted({len(str(v)) for v in U32}) == list(range(1, 11)) and max(U32) == 2 ** 32 - 1
    assert capi.NTL_SKETCH_TEXT_LEN == 1 and capi.NTL_SKETCH_TEXT_STRAND == 2
    assert pipeline.device_text_on(None) == (os.environ.get("NTL_INDEXLR_DEVICE_TEXT", "0") == "1")


CHECKS = [check_digits, check_empty_lines, check_shapes, check_refusals]


# ---------------------------------------------------------------- under the SIMT mock

@pytest.fixture(scope="module")
def sim_dev():
    from sim import simlib
    d = simlib.device()
    yield d
    d.close()


def _sim_env():
    from sim import simlib
    return dict(os.environ, NTLINK_AMD_LIB=simlib.build())


@pytest.mark.parametrize("check", CHECKS, ids=lambda c: c.__name__[6:])
def test_sim(sim_dev, check):
    check(sim_dev)


@pytest.mark.parametrize("part", range(RANDOM_PARTS))
def test_sim_random(sim_dev, part):
    check_random(sim_dev, part)


def test_sim_pieces(sim_dev, monkeypatch):
    check_pieces(sim_dev, monkeypatch)


def test_sim_goldens(sim_dev, tmp_path):
    check_goldens(sim_dev, tmp_path)


def test_sim_driver(sim_dev, tmp_path, monkeypatch):
    check_driver(sim_dev, tmp_path, monkeypatch)


@pytest.mark.parametrize("which", list(CLI_INPUTS))
def test_sim_cli(tmp_path, which):
    check_cli(tmp_path, _sim_env(), which, fastq_records=12)


def test_sim_pair_cli(tmp_path):
    check_pair_cli(tmp_path, _sim_env())


# ---------------------------------------------------------------- on the GPU

@pytest.fixture(scope="module")
def gpu_dev():
    d = capi.Device(0)
    yield d
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("check", CHECKS, ids=lambda c: c.__name__[6:])
def test_gpu(gpu_dev, check):
    check(gpu_dev)


@pytest.mark.gpu
@pytest.mark.parametrize("part", range(RANDOM_PARTS))
def test_gpu_random(gpu_dev, part):
    check_random(gpu_dev, part)


@pytest.mark.gpu
def test_gpu_pieces(gpu_dev, monkeypatch):
    check_pieces(gpu_dev, monkeypatch)


@pytest.mark.gpu
def test_gpu_goldens(gpu_dev, tmp_path):
    check_goldens(gpu_dev, tmp_path)


@pytest.mark.gpu
def test_gpu_driver(gpu_dev, tmp_path, monkeypatch):
    check_driver(gpu_dev, tmp_path, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("which", list(CLI_INPUTS))
def test_gpu_cli(tmp_path, which):
    check_cli(tmp_path, dict(os.environ), which)


@pytest.mark.gpu
def test_gpu_pair_cli(tmp_path):
    check_pair_cli(tmp_path, dict(os.environ))
