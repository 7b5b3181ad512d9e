"""ntl_mapres_liftover (csrc/liftover_kernels.h) and its Python layer -- under the SIMT mock and on the GPU, the same checks.

  golden     the 22 imported-reference cases of tests/golden/gen/liftover: liftover_mappings_device writes the committed bytes, with
             one block and with several
  crafted    records through mapres_from_host -> mapres_liftover -> download against the plain-Python restatement of the reference
             (tests/liftover_cases.py), record for record, and the same reads as text through the host's ntl_liftover: lines of 1, 63,
             64, 65 and 129 hits, the four bounds of the range filter, k longer than the component, the four modes, the run patterns,
             the joins, reads on both sides of NTL_LIFT_LANE_LINES, 255 / 256 / 257 reads, unused hit slots, an empty result
  random     300 seeded reads, which must take every branch often enough
  refusals   every NTL_EINVAL / NTL_ERANGE with its message; the two ValueErrors of the file path, with no file left
  tally      liftover_mappings_device(tally=) == the checkpoint path over the lifted file; lift_result on a mapped scenario == the file
             path on that result's own text
  cli        --device 0 gives the golden bytes"""
import gzip
import json
import os

import numpy as np
import pytest

import liftover_cases as lc
import parity_cases as pc
from helpers import ROOT
from ntlink_amd import capi, formats, liftover, pairing

GOLD = os.path.join(ROOT, "tests", "golden")
CASES = json.load(open(os.path.join(GOLD, "gen", "liftover", "cases.json")))
NO_PAFS = np.zeros(0, capi.PAF_DT)
TALLY_CASE = next(c for c in CASES if c["name"] == "syn_many_ctg_agp3")  # its lifted file makes 71 pairs


def _mappings_file(case, tmp_path):
    src = os.path.join(GOLD, case["mappings"])
    if not src.endswith(".gz"):
        return src
    dst = tmp_path / "in.verbose_mapping.tsv"
    dst.write_bytes(gzip.open(src, "rb").read())
    return str(dst)


def _golden(case):
    return gzip.open(os.path.join(GOLD, "gen", "liftover", case["name"] + ".liftover.tsv.gz"), "rb").read()


def _names_of(path, agp):
    "the AGP's ids plus whatever contig names the mappings hold beyond them"
    names, seen = list(agp), set(agp)
    with open(path) as fh:
        for line in fh:
            ctg = line.split("\t")[1]
            if ctg not in seen:
                seen.add(ctg)
                names.append(ctg)
    return names


def test_the_cases_cover_the_issue():
    assert len(CASES) == 22 and capi.NTL_LIFT_LANE_LINES == 16
    labels = [label for label, _ in lc.crafted_reads()]
    assert len(set(labels)) == len(labels)
    T = capi.NTL_LIFT_LANE_LINES
    for want in ["1-hits-shift", "63-hits-mirror", "64-hits-shift", "65-hits-every-other-kept", "129-hits-mirror", "bounds", "k-longer-than-component",
                 "mode0", "mode1-minus", "equal-positions", "single-hit", "all-filtered", "A-B-A", "A-X-A", "X-A-X", "X1-A-X2", "A-B-A-B", "A-B-A-C-A",
                 "A-A-B", "three-lines-broken-join"] + [f"{n}-lines-one-group" for n in (1, 2, T - 1, T, T + 1)]:
        assert want in labels, want
    # the restatement itself, by hand
    by = dict(lc.crafted_reads())
    lift = lambda label: lc.lift_read(by[label], lc.AGP, lc.K)
    assert lift("bounds") == [("A", [(2200, 1, 2, 1), (3168, 0, 3, 1)])]
    assert lift("1-hits-mirror") == [("A", [(1100 + 900 - 32, 1, 7, 1)])]  # inc(cs=2) starts with strand 0: flipped
    assert lift("mode1-minus") == [("keep1", [(100, 1, 2, 1), (500, 0, 3, 0), (868, 1, 4, 1)])]
    assert lift("A-B-A") == [("A", lc.inc(3) + [(2290, 1, 7, 1), (2293, 1, 12, 1), (2296, 1, 17, 1)])]
    assert lift("X-A-X") == [] and lift("A-B-A-B") == [] and lift("A-B-A-C-A") == [] and lift("mode0") == [] and lift("k-longer-than-component") == []
    assert [n for n, _ in lift("X1-A-X2")] == ["A"] and [n for n, _ in lift("A-A-B")] == ["A", "B"]
    assert lift("equal-positions") == [] and lift("three-lines-broken-join") == [] and len(lift("three-lines-increasing")[0][1]) == 6
    assert len(lift("three-lines-decreasing")[0][1]) == 5 and lift("A-B-B-A-C") == [("A", [(100, 1, 100, 1), (200, 1, 200, 1)]), ("C", [(5017, 0, 1, 1)])]  # 50 + (5000 - 1) - 32
    assert len(lift(f"{T + 1}-lines-one-group")[0][1]) == T + 1 and lift(f"{T + 1}-lines-B-A..A-B") == [("B", [(100, 1, 1, 1), (200, 1, 2, 1)])]


# ---------------------------------------------------------------- the checks (the same for the mock and the GPU)

def check_golden(dev, case, tmp_path, blocks):
    agp = liftover.read_agp(os.path.join(GOLD, case["agp"]))
    path = _mappings_file(case, tmp_path)
    max_bytes = os.path.getsize(path) // 3 if blocks else None  # three or four blocks
    out = tmp_path / "lifted.tsv"
    kw = {} if max_bytes is None else {"max_bytes": max_bytes}
    nin, nout = liftover.liftover_mappings_device(path, agp, str(out), case["k"], dev, contig_names=_names_of(path, agp), **kw)
    exp = _golden(case)
    assert out.read_bytes() == exp
    assert nout == case["lines"] == exp.count(b"\n") and nin == sum(1 for _ in open(path))
    assert [f for f in os.listdir(tmp_path) if ".tmp" in f] == []
    if max_bytes is not None:
        assert len(list(formats.read_verbose(path, list(agp), max_bytes=max_bytes, lib_path=dev.lib_path))) > 1, "several blocks"


def check_records(dev, reads, tmp_path, label, gaps=lc.GAPS):
    """device records == the restatement, record for record; the host's ntl_liftover on the same reads as text == the same lines"""
    table, out_names = liftover.lift_table(lc.AGP, lc.CONTIGS)
    maps, slots = lc.build(reads, gaps=gaps)
    exp_maps, exp_hits = lc.expected(reads, out_names)
    with dev.mapres_from_host(maps, slots, NO_PAFS) as res:
        with dev.mapres_liftover(res, table, lc.K) as lifted:
            assert isinstance(lifted, capi.MapResult)
            assert lifted.counts() == (len(exp_maps), len(exp_hits), 0), label
            assert lifted.n_index_hits == 0
            got = lifted.download()
        again = res.download()  # the input is left alone
    assert np.array_equal(got["maps"], exp_maps), f"{label}: mappings"
    assert np.array_equal(got["hits"], exp_hits), f"{label}: hits"
    assert len(again["maps"]) == len(maps) and int(again["maps"]["n_hits"].sum()) == int(maps["n_hits"].sum())
    read_names = [f"r{i}" for i in range(len(reads))]
    src, out = tmp_path / "crafted.tsv", tmp_path / "crafted.lifted.tsv"
    src.write_text(lc.verbose_text(reads, read_names))
    liftover.liftover_mappings(str(src), lc.AGP, str(out), lc.K)
    assert out.read_text() == lc.records_text(exp_maps, exp_hits, read_names, out_names), f"{label}: the host path"
    return got


def check_crafted(dev, tmp_path):
    crafted = lc.crafted_reads()
    got = check_records(dev, [lines for _, lines in crafted], tmp_path, "crafted")
    assert len(got["maps"]) > 40
    # every read on its own result as well: a first and a last line of the whole array, no neighbour
    for label in ("A-B-A", "X-A-X", "129-hits-mirror", f"{lc.LANE_LINES + 1}-lines-B-A..A-B", "all-filtered"):
        check_records(dev, [dict(crafted)[label]], tmp_path, label, gaps=(0,))


def check_shapes(dev, tmp_path):
    for n in (255, 256, 257):
        reads = [[("a1", [(100 + i, 1, i, 1)])] + ([("b1", [(5, 0, 1, 0)]), ("a3", [(700, 1, 2, 1)])] if i % 5 == 0 else []) for i in range(n)]
        got = check_records(dev, reads, tmp_path, f"{n} reads")
        assert len(np.unique(got["maps"]["read"])) == n
    # an empty result, with and without slots; a result whose every hit goes
    table, _ = liftover.lift_table(lc.AGP, lc.CONTIGS)
    for slots in (np.zeros(0, capi.HIT_DT), np.zeros(9, capi.HIT_DT)):
        with dev.mapres_from_host(np.zeros(0, capi.MAPPING_DT), slots, NO_PAFS) as res, dev.mapres_liftover(res, table, lc.K) as lifted:
            assert lifted.counts() == (0, 0, 0)
            d = lifted.download()
            assert len(d["maps"]) == 0 and len(d["hits"]) == 0
    check_records(dev, [[("x1", lc.inc(3))], [("short", lc.inc(2))]], tmp_path, "nothing stays")


def check_random(dev, tmp_path):
    reads = lc.random_reads()
    assert len(reads) == 300
    check_records(dev, reads, tmp_path, "random")
    # what the generator must have produced, from the host path's output (check_records has held it to the restatement)
    printed = {line.split("\t")[0] for line in (tmp_path / "crafted.lifted.tsv").read_text().splitlines()}
    events = set()
    for lines in reads:
        lc.lift_read(lines, lc.AGP, lc.K, events)
    assert len(printed) >= len(reads) / 3 and len(reads) - len(printed) >= len(reads) / 10 and events == {"subsumed", "mirror", "non-monotonic"}, \
        f"uninformative: {len(printed)} of {len(reads)} reads print a line, events {sorted(events)}"


def check_refusals(dev, tmp_path):
    hit = np.array([(10, 1, 1, 1, (0, 0))], capi.HIT_DT)
    entry = lambda *e: np.array([e], capi.LIFT_ENTRY_DT)
    good = entry(0, 2, 1, 1, 1000)

    def refused(ctg, table, k, code, message):
        with dev.mapres_from_host(np.array([(0, ctg, 1, 0, 0)], capi.MAPPING_DT), hit, NO_PAFS) as res:
            with pytest.raises(capi.NtlError, match=message) as ei:
                dev.mapres_liftover(res, table, k)
            assert ei.value.code == code, message
            assert res.counts() == (1, 1, 0)  # ... and the input is still good
    refused(1, good, 32, capi.NTL_EINVAL, "names a contig that the table does not hold")
    refused(capi.NO_CTG, good, 32, capi.NTL_EINVAL, "names a contig that the table does not hold")
    refused(0, np.zeros(0, capi.LIFT_ENTRY_DT), 32, capi.NTL_EINVAL, "names a contig that the table does not hold")
    refused(0, entry(0, 4, 1, 1, 1000), 32, capi.NTL_EINVAL, "table entry 0 has mode 4")
    for mode in (1, 2, 3):
        refused(0, entry(0, mode, 0, 1, 1000), 32, capi.NTL_EINVAL, "table entry 0 has a start of 0")
        refused(0, entry(0, mode, 1, 0, 1000), 32, capi.NTL_EINVAL, "table entry 0 has a start of 0")
        refused(0, entry(0, mode, 1, 11, 10), 32, capi.NTL_EINVAL, "table entry 0 ends in front of its start")
    refused(0, good, 0, capi.NTL_EINVAL, "k must be at least 1")
    refused(0, good, -3, capi.NTL_EINVAL, "k must be at least 1")
    refused(0, entry(0, 2, 2 ** 32 - 1, 1, 1000), 32, capi.NTL_ERANGE, "does not fit 32 bits")      # 2^32 - 2 + 10
    refused(0, entry(0, 3, 2 ** 32 - 1, 1, 1000), 32, capi.NTL_ERANGE, "does not fit 32 bits")
    # accepted at the edges: a mode-0 entry of zeros; the largest position that fits
    with dev.mapres_from_host(np.array([(0, 0, 1, 0, 0)], capi.MAPPING_DT), hit, NO_PAFS) as res:
        with dev.mapres_liftover(res, entry(0, 0, 0, 0, 0), 32) as lifted:
            assert lifted.counts() == (0, 0, 0)
        with dev.mapres_liftover(res, entry(0, 2, 2 ** 32 - 10, 1, 1000), 32) as lifted:
            assert lifted.download()["hits"]["ctg_pos"].tolist() == [2 ** 32 - 1]
    dev.sync()
    # the file path
    out = tmp_path / "o.tsv"
    src = tmp_path / "in.tsv"
    src.write_text("r1\ta1\t1\t100:+_5:+\nr1\tnowhere7\t1\t100:+_5:+\n")
    with pytest.raises(ValueError, match="nowhere7"):
        liftover.liftover_mappings_device(str(src), lc.AGP, str(out), 32, dev)
    assert os.listdir(tmp_path) == ["in.tsv"]
    assert liftover.liftover_mappings_device(str(src), lc.AGP, str(out), 32, dev, contig_names=list(lc.AGP) + ["nowhere7"]) == (2, 1)
    assert out.read_text() == "r1\tA\t1\t100:+_5:+\n"
    os.remove(out)
    for bad in ("r1\ta1\t1\t100:+_x:+\n", "r1\ta1\t1\t100:+_5\n", "r1\tx1\t1\tgarbage\n", "r1\ta1\t2\n"):
        src.write_text("r0\ta1\t1\t100:+_5:+\n" + bad)
        with pytest.raises(ValueError):
            liftover.liftover_mappings_device(str(src), lc.AGP, str(out), 32, dev, contig_names=lc.CONTIGS, max_bytes=10)
        assert os.listdir(tmp_path) == ["in.tsv"], bad
    src.write_text("")
    assert liftover.liftover_mappings_device(str(src), lc.AGP, str(out), 32, dev) == (0, 0) and out.read_bytes() == b""


def _scaffold_lengths(agp_path, out_names):
    length = {}
    for line in open(agp_path):
        cols = line.rstrip("\n").split("\t")
        length[cols[0]] = max(length.get(cols[0], 0), int(cols[2]))
    return np.array([length.get(n, 1) for n in out_names], np.uint32)


def check_tally(dev, case, tmp_path):
    agp_path = os.path.join(GOLD, case["agp"])
    agp = liftover.read_agp(agp_path)
    path = _mappings_file(case, tmp_path)
    names = _names_of(path, agp)
    _table, out_names = liftover.lift_table(agp, names)
    ctg_len = _scaffold_lengths(agp_path, out_names)
    handed = pairing.PairTally(out_names, ctg_len, case["k"], 10)
    out = tmp_path / "lifted.tsv"
    liftover.liftover_mappings_device(path, agp, str(out), case["k"], dev, contig_names=names, tally=handed, max_bytes=20000)
    assert out.read_bytes() == _golden(case)
    reread = pairing.PairTally(out_names, ctg_len, case["k"], 10)
    index_of = {n: i for i, n in enumerate(out_names)}
    with open(out) as fh:
        for _read, entries in formats.parse_verbose(fh):
            reread.add_checkpoint_read(entries, index_of)
    a, b = handed.export(), reread.export()
    assert len(a[0]) > 5, "the case makes pairs"
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def check_lift_result(dev, tmp_path, scenario="syn_default"):
    """a result of the mapper, lifted where it is == the file path over that result's own lines"""
    meta, _exp, arrs, kw, rn = pc.scenario_arrays(scenario)
    case = next(c for c in CASES if c["name"] == scenario + "_agp1")
    agp = liftover.read_agp(os.path.join(GOLD, case["agp"]))
    ctg_names = meta["ctg_names"]
    coff, ch, cp, cs, ctg_len, roff, rlen, rh, rp, rs = arrs
    with dev.sketch_from_arrays(coff, ch, cp, cs) as csk, dev.index(csk, ctg_len) as ix, dev.sketch_from_arrays(roff, rh, rp, rs) as rsk, \
            dev.map(ix, rsk, rlen, **kw) as res, dev.names(rn, rlen) as rnames:
        lifted, out_names = liftover.lift_result(res, agp, ctg_names, case["k"], dev)  # (the result is still pending here)
        with lifted, dev.names(out_names, np.zeros(len(out_names), np.uint32)) as onames, lifted.format(rnames, onames, True, False) as text:
            d = text.download()
            got = bytes(d["verbose"])
            dev.pinned_release(d["_pinned"])
        with dev.names(ctg_names, ctg_len) as cnames, res.format(rnames, cnames, True, False) as text:
            d = text.download()
            own = bytes(d["verbose"])
            dev.pinned_release(d["_pinned"])
    src, out = tmp_path / "own.tsv", tmp_path / "own.lifted.tsv"
    src.write_bytes(own)
    liftover.liftover_mappings_device(str(src), agp, str(out), case["k"], dev, contig_names=ctg_names)
    assert got == out.read_bytes() and got.count(b"\n") > 20
    if own == gzip.open(os.path.join(GOLD, case["mappings"]), "rb").read():  # the scenario's committed lines: then the committed liftover
        assert got == _golden(case)


def check_cli(case, tmp_path, lib_path=None):
    import subprocess
    import sys
    out = tmp_path / "cli.tsv"
    path = _mappings_file(case, tmp_path)
    env = dict(os.environ)
    if lib_path:
        env["NTLINK_AMD_LIB"] = lib_path
    fasta = tmp_path / "contigs.fa"
    agp = liftover.read_agp(os.path.join(GOLD, case["agp"]))
    fasta.write_text("".join(f">{n}\nACGT\n" for n in _names_of(path, agp)))
    rc = subprocess.call([sys.executable, os.path.join(ROOT, "bin", "ntlink_liftover_mappings.py"), "-m", path, "-a", os.path.join(GOLD, case["agp"]),
                          "-o", str(out), "-k", str(case["k"]), "--device", "0", "--contigs", str(fasta)], env=env)
    assert rc == 0
    assert out.read_bytes() == _golden(case)


# ---------------------------------------------------------------- under the SIMT mock

@pytest.fixture(scope="module")
def sim_dev():
    from sim import simlib
    d = simlib.device()
    yield d
    d.close()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
@pytest.mark.parametrize("blocks", [False, True], ids=["one-block", "blocks"])
def test_sim_golden(sim_dev, case, blocks, tmp_path):
    check_golden(sim_dev, case, tmp_path, blocks)


def test_sim_crafted(sim_dev, tmp_path):
    check_crafted(sim_dev, tmp_path)


def test_sim_shapes(sim_dev, tmp_path):
    check_shapes(sim_dev, tmp_path)


def test_sim_random(sim_dev, tmp_path):
    check_random(sim_dev, tmp_path)


def test_sim_refusals(sim_dev, tmp_path):
    check_refusals(sim_dev, tmp_path)


def test_sim_tally(sim_dev, tmp_path):
    check_tally(sim_dev, TALLY_CASE, tmp_path)


def test_sim_lift_result(sim_dev, tmp_path):
    check_lift_result(sim_dev, tmp_path)


def test_sim_cli(tmp_path):
    from sim import simlib
    check_cli(CASES[0], tmp_path, simlib.build())


# ---------------------------------------------------------------- on the GPU

@pytest.fixture(scope="module")
def gpu_dev():
    d = capi.Device(0)
    yield d
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
@pytest.mark.parametrize("blocks", [False, True], ids=["one-block", "blocks"])
def test_gpu_golden(gpu_dev, case, blocks, tmp_path):
    check_golden(gpu_dev, case, tmp_path, blocks)


@pytest.mark.gpu
def test_gpu_crafted(gpu_dev, tmp_path):
    check_crafted(gpu_dev, tmp_path)


@pytest.mark.gpu
def test_gpu_shapes(gpu_dev, tmp_path):
    check_shapes(gpu_dev, tmp_path)


@pytest.mark.gpu
def test_gpu_random(gpu_dev, tmp_path):
    check_random(gpu_dev, tmp_path)


@pytest.mark.gpu
def test_gpu_refusals(gpu_dev, tmp_path):
    check_refusals(gpu_dev, tmp_path)


@pytest.mark.gpu
def test_gpu_tally(gpu_dev, tmp_path):
    check_tally(gpu_dev, TALLY_CASE, tmp_path)


@pytest.mark.gpu
def test_gpu_lift_result(gpu_dev, tmp_path):
    check_lift_result(gpu_dev, tmp_path)


@pytest.mark.gpu
def test_gpu_cli(tmp_path):
    check_cli(CASES[0], tmp_path)
