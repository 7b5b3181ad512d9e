"""ntl_mapres_pairs (csrc/pair_kernels.h), ntl_tally_add_pairs and their Python layer -- under the SIMT mock and on the GPU, the same checks.

Every device check holds PairTally.export() after add_pairs(mapres_pairs(...)) against the export after add_batch on the downloaded
result -- all seven arrays -- and the records themselves against the plain-Python restatement of the rules (tests/pair_cases.py).

  restatement  the restatement against the host tally alone, crafted and random (no device)
  counts       reads of 0 .. 3 mappings, m = f - 1, f, f + 1 for f = 3 and 10, f = 0 and 1
  chains       the second list: nothing added, added, two weak in a row, a dropped neighbour that returns, A B A B, A A B, equal names
  strands      the four strand combinations of either side, on both sides of the swap
  bounds       |gap| == read length kept, + 1 dropped; overhangs of 0; -1 refused with nothing added; -1 outside every pair accepted
  shapes       reads around NTL_PAIR_LANE_MAPS, 130 mappings, 63 .. 65 and 255 .. 257 reads, empty results, unused slots, a read alone
  read length  the array; None against PairTally.add_checkpoint_read
  random       300 seeded reads that take every branch at least ten times
  refusals     every NTL_EINVAL with its message; add_pairs with a bad index or orientation
  fixtures     the checkpoint tally of test 4; run_pair(device_tally=True) with and without text; the liftover hand-over"""
import collections
import os
import shutil

import numpy as np
import pytest

import pair_cases as pc
from helpers import FIXTURES, GEN, REF, read_text
from ntlink_amd import capi, formats, liftover, pairing, pipeline, seqio

NO_PAFS = np.zeros(0, capi.PAF_DT)
GAPS = (3, 0, 1, 64, 0, 7, 2)


def _tally(contigs, k, f):
    return pairing.PairTally([n for n, _ in contigs], np.array([l for _, l in contigs], np.uint32), k, f)


def _same_export(a, b, label):
    for name, x, y in zip(("src", "src_ori", "tgt", "tgt_ori", "anchor", "gap_off", "gaps"), a, b):
        assert x.dtype == y.dtype and np.array_equal(x, y), f"{label}: {name}"


def _host_tally(reads, contigs, k, f, read_ids=None):
    "the host tally over the same records, dense"
    maps, hits = pc.build(reads, read_ids=read_ids)
    t = _tally(contigs, k, f)
    t.add_batch({"maps": maps, "hits": hits}, pc.read_lengths(reads, read_ids))
    return t


# ---------------------------------------------------------------- the restatement against the host tally (no device)

def _all_crafted():
    for f in (0, 1, 3, 10):
        yield f"counts f={f}", pc.count_reads(f), f
    yield "chains", [r for _l, r in pc.chain_reads()], 1
    yield "strands", pc.strand_reads(), 10
    yield "strands as chains", pc.strand_reads(), 1
    yield "bounds", pc.bound_reads(), 10
    yield "bounds as chains", pc.bound_reads(), 0
    yield "launch f=10", pc.launch_reads(), 10
    yield "launch f=200", pc.launch_reads(), 200
    yield "random", pc.random_reads(), pc.RANDOM_F


def test_restatement_is_the_host_tally():
    for label, reads, f in _all_crafted():
        recs = pc.records(reads, pc.CONTIGS, pc.K, f)
        _same_export(pc.export_of(recs, pc.CONTIGS), _host_tally(reads, pc.CONTIGS, pc.K, f).export(), label)
    for label, reads in pc.negative_reads().items():
        for f in (10, 1):
            with pytest.raises(pc.Negative):
                pc.records(reads, pc.CONTIGS, pc.K, f)
            with pytest.raises(AssertionError, match="Gap distance estimation less than 0"):
                _host_tally(reads, pc.CONTIGS, pc.K, f)


def test_the_cases_cover_the_issue():
    assert capi.NTL_PAIR_LANE_MAPS == 16 and capi.PAIR_REC_DT.itemsize == 24
    by = dict(pc.chain_reads())
    rec = lambda label, f=1: [tuple(r)[:7] for r in pc.records([by[label]], pc.CONTIGS, pc.K, f).tolist()]
    names = lambda label: [(pc.CONTIGS[r[0]][0], pc.CONTIGS[r[1]][0], r[6]) for r in rec(label)]
    assert names("all-strong") == [("ctg1", "ctg10", 1), ("b", "ctg1", 1), ("a", "b", 1), ("a", "z", 1)]  # (z as a source overhangs by 99 kb: dropped)
    assert names("strong-weak-strong") == [("ctg1", "ctg10", 0), ("b", "ctg1", 0), ("b", "ctg10", 1)]          # (A, B) from the second list
    assert names("two-weak-in-a-row") == [("ctg1", "ctg10", 0), ("a", "ctg1", 0), ("a", "b", 0), ("b", "ctg10", 1)]
    assert rec("dropped-neighbour-returns") == [(pc.B, pc.C1, 600 - 40 - (5000 - 140 - 32) - 100, 0, 0, 0, 1)]  # (1, 2) alone; swapped, both flipped
    assert rec("dropped-strong-pair-over-weak") == [(pc.A, pc.C10, 400 - 140 - (5000 - 140 - 32) - 100, 0, 0, 0, 0)]
    assert len(rec("A-B-A-B")) == 4 and len(rec("A-B-A-B-weak-middle")) == 3 and len(rec("A-weakA-B")) == 2 and len(rec("A-A-B")) == 2
    assert names("dup-weak-dup") == [("dup", "dup", 0), ("dup", "dup", 0)]  # equal names swap: (0, 2) has the key of (0, 1)
    ev = collections.Counter()
    pc.records([by["A-B-A-B-weak-middle"], by["dropped-neighbour-returns"]], pc.CONTIGS, pc.K, 1, events=ev)
    assert ev["skipped"] == 2 and ev["dropped"] == 2  # (the recorded neighbour (1, 2) comes back too, and is skipped by its key)
    # bounds: kept, dropped, kept, dropped, kept; the overhangs of 1; the lone mapping
    assert [len(pc.records([r], pc.CONTIGS, pc.K, 10)) for r in pc.bound_reads()] == [1, 0, 1, 0, 1, 1, 0]
    assert pc.records(pc.bound_reads()[:1], pc.CONTIGS, pc.K, 10)["gap"].tolist() == [1000]
    # the random set takes every branch often enough (the seed is chosen for it)
    ev = collections.Counter()
    assert len(pc.random_reads()) == 300
    pc.records(pc.random_reads(), pc.CONTIGS, pc.K, pc.RANDOM_F, events=ev)
    assert min(ev[key] for key in ("short", "chain", "swapped", "dropped", "skipped")) >= 10, dict(ev)


def test_add_pairs_refusals():
    t = _tally(pc.CONTIGS, pc.K, 10)
    good = (0, 1, 5, 0, 1, 1, 1, 0)
    for bad in ((len(pc.CONTIGS), 1, 5, 0, 1, 1, 1, 0), (0, len(pc.CONTIGS), 5, 0, 1, 1, 1, 0), (0, 1, 5, 0, 2, 1, 1, 0), (0, 1, 5, 0, 1, 2, 1, 0)):
        with pytest.raises(ValueError, match="ntl_tally_add_pairs failed with -1"):
            t.add_pairs(np.array([good, bad], capi.PAIR_REC_DT))
        assert len(t.export()[0]) == 0  # nothing added, the good record in front included
    t.add_pairs(np.zeros(0, capi.PAIR_REC_DT))
    t.add_pairs(np.array([good, good], capi.PAIR_REC_DT))
    assert t.pairs == {("ctg10", "+", "ctg1", "+"): [[5, 5], 2]}  # (the records are taken as they are: normalising is the device's part)


# ---------------------------------------------------------------- the checks (the same for the mock and the GPU)

def check_reads(dev, reads, f, label, contigs=pc.CONTIGS, k=pc.K, explicit=True, gaps=GAPS, tail=5, read_ids=None):
    maps, slots = pc.build(reads, gaps=gaps, tail=tail, read_ids=read_ids)
    rl = pc.read_lengths(reads, read_ids)
    host, devt = _tally(contigs, k, f), _tally(contigs, k, f)
    with dev.mapres_from_host(maps, slots, NO_PAFS) as res, dev.pair_table(devt) as tab:
        recs = dev.mapres_pairs(res, tab, rl if explicit else None)
        down = res.download()  # the result is left alone
    assert recs.dtype == capi.PAIR_REC_DT
    exp = pc.records(reads, contigs, k, f, explicit, read_ids)
    assert np.array_equal(recs, exp), f"{label}: records"
    if explicit:
        host.add_batch(down, rl)
    elif len({n for n, _l in contigs}) == len(contigs):  # the checkpoint path, read by read (it finds a contig by its name)
        index_of = {n: i for i, (n, _l) in enumerate(contigs)}
        for _rl, lines in reads:
            if lines:
                host.add_checkpoint_read([(contigs[c][0], hits) for c, hits in lines], index_of)
    else:  # its rule, spelled out
        host.add_batch(down, pc.read_lengths([(max(max(h[0][2], h[-1][2]) for _c, h in lines) if lines else 0, lines) for _rl, lines in reads], read_ids))
    devt.add_pairs(recs)
    _same_export(devt.export(), host.export(), label)
    return recs


def check_counts(dev):
    for f in (0, 1, 3, 10):
        assert len(check_reads(dev, pc.count_reads(f), f, f"counts f={f}")) > 0


def check_chains(dev):
    crafted = pc.chain_reads()
    check_reads(dev, [r for _l, r in crafted], 1, "chains")
    for label, read in crafted:  # alone in a result: a first and a last line of the whole array, no neighbour
        check_reads(dev, [read], 1, label, gaps=(0,), tail=0)
    check_reads(dev, pc.strand_reads(), 10, "strands")
    check_reads(dev, pc.strand_reads(), 1, "strands as chains")


def check_bounds(dev):
    assert len(check_reads(dev, pc.bound_reads(), 10, "bounds")) == 4
    assert len(check_reads(dev, pc.bound_reads(), 0, "bounds as chains")) == 4
    for label, reads in pc.negative_reads().items():
        for f in (10, 1):
            maps, slots = pc.build(reads)
            t = _tally(pc.CONTIGS, pc.K, f)
            with dev.mapres_from_host(maps, slots, NO_PAFS) as res, dev.pair_table(t) as tab:
                with pytest.raises(capi.NtlError, match="Gap distance estimation less than 0") as ei:
                    dev.mapres_pairs(res, tab, pc.read_lengths(reads))
                assert ei.value.code == capi.NTL_ERANGE, label
                assert res.counts()[0] == len(maps)
            assert len(t.export()[0]) == 0, label  # no partial result: nothing could be added


def check_shapes(dev):
    check_reads(dev, pc.launch_reads(), 10, "launch f=10")
    check_reads(dev, pc.launch_reads(), 200, "launch f=200")  # reads of 130 in the first branch: 8385 pairs each, by a wavefront
    for read in pc.launch_reads()[2:5]:
        check_reads(dev, [read], 10, "a long read alone", gaps=(0,), tail=0)
    for n in (63, 64, 65, 255, 256, 257):
        recs = check_reads(dev, pc.many_reads(n), 10, f"{n} reads")
        assert len(np.unique(recs["read"])) == n
    check_reads(dev, pc.many_reads(40), 10, "read numbers with holes", read_ids=[3 * i + 1 for i in range(40)])
    for slots in (0, 9):  # an empty result, with and without slots
        assert len(check_reads(dev, [], 10, "empty", tail=slots)) == 0
        assert len(check_reads(dev, [], 10, "empty", tail=slots, explicit=False)) == 0
    assert len(check_reads(dev, [(100, [pc.mp(pc.B, 5)])], 10, "one mapping")) == 0


def check_read_length(dev):
    unique = [c for i, c in enumerate(pc.CONTIGS) if i != pc.DUP2]  # add_checkpoint_read finds contigs by name
    reads = [(rl, [(c if c < pc.DUP2 else c - 1, hits) for c, hits in lines if c != pc.DUP2]) for rl, lines in pc.random_reads(seed=11, n_reads=120)]
    for f in (3, 10):
        a = check_reads(dev, reads, f, "checkpoint rule", contigs=unique, explicit=False)
        b = check_reads(dev, reads, f, "the array", contigs=unique)
        assert 0 < len(a) != len(b)  # the rule matters on this set
    check_reads(dev, pc.launch_reads(), 10, "checkpoint rule, by a wavefront", explicit=False)
    check_reads(dev, pc.bound_reads(5000), 10, "checkpoint rule, one hit a mapping", explicit=False)


def check_random(dev):
    check_reads(dev, pc.random_reads(), pc.RANDOM_F, "random")


def check_refusals(dev, grouped=None):
    hit = np.array([(10, 1, 1, 1, (0, 0))] * 2, capi.HIT_DT)
    t = _tally(pc.CONTIGS, pc.K, 10)

    def refused(maps, read_len, message):
        with dev.mapres_from_host(np.array(maps, capi.MAPPING_DT), hit, NO_PAFS) as res, dev.pair_table(t) as tab:
            with pytest.raises(capi.NtlError, match=message) as ei:
                dev.mapres_pairs(res, tab, read_len)
            assert ei.value.code == capi.NTL_EINVAL, message
            assert res.counts() == (len(maps), len(maps), 0)  # ... and the input is still good
    n = len(pc.CONTIGS)
    refused([(0, 0, 1, 0, 0), (0, n, 1, 0, 1)], [100], "names a contig that the table does not hold")
    refused([(0, capi.NO_CTG, 1, 0, 0)], None, "names a contig that the table does not hold")
    refused([(0, 0, 1, 0, 0), (1, 1, 1, 0, 1)], [100], "names a read that read_len does not hold")
    refused([(7, 0, 1, 0, 0)], np.zeros(0, np.uint32), "names a read that read_len does not hold")
    with dev.mapres_from_host(np.array([(0, 0, 1, 0, 0), (1, 1, 1, 0, 1)], capi.MAPPING_DT), hit, NO_PAFS) as res, dev.pair_table(t) as tab:
        assert len(dev.mapres_pairs(res, tab, None)) == 0   # without the array a read number is only a number
        assert len(dev.mapres_pairs(res, tab, [5, 5])) == 0
    if grouped is not None:
        with grouped() as res, dev.pair_table(t) as tab:
            with pytest.raises(capi.NtlError, match="a grouped result has no pair tally") as ei:
                dev.mapres_pairs(res, tab, None)
            assert ei.value.code == capi.NTL_EINVAL
    dev.sync()


def _grouped_result(dev):
    "a (tiny) result of map_grouped: one group of two contigs and one read, from sketches made of arrays"
    off = np.array([0, 1, 2], np.uint64)
    csk = dev.sketch_from_arrays(off, np.array([11, 12], np.uint64), np.array([5, 6], np.uint32), np.array([1, 1], np.uint8))
    rsk = dev.sketch_from_arrays(off[:2], np.array([11], np.uint64), np.array([3], np.uint32), np.array([1], np.uint8))
    try:
        return dev.map_grouped(csk, [2000, 2000], [0, 2], rsk, [3000], [0, 1], k=pc.K, z=1)
    finally:
        csk.close()
        rsk.close()


def check_checkpoint_fixture(dev, tmp_path):
    "test 4's verbose mapping, re-tallied from records that are resident: the committed checkpoint pairs"
    ctg = seqio.load_all([os.path.join(REF, "scaffolds_4.fa")])
    names = ctg.names.tolist()
    t = pairing.PairTally(names, ctg.lengths, 40, 10)
    with dev.pair_table(t) as tab:
        for block in formats.read_verbose(os.path.join(GEN, "fixtures", "t4_k40_w100.verbose_mapping.tsv"), names, max_bytes=20000, lib_path=dev.lib_path):
            with dev.mapres_from_host(block.maps, block.hits, NO_PAFS) as res:
                t.add_pairs(dev.mapres_pairs(res, tab, None))
    pipeline.finish_pairs(t, str(tmp_path / "out"), 1, 1, True)
    assert (tmp_path / "out.pairs.tsv").read_bytes() == open(os.path.join(GEN, "fixtures", "t4_k40_w100.checkpoint.pairs.tsv"), "rb").read()


def check_driver(dev, tmp_path, monkeypatch, tag, target, reads, k, w):
    """run_pair(device_tally=True) leaves the files of run_pair as it stands, with text and without; without, nothing is formatted"""
    for n in (target, reads):
        shutil.copy(os.path.join(REF, n), tmp_path / n)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("NTL_DEVICE_STREAMS", "1")  # one context: its events are all there is
    fixture = os.path.join(GEN, "fixtures", tag)
    pipeline.run_pair(dev, target, reads, k=k, w=w, paf=True, verbose=True, pairs_tsv=True, prefix="host", write_contig_tsv=False)
    dot = read_text("host.n1.scaffold.dot")
    assert read_text("host.pairs.tsv") == read_text(fixture + ".pairs.tsv")
    pipeline.run_pair(dev, target, reads, k=k, w=w, paf=True, verbose=True, pairs_tsv=True, prefix="text", write_contig_tsv=False, device_tally=True)
    for ext in (".verbose_mapping.tsv", ".paf", ".pairs.tsv"):
        assert read_text("text" + ext) == read_text(fixture + ext), ext
    assert read_text("text.n1.scaffold.dot") == dot
    dev.prof_enable(True)
    dev.prof_reset()
    try:
        monkeypatch.setenv("NTL_DEVICE_TALLY", "1")  # None reads the switch
        st = pipeline.run_pair(dev, target, reads, k=k, w=w, paf=False, verbose=False, pairs_tsv=True, prefix="bare", write_contig_tsv=False)
        dev.sync()
        assert dev.prof_get("format")[1] == 0 and dev.prof_get("pairs")[1] >= 1
    finally:
        dev.prof_enable(False)
    assert st["reads"] > 0 and st["t_tally"] > 0
    assert read_text("bare.pairs.tsv") == read_text(fixture + ".pairs.tsv") and read_text("bare.n1.scaffold.dot") == dot
    assert not os.path.exists("bare.verbose_mapping.tsv") and not os.path.exists("bare.paf")


def check_liftover(dev, tmp_path):
    import test_liftover_device as tl
    case = tl.TALLY_CASE
    agp_path = os.path.join(tl.GOLD, case["agp"])
    agp = liftover.read_agp(agp_path)
    path = tl._mappings_file(case, tmp_path)
    names = tl._names_of(path, agp)
    _table, out_names = liftover.lift_table(agp, names)
    ctg_len = tl._scaffold_lengths(agp_path, out_names)
    exports = []
    for on in (False, True):
        t = pairing.PairTally(out_names, ctg_len, case["k"], 10)
        out = tmp_path / f"lifted{int(on)}.tsv"
        liftover.liftover_mappings_device(path, agp, str(out), case["k"], dev, contig_names=names, tally=t, max_bytes=20000, device_tally=on)
        assert out.read_bytes() == tl._golden(case)
        exports.append(t.export())
    assert len(exports[0][0]) > 5, "the case makes pairs"
    _same_export(exports[1], exports[0], "liftover")


CHECKS = [check_counts, check_chains, check_bounds, check_shapes, check_read_length, check_random]


# ---------------------------------------------------------------- under the SIMT mock

@pytest.fixture(scope="module")
def sim_dev():
    from sim import simlib
    d = simlib.device()
    yield d
    d.close()


@pytest.mark.parametrize("check", CHECKS, ids=lambda c: c.__name__[6:])
def test_sim(sim_dev, check):
    check(sim_dev)


def test_sim_refusals(sim_dev):
    check_refusals(sim_dev, lambda: _grouped_result(sim_dev))


def test_sim_checkpoint_fixture(sim_dev, tmp_path):
    check_checkpoint_fixture(sim_dev, tmp_path)


def test_sim_driver_top5(sim_dev, tmp_path, monkeypatch):
    check_driver(sim_dev, tmp_path, monkeypatch, "t7_top5_k40_w100", "scaffolds_4.fa", "long_reads_4_top5.fa", 40, 100)


def test_sim_liftover(sim_dev, tmp_path):
    check_liftover(sim_dev, tmp_path)


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
def test_gpu_refusals(gpu_dev):
    check_refusals(gpu_dev, lambda: _grouped_result(gpu_dev))


@pytest.mark.gpu
def test_gpu_checkpoint_fixture(gpu_dev, tmp_path):
    check_checkpoint_fixture(gpu_dev, tmp_path)


@pytest.mark.gpu
@pytest.mark.parametrize("tag,target,reads,k,w,gold", FIXTURES[:4], ids=[f[0] for f in FIXTURES[:4]])
def test_gpu_driver(gpu_dev, tmp_path, monkeypatch, tag, target, reads, k, w, gold):
    check_driver(gpu_dev, tmp_path, monkeypatch, tag, target, reads, k, w)
    exp = os.path.join(REF, "expected_outputs", gold + ".z1000")
    assert read_text("bare.pairs.tsv") == read_text(exp + ".pairs.tsv")
    got, ref = read_text("bare.n1.scaffold.dot").splitlines(), read_text(exp + ".n1.scaffold.dot").splitlines()
    assert got[:2] == ref[:2] and [l for l in got if "->" in l] == [l for l in ref if "->" in l]  # (the reference lists the vertices in set order)
    assert sorted(l for l in got if "->" not in l) == sorted(l for l in ref if "->" not in l)


@pytest.mark.gpu
def test_gpu_liftover(gpu_dev, tmp_path):
    check_liftover(gpu_dev, tmp_path)
