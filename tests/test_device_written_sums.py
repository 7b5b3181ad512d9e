"""Sizes and sums that kernels write into the handles' page-locked slots (no copy on the stream): every count a handle reports equals
what its downloaded outputs hold, and the map results equal the oracle -- sub-batches queued back to back and collected late, the
strips' lists running out of pool (the second round through the bitmask), strips given to the redo pass, a sketch made without
mapping, handles destroyed before their work has run, and a batch destroyed while the map that reads its lengths is still queued.
Under the SIMT mock and on the GPU."""
import os
import re

import numpy as np
import pytest

import oracle
import parity_cases as pc
from helpers import contig_ids
from ntlink_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, W = 40, 100


def _sim_device(monkeypatch):
    from sim import simlib
    return simlib.device()


def _gpu_device(monkeypatch):
    return capi.Device(0)


DEVICES = [pytest.param(_sim_device, id="sim"), pytest.param(_gpu_device, id="gpu", marks=pytest.mark.gpu)]


@pytest.fixture(params=DEVICES)
def dev(request, monkeypatch):
    d = request.param(monkeypatch)
    yield d
    d.close()


def _index(dev, contigs):
    ctg_len = np.array([len(s) for s in contigs], np.uint32)
    cb = dev.batch(contigs)
    csk = dev.sketch(cb, K, W)
    ix = dev.index(csk, ctg_len)
    cb.close()
    coff, ch, cp, cs = csk.download()
    assert csk.count == int(coff[-1]) == len(ch)
    oix = oracle.Index(ch, contig_ids(coff), cp, cs)
    return csk, ix, oix, ctg_len


def _expected(oix, ctg_len, reads):
    rlen = np.array([len(s) for s in reads], np.uint32)
    qoff, qh, qp, qs = oracle.sketch_batch(b"".join(reads), pc.offsets_of(reads), K, W)
    return qoff, qh, oracle.map_reads(oix, ctg_len, qoff, rlen, qh, qp, qs, k=K, threads=0, z=1000)


def _index_hits(oix, qh):
    """read minimizers the index holds (a key that came from more than one contig place is not in it)"""
    return sum(1 for h in qh if oix.lookup(int(h)) is not None)


def _check_result(res, exp, n_hits_expected):
    got = res.download()
    nm, nh, npf = res.counts()
    assert (nm, nh, npf) == (len(got["maps"]), len(got["hits"]), len(got["pafs"]))
    assert int(got["maps"]["n_hits"].sum()) == nh
    pc.assert_same_records(got, exp)
    assert res.n_index_hits == n_hits_expected


def _reads():
    reads = pc.fixture_seqs("long_reads_4_top5.fa")
    return [reads[i::2] for i in range(2)] + [reads[1:4], reads[:1]]


def test_sub_batches_back_to_back_collected_late(dev):
    """As bench.py drives the hot path: read sketches made for the index and their maps queued one after the other (the window stage
    of sub-batch i+1 beside the map of sub-batch i on two streams), each batch destroyed at once, every result asked for at the end."""
    contigs = pc.fixture_seqs("scaffolds_4.fa")
    csk, ix, oix, ctg_len = _index(dev, contigs)
    held = []
    for g in _reads() * 2:
        rl = np.array([len(s) for s in g], np.uint32)
        rb = dev.batch(g)
        rsk = dev.sketch(rb, K, W, index=ix, records=False)
        rb.close()  # right after the sketch call: the map reads the batch's lengths
        res = dev.map(ix, rsk, rl, k=K, z=1000)
        held.append((g, rsk, res))
    for g, rsk, res in held:
        qoff, qh, exp = _expected(oix, ctg_len, g)
        assert rsk.count == len(qh) and rsk.from_lists
        _check_result(res, exp, _index_hits(oix, qh))
        res.close()
        rsk.close()
    dev.sync()
    ix.close(); csk.close()


def test_sketch_without_map(dev):
    """The lookup's count of a sketch that no map follows reaches the slot through a kernel of its own (sketch_finalize); the totals
    of a sketch made for the index, with records, match its download; a plain sketch too."""
    contigs = pc.fixture_seqs("scaffolds_4.fa")
    csk, ix, oix, ctg_len = _index(dev, contigs)
    reads = pc.fixture_seqs("long_reads_4_top5.fa")
    qoff, qh, exp = _expected(oix, ctg_len, reads)
    rl = np.array([len(s) for s in reads], np.uint32)
    with dev.batch(reads) as rb:
        for kw in ({}, {"index": ix}, {"index": ix, "records": False}):
            with dev.sketch(rb, K, W, **kw) as sk:
                assert sk.count == len(qh)
                if sk.has_records:
                    off, h, _, _ = sk.download()
                    assert int(off[-1]) == sk.count and np.array_equal(h, qh)
                # mapped only after its count was asked for: the map reads the sketch where it lies
                with dev.map(ix, sk, rl, k=K, z=1000) as res:
                    _check_result(res, exp, _index_hits(oix, qh))
    ix.close(); csk.close()


def test_list_pool_overflow_and_redo(dev, monkeypatch):
    """The strips' lists run out of pool (the sketch reports it through its slot and is made again through the bitmask when its count
    is asked for, its map with it); every strip through the redo pass (the redo kernel writes both counts into the slot)."""
    contigs = pc.fixture_seqs("scaffolds_4.fa")
    csk, ix, oix, ctg_len = _index(dev, contigs)
    reads = pc.fixture_seqs("long_reads_4_top5.fa")
    qoff, qh, exp = _expected(oix, ctg_len, reads)
    rl = np.array([len(s) for s in reads], np.uint32)
    with monkeypatch.context() as m:
        m.setenv("NTL_LIST_SLOT", "1")
        m.setenv("NTL_LIST_POOL", "500")
        rb = dev.batch(reads)
        rsk = dev.sketch(rb, K, W, index=ix, records=False)
        res = dev.map(ix, rsk, rl, k=K, z=1000)
        rb.close()
        _check_result(res, exp, _index_hits(oix, qh))
        assert rsk.count == len(qh) and not rsk.from_lists
        res.close(); rsk.close()
    with monkeypatch.context() as m:
        m.setenv("NTL_SKETCH_FORCE_REDO", "1")
        with dev.batch(reads) as rb, dev.sketch(rb, K, W, index=ix, records=False) as rsk, dev.map(ix, rsk, rl, k=K, z=1000) as res:
            _check_result(res, exp, _index_hits(oix, qh))
            assert rsk.count == len(qh) and rsk.from_lists
            assert rsk.redo_strips == rsk.fallback_strips > 0
    ix.close(); csk.close()


@pytest.mark.parametrize("make", DEVICES)
def test_handles_destroyed_before_their_work_has_run(make, monkeypatch):
    """Sketches and map results closed before anybody asked (the zombie checks read the words the kernels wrote), then more work on
    the recycled slots -- a context with four of them: its counts are those of its own outputs (the device half of a slot comes back
    zero)."""
    monkeypatch.setenv("NTL_NSLOTS", "4")
    dev = make(monkeypatch)
    try:
        _destroyed_early(dev)
    finally:
        dev.close()


def _destroyed_early(dev):
    contigs = pc.fixture_seqs("scaffolds_4.fa")
    csk, ix, oix, ctg_len = _index(dev, contigs)
    for g in _reads()[:3]:
        rl = np.array([len(s) for s in g], np.uint32)
        rb = dev.batch(g)
        rsk = dev.sketch(rb, K, W, index=ix, records=False)
        res = dev.map(ix, rsk, rl, k=K, z=1000)
        res.close(); rsk.close(); rb.close()
    dev.sync()  # nothing failed behind our back
    for g in _reads():
        qoff, qh, exp = _expected(oix, ctg_len, g)
        rl = np.array([len(s) for s in g], np.uint32)
        with dev.batch(g) as rb, dev.sketch(rb, K, W, index=ix, records=False) as rsk, dev.map(ix, rsk, rl, k=K, z=1000) as res:
            _check_result(res, exp, _index_hits(oix, qh))
    dev.sync()
    ix.close(); csk.close()


@pytest.mark.parametrize("make", DEVICES)
def test_refused_map_calls_give_everything_back(make, monkeypatch):
    """A map call that is refused after its result was armed (a sketch without records against another index than its own) hands
    back slot, event and references through the one error exit: six refusals on a context with four slots, then ordinary work on
    the same slots with the counts of its own outputs."""
    monkeypatch.setenv("NTL_NSLOTS", "4")
    dev = make(monkeypatch)
    try:
        _refused_then_mapped(dev)
    finally:
        dev.close()


def _refused_then_mapped(dev):
    contigs = pc.fixture_seqs("scaffolds_4.fa")
    csk, ix, oix, ctg_len = _index(dev, contigs)
    csk_b, ix_b, _, _ = _index(dev, contigs)
    g = _reads()[0]
    rl = np.array([len(s) for s in g], np.uint32)
    with dev.batch(g) as rb, dev.sketch(rb, K, W, index=ix, records=False) as rsk:
        for _ in range(6):
            with pytest.raises(capi.NtlError, match="maps against the index it was made for only") as e:
                dev.map(ix_b, rsk, rl, k=K, z=1000)
            assert e.value.code == capi.NTL_EINVAL
    ix_b.close(); csk_b.close()
    for g in _reads():
        qoff, qh, exp = _expected(oix, ctg_len, g)
        rl = np.array([len(s) for s in g], np.uint32)
        with dev.batch(g) as rb, dev.sketch(rb, K, W, index=ix, records=False) as rsk, dev.map(ix, rsk, rl, k=K, z=1000) as res:
            _check_result(res, exp, _index_hits(oix, qh))
    dev.sync()
    ix.close(); csk.close()


def _function_body(src, name):
    m = re.search(r"^(?:static |extern \"C\" )[^\n]*\b" + re.escape(name) + r"\(", src, re.M)
    assert m, name
    i = src.index("\n{", m.end())
    depth, j = 0, i + 1
    while True:
        if src[j] == "{":
            depth += 1
        elif src[j] == "}":
            depth -= 1
            if depth == 0:
                return src[i:j + 1]
        j += 1


# the stages sketch_enqueue is split into (mask_take, device_scan and launch_window_pass were separate before and stay out)
SKETCH_STAGES = ["sketch_prepare", "g8k_for", "sketch_window_stage", "emit_grid", "emit_launch", "sketch_emit_stage"]
# the stages map_enqueue is split into (device_scan was separate before and stays out)
MAP_STAGES = ["map_prepare", "map_lookup_stage", "map_kernels_stage", "map_gather_stage"]


def test_hot_path_queues_no_copies_or_fills():
    """The calls of the hot path (a read sketch made for an index, then its map) put no copy and no fill on a stream: the sizes and sums
    reach the host through the slots, written by the kernels.  What is left in sketch_enqueue and its stages belongs to the bitmask
    path (its totals) and to a batch without sequences."""
    src = open(os.path.join(ROOT, "ntlink_amd", "csrc", "ntl_hip.hip")).read()
    ops = re.compile(r"hip(?:Memcpy|Memset)(?:Async|D2D|D2H|H2D)?\s*\(")
    map_top = _function_body(src, "map_enqueue")
    for name in MAP_STAGES:  # map_enqueue itself calls every stage,
        assert re.search(r"\b" + name + r"\(", map_top), name
    assert not ops.findall(map_top + "".join(_function_body(src, name) for name in MAP_STAGES))  # and none of it copies or fills
    top = _function_body(src, "sketch_enqueue")
    stages = {name: _function_body(src, name) for name in SKETCH_STAGES}  # (asserts that each is found)
    body = top + "".join(stages.values())
    for name in ("sketch_prepare", "sketch_window_stage", "sketch_emit_stage"):  # sketch_enqueue itself calls the three stages,
        assert re.search(r"\b" + name + r"\(", top), name
    for name in SKETCH_STAGES:  # and every helper is called by it or by one of them: nothing is listed that the hot path does not run
        assert re.search(r"\b" + name + r"\(", body.replace(stages[name], "")), name
    left = [body[m.start():body.index(";", m.start())] for m in ops.finditer(body)]
    assert len(left) == 3, left
    assert "if (!nseq) HIPCHK(c, hipMemsetAsync(dsums" in body
    marker = "if (!lists) { /* the bitmask path"
    assert body.count(marker) == 1
    holder, = [b for b in [top, *stages.values()] if marker in b]
    bitmask = holder[holder.index(marker):]
    assert sum(1 for m in ops.finditer(bitmask)) == 2
    assert "redo.p, 8, hipMemcpyDeviceToHost" not in body
