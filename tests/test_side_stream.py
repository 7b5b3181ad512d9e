"""The side stream of the window stage: what follows a sketch's first window kernel -- the block-minima pass over the strips
it gave up, the exact passes -- is queued on a third stream and runs beside the NEXT sketch's window kernel.  What can go wrong is a block
that two sketches in flight share, or a wait on the wrong event; both show at any size once sketches overlap, so the shapes are small.

Every case runs twice: under the SIMT mock (no marker) and on the GPU (`gpu`).  The mock executes every stream in order at the call, so its
half checks the bookkeeping -- stream ids, the allocator's third cache, the switch of ntl_ctx_set_pipeline, that NTL_SIDE_STREAM=0 (the
default) and NTL_PIPELINE=0 give the same bytes -- and costs seconds per sketch: its batches hold 3 reads of 3-8 kb where the GPU's hold 40 of 3-20 kb,
its contigs 28 kb instead of 155, and there are three batches instead of six (in-flight sketches do not exist there).  The concurrency
is the GPU half's."""
import threading

import numpy as np
import pytest

import oracle
import parity_cases as pc
from helpers import contig_ids
from ntlink_amd import capi

K, W, Z = 32, 250, 500
ON = {"NTL_SIDE_STREAM": "1"}  # (not the default: the knob is read when a context is made)
BACKENDS = [pytest.param("mock", id="mock"), pytest.param("gpu", id="gpu", marks=pytest.mark.gpu)]


def _open(backend):
    """a fresh context: the stream knobs are read when it is made"""
    if backend == "gpu":
        return capi.Device(0)
    from sim import simlib
    return simlib.device()


def _rc(s):
    return s[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))


_cases = {}


def _case(backend, kind):
    """contigs, six read batches of different sizes and the oracle's answers, made once per process.  `random`: reads cut from the
    contigs (both strands) and unrelated ones, 3-20 kb, plus one read shorter than k + w.  `mixed`: the same with a low-complexity
    stretch of more than w equal k-mers inside random sequence (its strips are given up: no window of theirs has one minimum) and a read
    with an N run (a multi-run strip: the exact pass)."""
    key = (backend, kind)
    if key in _cases:
        return _cases[key]
    rng = np.random.default_rng(77 if kind == "random" else 78)
    n_reads, longest = (40, 20000) if backend == "gpu" else (3, 8000)
    contigs = [pc.random_bases(rng, n) for n in ((60000, 45000, 30011, 20000) if backend == "gpu" else (16000, 12011))]
    batches = []
    for i in range(6 if backend == "gpu" else 3):
        reads = []
        for j in range(n_reads + i):  # (batches of different sizes: no two ask for the same blocks)
            n = int(rng.integers(3000, longest))
            if j % 4 == 3:
                reads.append(pc.random_bases(rng, n))
            else:
                c = contigs[int(rng.integers(0, len(contigs)))]
                at = int(rng.integers(0, len(c) - n))
                reads.append(c[at:at + n] if j % 2 else _rc(c[at:at + n]))
        reads.append(pc.random_bases(rng, K + W - 2 - i))  # shorter than k + w: no window
        if kind == "mixed":
            reads[0] = reads[0][:1500] + b"A" * (K + W + 700) + reads[0][1500:]
            reads[1] = reads[1][:2000] + b"N" * 9 + reads[1][2000:]
        batches.append(reads)
    ctg_len = np.array([len(s) for s in contigs], np.uint32)
    ooff, oh, op, os_ = oracle.sketch_batch(b"".join(contigs), pc.offsets_of(contigs), K, W)
    oix = oracle.Index(oh, contig_ids(ooff), op, os_)
    exp = []
    for reads in batches:
        rl = np.array([len(s) for s in reads], np.uint32)
        q = oracle.sketch_batch(b"".join(reads), pc.offsets_of(reads), K, W)
        exp.append((q, oracle.map_reads(oix, ctg_len, q[0], rl, q[1], q[2], q[3], k=K, threads=0, z=Z)))
    _cases[key] = (contigs, ctg_len, batches, exp)
    return _cases[key]


def _queue(dev, case, records, close_early=(), between=None):
    """The index, then every batch's sketch and map queued back to back with no host wait between them; then the results, in order.
    close_early: batches whose sketch and result are closed right after queueing.  between(i): called in front of batch i."""
    contigs, ctg_len, batches, _ = case
    csk = dev.sketch(dev.batch(contigs), K, W)
    ix = dev.index(csk, ctg_len)
    held = []
    for i, reads in enumerate(batches):
        if between:
            between(i)
        rl = np.array([len(s) for s in reads], np.uint32)
        rb = dev.batch(reads)
        sk = dev.sketch(rb, K, W, index=ix, records=records)
        res = dev.map(ix, sk, rl, k=K, z=Z)
        rb.close()
        if i in close_early:
            res.close(); sk.close()
            held.append(None)
        else:
            held.append((sk, res))
    out = []
    for h in held:
        if h is None:
            out.append(None)
            continue
        sk, res = h
        got = res.download()
        rec = sk.download() if sk.has_records else None
        out.append({"count": sk.count, "rec": rec, "maps": got, "strips": sk.strips, "redo": sk.redo_strips, "fallback": sk.fallback_strips,
                    "from_lists": sk.from_lists})
        res.close(); sk.close()
    ix.close(); csk.close()
    dev.sync()  # nothing failed behind our back
    return out


def _assert_oracle(out, case):
    for got, (q, exp) in zip(out, case[3]):
        if got is None:
            continue
        assert got["count"] == len(q[1]), "sketch count differs from the oracle's"
        if got["rec"] is not None:
            for a, b, what in zip(got["rec"], q, ("offsets", "hashes", "positions", "strands")):
                assert np.array_equal(a, b), f"{what} differ from the oracle's"
        pc.assert_same_records(got["maps"], exp)


def _blob(out):
    """everything a run returned, as bytes"""
    parts = []
    for got in out:
        if got is None:
            continue
        parts.append(np.uint64(got["count"]).tobytes())
        if got["rec"] is not None:
            parts += [a.tobytes() for a in got["rec"]]
        parts += [got["maps"][nm].tobytes() for nm in ("maps", "hits", "pafs")]
    return b"".join(parts)


def _run(backend, monkeypatch, case, records, env, **kw):
    """one run on a context of its own, made under `env`: (results, whether the side stream was in use)"""
    with monkeypatch.context() as m:
        for name, v in env.items():
            m.setenv(name, v)
        dev = _open(backend)
        try:
            side = dev.side_stream
            return _queue(dev, case, records, **kw), side
        finally:
            dev.close()


def _check_against_the_ways_back(backend, monkeypatch, case, records, env):
    out, side = _run(backend, monkeypatch, case, records, dict(env, **ON))
    assert side, "a pipelined context made under NTL_SIDE_STREAM=1 has its side stream"
    _assert_oracle(out, case)
    for back in ({"NTL_SIDE_STREAM": "0"}, {"NTL_SIDE_STREAM": "1", "NTL_PIPELINE": "0"}, {"NTL_SIDE_STREAM": "2"}):  # (2: the preparation on the side stream too)
        ref, ref_side = _run(backend, monkeypatch, case, records, dict(env, **back))
        assert ref_side == (back == {"NTL_SIDE_STREAM": "2"}), back
        assert _blob(ref) == _blob(out), f"not the bytes of the same calls under {back}"
    return out


@pytest.mark.parametrize("records", [True, False], ids=["records", "for_map"])
@pytest.mark.parametrize("backend", BACKENDS)
def test_overlap_with_every_strip_given_up(backend, records, monkeypatch):
    """NTL_SKETCH_FORCE_REDO=1: every strip's minimizers come from the side stream's passes.  Six sketches of different batches in
    flight, each followed by its map: counts, minimizers and mappings == the oracle's, and the bytes of the same calls without the
    side stream, on one stream, and with the preparation on the side stream as well."""
    case = _case(backend, "random")
    out = _check_against_the_ways_back(backend, monkeypatch, case, records, {"NTL_SKETCH_FORCE_REDO": "1"})
    for got in out:
        assert got["from_lists"] and got["redo"] == got["fallback"] == got["strips"] > 0, got["redo"]


@pytest.mark.parametrize("backend", BACKENDS)
def test_overlap_with_some_strips_given_up(backend, monkeypatch):
    """No knob: most strips are finished by the window kernel, the low-complexity stretch's are given up and redone by the exact pass,
    the strips across the N run take the multi-run pass."""
    case = _case(backend, "mixed")
    out = _check_against_the_ways_back(backend, monkeypatch, case, True, {})
    for got in out:
        print("strips", got["strips"], "redo", got["redo"], "fallback", got["fallback"])
        assert got["from_lists"] and 0 < got["redo"] < got["strips"], (got["redo"], got["strips"])  # both kinds of strip occurred
        assert got["fallback"] < got["strips"]


@pytest.mark.parametrize("backend", BACKENDS)
def test_list_pool_runs_out_while_the_next_sketch_is_queued(backend, monkeypatch):
    """A list slot of one entry and a pool of 50 (a strip lists some 30 minimizers): every sketch's lists run out, which the host learns when it asks for the first
    result -- with the later sketches queued behind it.  Each is made again through the bitmask: same records as the oracle."""
    case = _case(backend, "random")
    out, side = _run(backend, monkeypatch, case, True, dict(ON, NTL_LIST_SLOT="1", NTL_LIST_POOL="50"))
    assert side
    _assert_oracle(out, case)
    assert not any(got["from_lists"] for got in out)


@pytest.mark.parametrize("backend", BACKENDS)
def test_handles_closed_while_later_sketches_are_in_flight(backend, monkeypatch):
    """Sketch and result of batches 0, 2 and 3 are closed right after queueing: their blocks go back while the side stream's
    passes on them may not have run, and their events and slots wait on the queue of orphans.  The others == the oracle, and the sync
    at the end reports nothing."""
    case = _case(backend, "random")
    out, side = _run(backend, monkeypatch, case, True, dict(ON, NTL_SKETCH_FORCE_REDO="1"), close_early=(0, 2, 3))
    assert side and sum(got is None for got in out) == (3 if backend == "gpu" else 2)
    _assert_oracle(out, case)


@pytest.mark.parametrize("backend", BACKENDS)
def test_a_clone_beside_its_parent(backend, monkeypatch):
    """Two contexts, three streams each, driven by two threads at the same time: both == the oracle."""
    case = _case(backend, "random")
    monkeypatch.setenv("NTL_SKETCH_FORCE_REDO", "1")
    monkeypatch.setenv("NTL_SIDE_STREAM", "1")
    dev = _open(backend)
    other = dev.clone()
    results, errors = {}, []

    def work(name, d):
        try:
            results[name] = _queue(d, case, True)
        except BaseException as e:  # noqa: BLE001 (reported below, in the test's thread)
            errors.append((name, e))

    try:
        assert dev.side_stream and other.side_stream
        th = [threading.Thread(target=work, args=("parent", dev)), threading.Thread(target=work, args=("clone", other))]
        for t in th:
            t.start()
        for t in th:
            t.join()
    finally:
        other.close()
        dev.close()
    assert not errors, errors
    for name in ("parent", "clone"):
        _assert_oracle(results[name], case)


@pytest.mark.parametrize("backend", BACKENDS)
def test_pipeline_off_and_on_between_sketches(backend, monkeypatch):
    """ntl_ctx_set_pipeline(False) in front of the second batch and (True) in front of the third: the side stream is in use only while
    the pipeline is on, and the results are the oracle's on both sides of either switch."""
    case = _case(backend, "random")
    monkeypatch.setenv("NTL_SKETCH_FORCE_REDO", "1")
    monkeypatch.setenv("NTL_SIDE_STREAM", "1")
    dev = _open(backend)
    seen = []

    def between(i):
        if i == 1:
            dev.set_pipeline(False)
        if i == 2:
            dev.set_pipeline(True)
        seen.append((dev.pipelined, dev.side_stream))

    try:
        out = _queue(dev, case, True, between=between)
    finally:
        dev.close()
    assert seen == [(True, True), (False, False)] + [(True, True)] * (len(out) - 2)
    _assert_oracle(out, case)
