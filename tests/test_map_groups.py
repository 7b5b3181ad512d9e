"""The group path of the first map class (csrc/map_kernels.h map_read_groups) -- under the SIMT mock and on the GPU.

A wavefront of map_kernel<256,64,0> maps four reads at a time, one per group of 16 lanes, on quarters of the class's staging; a read
that is not SIMPLE (more than 64 hits or 16 runs, a contig in two runs, a noisy run, a run whose PAF record needs the rank sort)
leaves its group and is mapped by the full wavefront.  Minimizers and hits are crafted: every hit is a key of its own on a chosen
contig at a chosen position, so the shapes at which the group path can go wrong are met exactly:
  * 0 .. 65 hits around the group's lane count and capacity, each among no and among 255 / 256 minimizers (65 leaves, 64 among 256 stays);
  * 1, 2, 15, 16, 17 runs on distinct contigs (17 leaves), 16 runs of one hit, 64 hits in 16 runs of four;
  * every reason to leave in each of the four group positions, the neighbours simple reads of different lengths; all four at once
    (the rank sort with its modes 1, 2 and 3: mode 0 -- every transition of the sorted hits one way -- means the read order is the
    sorted order or, read positions being distinct, its exact reverse without a tie, which is the fast path: a run cannot reach it
    through the sort);
  * the fast PAF path's edges: increasing, strictly decreasing, two equal neighbours, one hit, a strand vote at exactly half, both strands;
  * batches of 1, 3, 4, 5, 8, 9, 13 reads, the other classes and an overflow read inside one group of eight, no hit at all, no read;
  * every flag; NTL_MAP_LANES=64 (the path is never entered) beside the default; and NTL_MAP_GROUP_STRICT=1, under which a result
    fails when a first-class read left its group: batches of reads that are simple by construction (shown from the oracle's records
    alone, test_simple_by_construction) must succeed -- the groups finished every one -- and every leaving case must fail with that
    message and no other, and succeed without the knob;
  * two results in flight and a slot's next holder: the strict bit one result raised is not seen by the next.
All of it record for record against the oracle."""
import contextlib
import functools
import os

import numpy as np
import pytest

import oracle
import parity_cases as pc
from helpers import contig_ids
from ntlink_amd import capi
from test_map_classes import CTG_LEN, FLAGS, K, World

LEFT = "left the group path"
HIT_COUNTS = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65]


class GWorld(World):
    """World with chosen hits: craft() takes (contig, contig position, contig strand, read strand) per hit, in read order.  One key per
    (contig, position): a position used twice in a read is a minimizer the read holds twice."""

    def __init__(self, seed):
        super().__init__(seed)
        self.at = {}
        self.runs = []   # per read: runs of its plan

    def craft(self, hits, nmx=None):
        nmx = len(hits) if nmx is None else nmx
        at = set(np.sort(self.rng.choice(nmx, len(hits), replace=False)).tolist()) if hits else set()
        it = iter(hits)
        toks = []
        for i in range(nmx):
            if i not in at:
                toks.append((self.key(), int(self.rng.integers(0, 2))))
                continue
            c, pos, cs, rs = next(it)
            assert 0 <= pos < CTG_LEN - K
            if (c, pos) not in self.at:
                self.at[c, pos] = self.key()
                self.ctgs[c].append((self.at[c, pos], pos, cs))
            toks.append((self.at[c, pos], rs))
        self.reads.append(toks)
        self.found.append(len(hits))
        ctgs = [h[0] for h in hits]
        self.runs.append(sum(1 for i, c in enumerate(ctgs) if i == 0 or c != ctgs[i - 1]))
        return len(self.reads) - 1

    def run(self, m, start=100, step=10, c=None):
        """m hits on one (new) contig, `step` apart from `start`, strands at random"""
        c = self.contigs(1)[0] if c is None else c
        return [(c, start + step * i, int(self.rng.integers(0, 2)), int(self.rng.integers(0, 2))) for i in range(m)]

    def simple(self, h, runs=None, nmx=None, step=10):
        """h hits in `runs` increasing runs on contigs of their own"""
        runs = min(h, 3) if runs is None else runs
        hits = []
        for q in range(runs):
            hits += self.run(h // runs + (1 if q < h % runs else 0), step=step)
        assert len(hits) == h
        return self.craft(hits, nmx)


def leavers(w):
    """one read per reason to leave the group path (default flags)"""
    a, b = w.contigs(2)
    aba = w.craft(w.run(2, c=a) + w.run(2, c=b) + w.run(2, 200, c=a))
    a, b = w.contigs(2)
    abab = w.craft(w.run(2, c=a) + w.run(2, c=b) + w.run(2, 200, c=a) + w.run(2, 200, c=b), 40)
    noisy0 = w.craft(w.run(3, 100, 40000))   # the x == 0 form: 80000 on the contig, a read of 1120 bases
    c = w.contigs(1)[0]
    up = lambda ps: [(c, p, 1, 1) for p in ps]
    mode1 = w.craft(up([100, 110, 120, 130, 140, 135, 150, 160, 170]))   # rank sort: 7 of 8 transitions increasing
    c = w.contigs(1)[0]
    mode2 = w.craft(up([170, 160, 150, 140, 130, 135, 120, 110, 100]), 30)   # 7 of 8 decreasing
    c = w.contigs(1)[0]
    mode3 = w.craft(up([100, 200, 110, 190, 120, 180]))   # neither: no PAF line
    hits65 = w.simple(65, 2)
    runs17 = w.simple(34, 17, 60)
    return {"aba": aba, "abab": abab, "noisy0": noisy0, "mode1": mode1, "mode2": mode2, "mode3": mode3,
            "hits65": hits65, "runs17": runs17}


@functools.lru_cache(maxsize=None)
def world():
    """the one world of this file: (world, batches, names of the batches in which a read leaves under the flags it is run with)"""
    w = GWorld(4242)
    b, leaving = {}, set()
    # hit counts, each with every minimizer found and among 255 or 256
    b["hits"] = [w.simple(h) for h in HIT_COUNTS[:-1]] + [w.simple(h, nmx=255 + (j & 1)) for j, h in enumerate(HIT_COUNTS[:-1])]
    b["hits65"] = [w.simple(65), w.simple(64, nmx=256), w.simple(65, nmx=256), w.simple(65, 1, nmx=255)]
    # run counts
    b["runs"] = [w.simple(2 * r, r) for r in (1, 2, 15, 16)] + [w.simple(16, 16), w.simple(64, 16), w.simple(16, 16, 256), w.simple(64, 16, 256)]
    b["runs17"] = [w.simple(16, 16), w.simple(34, 17), w.simple(17, 17, 200), w.simple(5)]
    # the fast PAF path
    c = w.contigs(1)[0]
    half = [(c, 100 + 10 * i, 1, i & 1) for i in range(4)]            # 2 * same == m
    c2 = w.contigs(1)[0]
    under = [(c2, 100 + 10 * i, 1, 0 if i else 1) for i in range(4)]   # one below half
    b["paf"] = [w.craft(w.run(7)), w.craft(w.run(7, 900, -10)), w.craft(w.run(2, 500, -10)), w.craft(w.run(3) + w.run(4, 900, -10) + w.run(1)),
                w.craft([h for i, h in enumerate(w.run(6)) for _ in range(2 if i == 2 else 1)]),   # two equal neighbours: non-decreasing
                w.craft(w.run(1)), w.craft(w.run(1), 200), w.craft(half), w.craft(under),
                w.craft([(h[0], h[1], h[2], 0) for h in w.run(5)]), w.craft([(h[0], h[1], h[2], 1) for h in w.run(5)], 100)]
    # every reason to leave, in each of the four group positions (read 4 * p + p of sixteen), beside simple reads of different lengths
    lv = leavers(w)
    pool = [w.simple(3), w.simple(40, 5, 250), w.simple(12, 2, 30), w.simple(0, 0, 130), w.simple(64, 16, 70), w.simple(1, 1, 256),
            w.simple(20, 4), w.simple(7, 7, 90), w.simple(33, 2, 40), w.simple(16, 1), w.simple(9, 3, 180), w.simple(2, 2)]
    for name, rd in lv.items():
        it = iter(pool)
        b["leave-" + name] = [rd if i % 4 == i // 4 else next(it) for i in range(16)]
        leaving.add("leave-" + name)
    b["leave-all4"] = [lv["abab"], lv["hits65"], lv["mode3"], lv["noisy0"]]
    b["leave-mixed"] = [pool[0], lv["aba"], pool[1], pool[2], lv["runs17"], pool[3], pool[4], lv["mode1"], pool[5]]
    # x = 0.3: a run on a contig whose hits are 37 apart is noisy (read positions are 40 apart); 10 apart is not
    b["noisy-x"] = [pool[0], w.simple(6, 1, step=37), pool[2], w.simple(30, 3, 40, step=37), w.simple(5, 1, step=37), pool[4], pool[5], w.simple(2, 1, step=37)]
    # batch shapes: partial rounds of four, partial groups of eight
    for n in (1, 3, 4, 5, 8, 9, 13):
        b[f"shape-{n}"] = [pool[(i + n) % len(pool)] for i in range(n)]
    # the other classes and an overflow read inside one group of eight
    c512, c1024, over = w.simple(5, 2, 300), w.simple(300, 4, 600), w.craft(w.run(1030))
    b["classes"] = [pool[0], c512, pool[1], c1024, over, pool[2], pool[4], pool[6], pool[7], c512, pool[8]]
    b["no-hit"] = [w.simple(0, 0, n) for n in (1, 17, 64, 200, 256)]
    b["empty"] = []
    leaving |= {"hits65", "runs17", "leave-all4", "leave-mixed"}
    return w, b, leaving


SIMPLE = ["hits", "runs", "paf", "classes", "no-hit", "empty"] + [f"shape-{n}" for n in (1, 3, 4, 5, 8, 9, 13)]
LEAVING = sorted(world()[2])


@functools.lru_cache(maxsize=None)
def expected(batch, flags):
    w, b, _ = world()
    coff, ch, cp, cs, ctg_len = w.contig_arrays()
    oix = oracle.Index(ch, contig_ids(coff), cp, cs)
    assert len(oix) == len(ch)
    arrays = w.read_arrays(b[batch])
    roff, rlen, rh, rp, rs = arrays
    exp = oracle.map_reads(oix, ctg_len, roff, rlen, rh, rp, rs, k=K, threads=0, **FLAGS[flags])
    return arrays, exp, sum(w.found[i] for i in b[batch])


@contextlib.contextmanager
def knobs(**kw):
    """the environment the map stage reads its knobs from when a result is queued"""
    names = {"lanes": "NTL_MAP_LANES", "strict": "NTL_MAP_GROUP_STRICT"}
    old = {n: os.environ.get(n) for n in names.values()}
    try:
        for key, n in names.items():
            os.environ.pop(n, None)
            if key in kw:
                os.environ[n] = str(kw[key])
        yield
    finally:
        for n, v in old.items():
            os.environ.pop(n, None)
            if v is not None:
                os.environ[n] = v


class Mapper:
    def __init__(self, dev):
        self.dev = dev
        coff, ch, cp, cs, ctg_len = world()[0].contig_arrays()
        with dev.sketch_from_arrays(coff, ch, cp, cs) as csk:
            self.ix = dev.index(csk, ctg_len)
        assert len(self.ix) == len(ch)

    def queue(self, batch, flags="default", **kw):
        (roff, rlen, rh, rp, rs), _, _ = expected(batch, flags)
        with knobs(**kw), self.dev.sketch_from_arrays(roff, rh, rp, rs) as rsk:
            return self.dev.map(self.ix, rsk, rlen, k=K, **FLAGS[flags])

    def verify(self, res, batch, flags="default"):
        _, exp, found = expected(batch, flags)
        got = res.download()
        try:
            pc.assert_same_records(got, exp)
        except AssertionError as e:
            raise AssertionError(f"{batch}, {flags}: {e}") from None
        assert res.counts() == (len(exp["maps"]), len(exp["hits"]), len(exp["pafs"])), f"{batch}, {flags}: counts"
        assert res.n_index_hits == found, f"{batch}, {flags}: n_index_hits {res.n_index_hits}, the index holds {found}"

    def check(self, batch, flags="default", **kw):
        with self.queue(batch, flags, **kw) as res:
            self.verify(res, batch, flags)

    def check_leaves(self, batch, flags="default"):
        """with the strict knob the result fails, with the message of a read that left its group and no other"""
        with self.queue(batch, flags, strict=1) as res:
            with pytest.raises(capi.NtlError) as e:
                res.wait()
        assert LEFT in str(e.value) and "twice" not in str(e.value) and "probe" not in str(e.value), str(e.value)

    def close(self):
        self.ix.close()
        self.dev.sync()
        self.dev.close()


# ---------------------------------------------------------------- the inputs are what the docstring says (no device)

def test_simple_by_construction():
    """From the oracle's records alone: every read of the SIMPLE batches that belongs to the first class has at most 64 hits in at most 16
    runs, as many mappings as runs -- no run dropped as noisy or subsumed, no contig twice -- on distinct contigs, and one PAF record per
    mapping, whose hits are all of the run's (the fast path: the rank sort's filter would drop some or make several)."""
    w, b, _ = world()
    seen = 0
    for batch in SIMPLE:
        _, exp, _ = expected(batch, "default")
        for j, i in enumerate(b[batch]):
            if len(w.reads[i]) > 256:
                continue
            seen += 1
            maps, pafs = exp["maps"][exp["maps"]["read"] == j], exp["pafs"][exp["pafs"]["read"] == j]
            assert w.found[i] <= 64 and w.runs[i] <= 16, (batch, j)
            assert len(maps) == w.runs[i] and int(maps["n_hits"].sum()) == w.found[i], (batch, j)
            assert len(set(maps["ctg"].tolist())) == len(maps), (batch, j)
            assert len(pafs) == len(maps) and (pafs["ctg"] == maps["ctg"]).all() and (pafs["n_hits"] == maps["n_hits"]).all(), (batch, j)
    assert seen > 80
    assert [w.found[i] for i in b["hits"][:10]] == HIT_COUNTS[:-1] == [w.found[i] for i in b["hits"][10:]]
    assert {len(w.reads[i]) for i in b["hits"][10:]} == {255, 256}
    assert [w.runs[i] for i in b["runs"]] == [1, 2, 15, 16, 16, 16, 16, 16]


def test_leavers_are_what_they_say():
    w, b, leaving = world()
    per = lambda exp, nm, j: exp[nm][exp[nm]["read"] == j]
    _, exp, _ = expected("leave-all4", "default")
    assert len(per(exp, "maps", 0)) == 0, "A B A B: each subsumes the other"
    assert per(exp, "maps", 1)["n_hits"].tolist() == [33, 32], "65 hits"
    assert len(per(exp, "maps", 2)) == 1 and len(per(exp, "pafs", 2)) == 0, "mode 3: a mapping without a PAF line"
    assert len(per(exp, "maps", 3)) == 0, "the noisy run is dropped"
    _, exp, _ = expected("leave-aba", "default")
    assert per(exp, "maps", 0)["n_hits"].tolist() == [4], "A B A: B is subsumed, the two runs on A become one"
    _, exp, _ = expected("leave-abab", "default")
    _, sens, _ = expected("leave-abab", "sensitive")
    assert len(per(exp, "maps", 0)) == 0 and per(sens, "maps", 0)["n_hits"].tolist() == [2, 2], \
        "A B A B: both contigs dropped by default; under sensitive only the inner runs, the outer two kept apart"
    for name in ("mode1", "mode2"):
        _, exp, _ = expected("leave-" + name, "default")
        assert per(exp, "pafs", 0)["n_hits"].tolist() == [8], name  # nine hits: the filter drops the one out of line
    _, exp, _ = expected("noisy-x", "x0.3")
    assert [len(per(exp, "maps", j)) for j in range(8)] == [3, 0, 2, 0, 0, 16, 1, 0]
    for batch in leaving:
        assert all(len(w.reads[i]) <= 256 for i in b[batch])


# ---------------------------------------------------------------- the checks (one set for the mock and the GPU)

def check_batch(m, batch, flags):
    m.check(batch, flags)
    m.check(batch, flags, lanes=64)
    if flags != "default":
        return
    if batch in world()[2]:
        m.check_leaves(batch)
    else:
        m.check(batch, flags, strict=1)          # the groups finished every first-class read
        m.check(batch, flags, strict=1, lanes=64)  # (nothing to leave)


def check_noisy_x(m):
    m.check("noisy-x", "x0.3")
    m.check("noisy-x", "x0.3", lanes=64)
    m.check_leaves("noisy-x", "x0.3")
    m.check("noisy-x", "default", strict=1)  # the same reads are simple without x


def check_repeat_filter_stays_out(m):
    """the group path is not entered: reads that would leave it raise nothing"""
    for batch in ("paf", "leave-all4", "leave-mode2", "hits65"):
        m.check(batch, "repeat_filter", strict=1)


def check_back_to_back(m):
    """two results in flight (two slots), one of which raises the strict bit; then the next holders of those slots"""
    a = m.queue("leave-mixed", strict=1)
    c = m.queue("shape-13", strict=1)
    with a, c:
        m.verify(c, "shape-13")
        with pytest.raises(capi.NtlError) as e:
            a.wait()
        assert LEFT in str(e.value)
    for batch in ("shape-9", "hits", "empty", "classes"):
        with m.queue(batch, strict=1) as res:
            m.verify(res, batch)
    a = m.queue("leave-mixed")
    c = m.queue("leave-all4", lanes=64)
    with a, c:
        m.verify(c, "leave-all4")
        m.verify(a, "leave-mixed")


CASES = [(b, "default") for b in SIMPLE + LEAVING] + \
        [(b, f) for f in ("sensitive", "x0.3", "repeat_filter") for b in ("hits", "runs", "paf", "leave-aba", "leave-abab", "leave-all4", "leave-mixed", "hits65")]
IDS = ["-".join(c) for c in CASES]


@pytest.fixture(scope="module")
def sim():
    from sim import simlib
    m = Mapper(simlib.device())
    yield m
    m.close()


@pytest.mark.parametrize("batch,flags", CASES, ids=IDS)
def test_sim_groups(sim, batch, flags):
    check_batch(sim, batch, flags)


def test_sim_noisy_x(sim):
    check_noisy_x(sim)


def test_sim_repeat_filter_stays_out(sim):
    check_repeat_filter_stays_out(sim)


def test_sim_back_to_back(sim):
    check_back_to_back(sim)


@pytest.fixture(scope="module")
def gpu():
    m = Mapper(capi.Device(0))
    yield m
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("batch,flags", CASES, ids=IDS)
def test_gpu_groups(gpu, batch, flags):
    check_batch(gpu, batch, flags)


@pytest.mark.gpu
def test_gpu_noisy_x(gpu):
    check_noisy_x(gpu)


@pytest.mark.gpu
def test_gpu_repeat_filter_stays_out(gpu):
    check_repeat_filter_stays_out(gpu)


@pytest.mark.gpu
def test_gpu_back_to_back(gpu):
    check_back_to_back(gpu)
