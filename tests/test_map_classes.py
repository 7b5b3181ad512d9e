"""The map stage's staging classes and the lane-per-read gather (csrc/map_kernels.h) -- under the SIMT mock and on the GPU.

A read is mapped by the kernel of its class -- 256 / 512 / 1024 staged hits, chosen by its number of minimizers -- or, with more hits or
more runs than that kernel stages, on global scratch from the overflow list.  Every other test feeds the map reads whose hit count
follows their minimizer count; here both are chosen:
  * hit counts on both sides of every staging boundary (0, 1, 255 .. 257, 511 .. 513, 1023 .. 1025, 3000), each once with every minimizer
    found and once among 1744 more that the index does not hold (256 hits among 2000) -- one hit too many in a class overruns its
    LDS arrays and shows as a mismatch;
  * more runs than a class stages with few hits: 200 hits alternating over 65 and over 129 contigs (runs == hits), 400 and 600 over 129;
  * a read with more than 64 mappings (65 contigs, two hits each), reads with no record and with one;
  * every flag of the map (the boundary reads hold some minimizers twice: the repeat filter changes the hit count after the read
    was found to fit);
  * batches of 1, 7, 65 and 130 reads with all classes interleaved, an empty batch, one in which every read has more than 256 hits,
    one in which none has: mappings, hit_off, hits and PAF records in read order (the gather: a lane per read, reads beyond the
    last read of the last workgroup);
  * two results in flight on one context and a slot's next holder: the device sums a result leaves behind are seen by the next map
    on that slot -- an overflow count that is not zero makes it map reads of a list that is no longer there;
  * each of them behind a batch that found none of its minimizers and behind one that found all (the lookup reads the tags first, or
    the slots directly).
All of it record for record against the oracle."""
import functools

import numpy as np
import pytest

import oracle
import parity_cases as pc
from helpers import contig_ids
from ntlink_amd import capi

K = 24
CTG_LEN = 100000
FAR = 1744      # absent minimizers around the hits of the "far above" reads: 256 hits among 2000
BOUNDARY_HITS = [0, 1, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 3000]
FLAGS = {"default": {}, "sensitive": {"sensitive": True}, "repeat_filter": {"repeat_filter": True}, "x0.3": {"x": 0.3}}


class World:
    """Contigs and reads made together: a hit of a read is a key of its own, put on a contig at the next position of that contig -- but
    every 50th hit on a contig is the key of the hit before it once more (a minimizer the read has twice: one contig position twice
    among its hits, what the repeat filter drops); the absent minimizers of a read are keys no contig holds.  Read positions are 40
    apart, contig positions 10 or 37 apart by contig (with x = 0.3 the span filter drops the contigs of the second kind)."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.keys = set()
        self.ctgs = []    # per contig: [(key, pos, strand)]
        self.nhit = []    # per contig: hits made on it
        self.reads = []   # per read: [(key, strand)]
        self.found = []   # per read: hits

    def key(self):
        while True:
            key = int(self.rng.integers(1, 1 << 63)) * 2 + int(self.rng.integers(0, 2))
            if key not in self.keys and key != (1 << 64) - 1:
                self.keys.add(key)
                return key

    def contigs(self, n):
        first = len(self.ctgs)
        self.ctgs += [[] for _ in range(n)]
        self.nhit += [0] * n
        return list(range(first, first + n))

    def _hit(self, c):
        recs = self.ctgs[c]
        self.nhit[c] += 1
        if self.nhit[c] % 50 == 0:
            return recs[-1][0]
        pos = 100 + (10 if c % 2 == 0 else 37) * len(recs)
        assert pos < CTG_LEN - K
        key = self.key()
        recs.append((key, pos, int(self.rng.integers(0, 2))))
        return key

    def read(self, plan, nmx=None):
        """plan: the contig of every hit, in read order; nmx minimizers in all (the others absent, at random places)"""
        nmx = len(plan) if nmx is None else nmx
        at = set(np.sort(self.rng.choice(nmx, len(plan), replace=False)).tolist()) if plan else set()
        it = iter(plan)
        toks = [(self._hit(next(it)) if i in at else self.key(), int(self.rng.integers(0, 2))) for i in range(nmx)]
        self.reads.append(toks)
        self.found.append(len(plan))
        return len(self.reads) - 1

    # plans
    def blocks(self, h):
        """A A .. B B .. A A .. C C ..: a quarter each (B lies inside A: subsumed)"""
        a, b, c = self.contigs(3)
        q = h // 4
        return [a] * q + [b] * q + [a] * q + [c] * (h - 3 * q)

    def alternating(self, h, m):
        cs = self.contigs(m)
        return [cs[i % m] for i in range(h)]

    def pairs(self, m):
        return [c for c in self.contigs(m) for _ in range(2)]

    # arrays
    def contig_arrays(self):
        coff = np.zeros(len(self.ctgs) + 1, np.uint64)
        np.cumsum([len(c) for c in self.ctgs], out=coff[1:])
        flat = [rec for c in self.ctgs for rec in c]
        return (coff, np.array([r[0] for r in flat], np.uint64), np.array([r[1] for r in flat], np.uint32),
                np.array([r[2] for r in flat], np.uint8), np.full(len(self.ctgs), CTG_LEN, np.uint32))

    def read_arrays(self, ids):
        reads = [self.reads[i] for i in ids]
        roff = np.zeros(len(reads) + 1, np.uint64)
        np.cumsum([len(t) for t in reads], out=roff[1:])
        rh = np.array([key for t in reads for key, _ in t], np.uint64)
        rp = np.array([40 * i for t in reads for i in range(len(t))], np.uint32)
        rs = np.array([s for t in reads for _, s in t], np.uint8)
        rlen = np.array([40 * len(t) + 1000 for t in reads], np.uint32)
        return roff, rlen, rh, rp, rs


@functools.lru_cache(maxsize=None)
def world():
    """the one world of this file and its batches (lists of read numbers); the mock half and the GPU half share it"""
    w = World(2025)
    b = {}
    boundary = []
    for h in BOUNDARY_HITS:
        boundary.append(w.read(w.blocks(h)))             # nmx == hits
        boundary.append(w.read(w.blocks(h), h + FAR))    # the same hits among 1744 absent minimizers
    runs = [w.read(w.alternating(200, 65)), w.read(w.alternating(200, 129)), w.read(w.alternating(400, 129)),
            w.read(w.alternating(600, 129)), w.read(w.alternating(200, 65), 200 + FAR)]
    many = w.read(w.pairs(65))
    b["boundaries"] = boundary + runs + [many]
    # a pool of every kind, dealt round: no record, one hit, few hits, 257 / 513 / 1025 hits (the 512 class, the 1024 class, the
    # overflow list), few hits among many minimizers, more runs than the first class stages, more than 64 mappings
    pool = [w.read([]), w.read(w.blocks(1)), w.read(w.blocks(40)), boundary[8], w.read(w.blocks(100), 400),
            boundary[14], w.read(w.blocks(5)), boundary[20], runs[0], many, w.read(w.blocks(3), 30)]
    for n in (1, 7, 65, 130):
        b[f"mixed-{n}"] = [pool[(i + 3) % len(pool)] for i in range(n)]  # (a batch of one read: one of 257 hits)
    b["empty"] = []
    b["prime-tags"], b["prime-direct"] = [boundary[1]], [pool[2]]  # a batch that finds none of its minimizers, one that finds all
    b["all-above-256"] = [pool[3], pool[5], pool[7], runs[2], runs[3], boundary[9], boundary[13], boundary[21], boundary[23]]
    b["none-above-256"] = [pool[0], pool[1], pool[2], pool[4], pool[6], boundary[6], boundary[7], runs[4], pool[10]]
    above = lambda i: w.found[i] > 256
    assert all(above(i) for i in b["all-above-256"]) and not any(above(i) for i in b["none-above-256"])
    assert any(len(w.reads[i]) > 256 for i in b["none-above-256"])  # long reads among them: the hits of a long read may fit the first class
    return w, b


@functools.lru_cache(maxsize=None)
def expected(batch, flags):
    """(the read arrays, the oracle's records of them, the hits the index holds), made once per batch and flag set"""
    w, b = world()
    coff, ch, cp, cs, ctg_len = w.contig_arrays()
    oix = oracle.Index(ch, contig_ids(coff), cp, cs)
    assert len(oix) == len(ch)
    arrays = w.read_arrays(b[batch])
    roff, rlen, rh, rp, rs = arrays
    exp = oracle.map_reads(oix, ctg_len, roff, rlen, rh, rp, rs, k=K, threads=0, **FLAGS[flags])
    return arrays, exp, sum(w.found[i] for i in b[batch])


class Mapper:
    """a device with the world's index on it"""

    def __init__(self, dev):
        self.dev = dev
        coff, ch, cp, cs, ctg_len = world()[0].contig_arrays()
        with dev.sketch_from_arrays(coff, ch, cp, cs) as csk:
            self.ix = dev.index(csk, ctg_len)
        assert len(self.ix) == len(ch)

    def queue(self, batch, flags="default"):
        (roff, rlen, rh, rp, rs), _, _ = expected(batch, flags)
        with self.dev.sketch_from_arrays(roff, rh, rp, rs) as rsk:
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

    def prime(self, form):
        """a batch that finds none of its minimizers ("tags": the next lookup on this index reads the tags first) or all of them
        ("direct": the slots directly).  The result is the same."""
        with self.queue("prime-" + form) as res:
            found, nmx = res.n_index_hits, len(expected("prime-" + form, "default")[0][2])
        assert found == (0 if form == "tags" else nmx) and nmx

    def check(self, batch, flags="default", form="tags"):
        self.prime(form)
        with self.queue(batch, flags) as res:
            self.verify(res, batch, flags)

    def close(self):
        self.ix.close()
        self.dev.sync()
        self.dev.close()


# ---------------------------------------------------------------- the inputs are what the docstring says (no device)

def test_world():
    w, b = world()
    assert [w.found[i] for i in b["boundaries"][:24:2]] == BOUNDARY_HITS == [w.found[i] for i in b["boundaries"][1:24:2]]
    assert [len(w.reads[i]) for i in b["boundaries"][:24:2]] == BOUNDARY_HITS
    assert [len(w.reads[i]) for i in b["boundaries"][1:24:2]] == [h + FAR for h in BOUNDARY_HITS]
    _, exp, found = expected("boundaries", "default")
    per_read = np.bincount(exp["maps"]["read"], minlength=len(b["boundaries"]))
    assert per_read.max() > 64 and per_read[-1] == 65, "a read with more than 64 mappings"
    assert (per_read == 0).any() and (per_read == 1).any() and 0 < len(exp["hits"]) <= found
    # the repeat filter drops hits of the boundary reads (a minimizer twice in a read): fewer hit records than without it
    assert len(expected("boundaries", "repeat_filter")[1]["hits"]) < len(exp["hits"])
    # x = 0.3 drops contigs the default keeps
    assert len(expected("boundaries", "x0.3")[1]["maps"]) < len(exp["maps"])
    for n in (1, 7, 65, 130):
        assert len(b[f"mixed-{n}"]) == n
    assert len(expected("mixed-130", "default")[1]["maps"]) > 130


# ---------------------------------------------------------------- the checks (one set for the mock and the GPU)

def check_back_to_back(m):
    """two results in flight (two slots), then the next holders of those slots"""
    m.prime("tags")
    a = m.queue("mixed-65")
    c = m.queue("all-above-256")
    with a, c:
        m.verify(c, "all-above-256")
        m.verify(a, "mixed-65")
    for batch in ("none-above-256", "mixed-7", "empty", "all-above-256"):
        with m.queue(batch) as res:
            m.verify(res, batch)


BATCHES = ["mixed-1", "mixed-7", "mixed-65", "mixed-130", "empty", "all-above-256", "none-above-256"]
CASES = [("boundaries", f, "tags") for f in FLAGS] + [("boundaries", "default", "direct"), ("boundaries", "repeat_filter", "direct")] + \
        [(b, "default", "tags") for b in BATCHES] + [(b, "default", "direct") for b in ("mixed-65", "all-above-256", "none-above-256")]
IDS = ["-".join(c) for c in CASES]
# the mock (one thread per lane) pays seconds for a batch of a hundred reads or of several thousand hits: its half leaves out the
# largest batch and the second run of the boundary reads under the repeat filter; every kind of read, every flag and both forms stay
SIM_SKIP = {"mixed-130-default-tags", "boundaries-repeat_filter-direct"}
SIM_CASES = [c for c, i in zip(CASES, IDS) if i not in SIM_SKIP]


@pytest.fixture(scope="module")
def sim():
    from sim import simlib
    m = Mapper(simlib.device())
    yield m
    m.close()


@pytest.mark.parametrize("batch,flags,form", SIM_CASES, ids=[i for i in IDS if i not in SIM_SKIP])
def test_sim_map(sim, batch, flags, form):
    sim.check(batch, flags, form)


def test_sim_back_to_back(sim):
    check_back_to_back(sim)


@pytest.fixture(scope="module")
def gpu():
    m = Mapper(capi.Device(0))
    yield m
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("batch,flags,form", CASES, ids=IDS)
def test_gpu_map(gpu, batch, flags, form):
    gpu.check(batch, flags, form)


@pytest.mark.gpu
def test_gpu_back_to_back(gpu):
    check_back_to_back(gpu)
