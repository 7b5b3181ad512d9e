"""The PAF block path of the map stage (csrc/map_kernels.h map_read, the general case behind the fast path) -- under the SIMT mock and on
the GPU.

A run whose read order is neither the (ctg_pos, read_pos) order nor its exact reverse is rank-sorted by counting, its duplicate contig
positions are marked, its transitions counted against the 3/4 threshold, and a four-way stencil filters single hits and breaks the run
into blocks: one record per block.  The runs here are crafted in the stencil's own terms (tests/paf_cases.py: a run is its sorted-order
sequence of read ranks) and every case is shown, from the plain restatement's trace alone, to have the event it is named for at the
sorted index it names:
  * every outcome of the stencil alone in a run of 14 to 18 hits, rising (mode 1) and as its mirror (mode 2): filter-next,
    filter-current, break (each at t = 1 as well), a false transition at t = 0 and at nt-1, nt-2, nt-3, duplicates at t, t+1, t+2, t-1, at sorted 0 and m-1,
    three hits on one position, two breaks in a row, a filter behind a break, a dropped hit just before a block's last;
  * the 3/4 threshold at equality and one transition to either side, for nt = 4, 7, 8; a block's strand vote at exactly half, one
    below half, and against the run's vote;
  * runs of 63 .. 67 and 127 .. 130 hits with every kind of event at sorted t = 62 .. 65, across the 64-lane stride, in sorted read
    order and reversed (the rank sort then moves every hit across strides), a duplicate pair on sorted 63 / 64, events at the run's end;
  * the same 130-hit runs inside reads of 300 and 600 minimizers (the 512 and 1024 staging classes) at an even and an odd first hit;
    runs of 257, 513 and 1030 hits (the last on the overflow list: 32-bit flags in global scratch) with events at both ends and at
    255 .. 257, 511 .. 513, 1023 / 1024, alone and behind a fast-path run of 4 and of 7 hits;
  * a read of five runs -- fast path, three blocks, mode 3 (no record), two blocks, fast path down -- of 40 and of 1100 hits;
  * all of them between simple reads in batches of 1, 5 and 13 (partial rounds and groups of the group path); every flag;
    NTL_MAP_LANES=64;
  * 300 seeded random runs of 3 to 200 hits, three to a read.
The restatement is held to the reference's own print_paf by tests/golden/gen/paf_blocks.json.gz, and to the oracle on every batch; the
device to the oracle, record for record."""
import collections
import functools
import gzip
import itertools
import json
import os

import numpy as np
import pytest

import oracle
import paf_cases as P
import parity_cases as pc
from helpers import contig_ids
from ntlink_amd import capi
from test_map_classes import FLAGS, K
from test_map_groups import GWorld, knobs

assert K == P.K
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gen", "paf_blocks.json.gz")
# what SWEEP_SEED gives, counted by the restatement (test_sweep_has_every_event prints the counts): the least each event must occur
SWEEP_MIN = {("filter-next", "pos"): 594, ("filter-current", "pos"): 179, ("dup-skip", "dup@t"): 101, ("break", "pos"): 67,
             ("dup-skip", "dup@t+1"): 25, ("filter-next", "dup@t+2"): 23, ("end-break", "end"): 20, ("filter-current", "dup@t-1"): 6}
SWEEP_PATHS = {"mode1": 120, "mode2": 120, "mode3": 51, "fast-up": 7, "fast-down": 2}


@functools.lru_cache(maxsize=None)
def world():
    """the one world of this file: (world, {batch: [read numbers]}, {read number: paf_cases.Read})"""
    w = GWorld(5150)
    defs, b = {}, {}

    def place(rd):
        hits = []
        for _, run, _ in rd.runs:
            c = w.contigs(1)[0]
            hits += [(c, pos, cs, rs) for pos, cs, rs in run]
        rid = w.craft(hits, rd.nmx)
        defs[rid] = rd
        return rid

    for name, reads in P.crafted().items():
        b[name] = [place(rd) for rd in reads]
    sw = [place(rd) for rd in P.sweep()]
    b["sweep-0"], b["sweep-1"] = sw[:len(sw) // 2], sw[len(sw) // 2:]
    simple = [w.simple(3), w.simple(40, 5, 250), w.simple(12, 2, 30), w.simple(0, 0, 130), w.simple(64, 16, 70), w.simple(1, 1, 256), w.simple(20, 4)]
    b["mix-1"] = [b["five"][1]]
    b["mix-5"] = [simple[0], b["five"][0], simple[2], b["long-257"][8], simple[1]]
    b["mix-13"] = [simple[0], b["small"][3], simple[1], b["class-300"][5], b["long-1030"][1], simple[2], b["five"][1], b["seam-129"][2],
                   simple[3], b["five-1100"][0], b["long-513"][9], simple[4], b["class-600"][2]]
    return w, b, defs


BATCHES = list(P.crafted()) + ["sweep-0", "sweep-1", "mix-1", "mix-5", "mix-13"]
SMALL = ["small", "votes"]
SEAMS = [f"seam-{m}" for m in P.SEAM_M]


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


def traced(rid, repeat_filter=False):
    """[(contig, hits, records, trace)] per run of a read, by the restatement"""
    return [(c, hits) + P.paf_of_run(hits, K) for c, hits in P.runs_in_world(world()[0], rid, repeat_filter) if hits]


def crafted_runs(batches):
    """(run name, spec, trace) of every crafted run of the batches, from the hits the world's read holds"""
    _, b, defs = world()
    for batch in batches:
        for rid in b[batch]:
            got = traced(rid)
            assert [len(x[1]) for x in got] == [len(r[1]) for r in defs[rid].runs], defs[rid].name
            for (name, _, sp), (_, _, _, tr) in zip(defs[rid].runs, got):
                yield name, sp, tr


class Mapper:
    def __init__(self, dev):
        self.dev = dev
        coff, ch, cp, cs, ctg_len = world()[0].contig_arrays()
        with dev.sketch_from_arrays(coff, ch, cp, cs) as csk:
            self.ix = dev.index(csk, ctg_len)
        assert len(self.ix) == len(ch)

    def check(self, batch, flags="default", **kw):
        (roff, rlen, rh, rp, rs), exp, found = expected(batch, flags)
        with knobs(**kw), self.dev.sketch_from_arrays(roff, rh, rp, rs) as rsk:
            res = self.dev.map(self.ix, rsk, rlen, k=K, **FLAGS[flags])
        with res:
            got = res.download()
            try:
                pc.assert_same_records(got, exp)
            except AssertionError as e:
                _, b, defs = world()
                at = ""
                if str(e).startswith("pafs["):
                    i = int(str(e)[5:str(e).index("]")])
                    rid = b[batch][int(exp["pafs"]["read"][i])]
                    at = f" (read {int(exp['pafs']['read'][i])}: {defs[rid].name if rid in defs else 'simple'})"
                raise AssertionError(f"{batch}, {flags}, {kw}: {e}{at}") from None
            assert res.counts() == (len(exp["maps"]), len(exp["hits"]), len(exp["pafs"])), f"{batch}, {flags}: counts"
            assert res.n_index_hits == found, f"{batch}, {flags}: n_index_hits {res.n_index_hits}, the index holds {found}"

    def close(self):
        self.ix.close()
        self.dev.sync()
        self.dev.close()


# ---------------------------------------------------------------- the restatement against the reference and the oracle (no device)

def test_restatement_equals_reference():
    """paf_of_run gives what the reference's print_paf printed for every run of the fixture, and the fixture holds the runs of this file"""
    with gzip.open(FIXTURE, "rt") as fh:
        fx = json.load(fh)
    assert fx["k"] == K and fx["read_step"] == P.RSTEP
    cases = P.fixture_cases()
    assert [c["name"] for c in fx["cases"]] == [name for name, _ in cases]
    n_lines = 0
    for c, (name, hits) in zip(fx["cases"], cases):
        stored = [(p, P.RSTEP * i, int(cs), int(rs)) for i, (p, cs, rs) in enumerate(zip(c["ctg_pos"], c["ctg_strand"], c["read_strand"]))]
        assert stored == hits, name
        recs, _ = P.paf_of_run(stored, fx["k"])
        assert [list(r) for r in recs] == c["paf"], name
        n_lines += len(recs)
    assert len(cases) > 400 and n_lines > len(cases)


def oracle_cases():
    return [(b, "default") for b in BATCHES] + [(b, f) for f in FLAGS if f != "default" for b in SMALL + SEAMS + ["five"]]


@pytest.mark.parametrize("batch,flags", oracle_cases(), ids=["-".join(c) for c in oracle_cases()])
def test_restatement_equals_oracle(batch, flags):
    """Per read: the oracle's mappings are the read's runs (every run an accepted contig; x = 0.3 may drop some: then the records of the
    ones it kept), its hit records their hits, its PAF records what the restatement makes of each run"""
    w, b, _ = world()
    _, exp, _ = expected(batch, flags)
    n_hits = 0
    for j, rid in enumerate(b[batch]):
        maps, pafs = exp["maps"][exp["maps"]["read"] == j], exp["pafs"][exp["pafs"]["read"] == j]
        runs = traced(rid, flags == "repeat_filter")
        if flags == "x0.3":
            kept = set(maps["ctg"].tolist())
            runs = [x for x in runs if x[0] in kept]
        assert [(x[0], len(x[1])) for x in runs] == list(zip(maps["ctg"].tolist(), maps["n_hits"].tolist())), (batch, j)
        hits = exp["hits"][int(maps["hit_off"][0]):][:int(maps["n_hits"].sum())] if len(maps) else []
        assert [h for x in runs for h in x[1]] == [(int(h["ctg_pos"]), int(h["read_pos"]), int(h["ctg_strand"]), int(h["read_strand"])) for h in hits]
        n_hits += len(hits)
        want = [(c,) + r[:5] + (1 if r[5] == "+" else 0,) for c, _, recs, _ in runs for r in recs]
        got = [tuple(int(p[f]) for f in ("ctg", "q_start", "q_end", "t_start", "t_end", "n_hits", "strand")) for p in pafs]
        assert got == want, (batch, j)
    assert n_hits == len(exp["hits"])


# ---------------------------------------------------------------- the cases are what their names say (from the trace alone)

def test_planted_events():
    """every crafted run takes the path it was made for and has exactly the events planted in it, where they were planted; none has a
    sorted index both filtered and a break, or a filtered one right in front of a break or of the end"""
    n = 0
    for name, sp, tr in crafted_runs(list(P.crafted())):
        assert tr["path"] == sp.path, (name, tr["path"])
        assert sp.want is None or sorted(tr["events"]) == sorted(sp.want), (name, tr["events"])
        assert not tr["both"] and not tr["tail_filtered"], name
        n += 1
    assert n > 800


def test_small_cases_cover_the_stencil():
    got = collections.defaultdict(set)
    for name, sp, tr in crafted_runs(["small"]):
        for t, what, why in tr["events"]:
            got[tr["path"]].add((what, why))
            if t <= 1:
                got[tr["path"]].add(f"t={t} {what}")
            got[tr["path"]] |= {f"nt-{d}" for d in (1, 2, 3) if t == tr["nt"] - d}
        if 0 in sp.tie - {1} or len(sp.vals) - 1 in sp.tie:
            got[tr["path"]].add("dup at m-1")
        if 1 in sp.tie:
            got[tr["path"]].add("dup at 0")
        if any(e - a == 2 for a, e in sp.groups()):
            got[tr["path"]].add("three on one")
        blocks = tr["blocks"]
        if len(blocks) == 3 and blocks[1] == 1:
            got[tr["path"]].add("block of one inside")
        if blocks[0] == 1:
            got[tr["path"]].add("first block of one")
        if any(f - 1 in tr["breaks"] for f in tr["filtered"]):
            got[tr["path"]].add("filter behind a break")
        if any(c - 2 in tr["filtered"] for c in tr["breaks"]):
            got[tr["path"]].add("dropped one before a block's last")
    every = P.DECIDERS | {"t=0 break", "t=1 filter-next", "t=1 filter-current", "t=1 break", "t=1 dup-skip", "nt-1", "nt-2", "nt-3", "dup at 0", "dup at m-1", "three on one", "block of one inside", "first block of one",
                          "filter behind a break", "dropped one before a block's last"}
    assert every <= got["mode1"] and every <= got["mode2"], (every - got["mode1"], every - got["mode2"])


def test_thresholds_and_votes():
    seen = {}
    for name, sp, tr in crafted_runs(["votes"]):
        if name.startswith("threshold"):
            seen[tr["nt"], tr["ups"]] = tr["path"]
    assert seen == {(nt, ups): path for nt, row in P.THRESHOLDS.items() for ups, path in row.items()}
    assert all(4 * ups == 3 * nt for nt, ups in ((4, 3), (8, 6))) and 4 * 5 == 3 * 7 - 1   # equality, and the nearest 7 comes to it
    _, b, defs = world()
    for rid in b["votes"]:
        if defs[rid].name in ("vote", "vote/down"):
            (_, hits, recs, tr), = traced(rid)
            assert tr["blocks"] == [4, 5, 7] and [r[5] for r in recs] == ["+", "-", "+"], defs[rid].name
            assert 2 * sum(1 for h in hits if h[2] == h[3]) >= len(hits), "the run as a whole votes +"
            break
    else:
        raise AssertionError("no vote case")


def test_seams_have_their_events():
    """per m and direction: every kind of event at every t of 62 .. 65 that the run has room for (all of them from m = 127 on), end events
    at nt-1, nt-2 and nt-3 (for m = 63 .. 67 these are the ones at 62 .. 65), a pair on sorted 63 / 64 from m = 65 on"""
    for m in P.SEAM_M:
        at = collections.defaultdict(set)
        pair = set()
        for name, sp, tr in crafted_runs([f"seam-{m}"]):
            assert tr["m"] == m and tr["path"] == ("mode2" if name.endswith("/down") else "mode1")
            for t, what, why in tr["events"]:
                at[tr["path"]].add((t, what, why))
            if 64 in sp.tie:
                pair.add(tr["path"])
        nt = m - 1
        for path in ("mode1", "mode2"):
            assert {(nt - 1, "end-break", "end"), (nt - 2, "end-break", "end"), (nt - 3, "filter-next", "pos")} <= at[path], (m, path)
            if m >= 127:
                assert {(t,) + d for t in P.SEAM_T for d in P.DECIDERS - {("end-break", "end")}} <= at[path], (m, path)
            assert (path in pair) == (m >= 65)
        if m >= 65:
            assert (63, "dup-skip", "dup@t") in at["mode2"]   # read backwards, the pair itself is out of line
    ends = {m: sorted(t for t in (m - 2, m - 3, m - 4) if t in P.SEAM_T) for m in P.SEAM_M[:5]}
    assert ends == {63: [], 64: [62], 65: [62, 63], 66: [62, 63, 64], 67: [63, 64, 65]}


def test_long_runs_have_their_events():
    for m, seams in ((257, ()), (513, (256,)), (1030, (256, 512, 1024))):
        ts, paths = set(), set()
        for name, sp, tr in crafted_runs([f"long-{m}"]):
            if not name.startswith("long"):
                continue
            assert tr["m"] == m and (0, "break", "pos") in tr["events"] and max(e[0] for e in tr["events"]) >= m - 5
            ts |= {e[0] for e in tr["events"]}
            paths.add(tr["path"])
        assert paths == {"mode1", "mode2"}
        assert {t for s in seams for t in ((s - 1, s) if s == 1024 else (s - 1, s, s + 1))} <= ts, m
        assert m - 2 in ts   # the end break at nt - 1: 255 of 257, 511 of 513
    w, b, defs = world()
    assert sorted({w.found[i] for i in b["long-1030"]}) == [1030, 1034, 1037] and sorted({w.found[i] for i in b["long-513"]}) == [513, 517, 520]
    assert {len(w.reads[i]) for i in b["class-300"]} == {300} and {len(w.reads[i]) for i in b["class-600"]} == {600}
    assert {len(defs[i].runs[0][1]) for i in b["class-300"]} == {2, 3}   # the general run begins at an even and at an odd hit
    for name in ("five", "five-1100"):
        for rid in b[name]:
            got = traced(rid)
            assert [x[3]["path"] for x in got] == ["fast-up", "mode1", "mode3", "mode2", "fast-down"]
            assert [len(x[2]) for x in got] == [1, 3, 0, 2, 1]
    assert [w.found[i] for i in b["five-1100"]] == [1100, 1100] and sorted(len(traced(i)[0][1]) for i in b["five"]) == [3, 4]
    assert [len(b[f"mix-{n}"]) for n in (1, 5, 13)] == [1, 5, 13]


def test_repeat_filter_changes_the_path():
    """under the repeat filter a duplicate is no hit at all: the cases named for one lose it, and take another way through the stencil"""
    _, b, defs = world()
    n = 0
    for rid in b["small"] + b["seam-130"]:
        with_dups, without = traced(rid), traced(rid, True)
        for (name, _, sp), a, z in zip(defs[rid].runs, with_dups, without):
            if not sp.tie:
                assert a[1:] == z[1:]
                continue
            n += 1
            assert any(why.startswith("dup@") for _, _, why in a[3]["events"]) or "pair" in name, name
            assert not any(why.startswith("dup@") for _, _, why in z[3]["events"]), name
            assert len(z[1]) < len(a[1]) and (a[3]["events"] != z[3]["events"] or a[3]["path"] != z[3]["path"] or "pair" in name), name
    assert n > 30


def test_sweep_has_every_event():
    events, paths = collections.Counter(), collections.Counter()
    _, b, defs = world()
    for rid in b["sweep-0"] + b["sweep-1"]:
        for _, _, _, tr in traced(rid):
            paths[tr["path"]] += 1
            assert not tr["both"] and not tr["tail_filtered"]
            for _, what, why in tr["events"]:
                events[what, why] += 1
    print(dict(events), dict(paths))
    assert sum(paths.values()) == P.SWEEP_RUNS == 300
    assert set(SWEEP_MIN) == P.DECIDERS
    for key, least in SWEEP_MIN.items():
        assert events[key] >= least, (key, events[key])
    for key, least in SWEEP_PATHS.items():
        assert paths[key] >= least, (key, paths[key])


def test_nothing_dropped_in_front_of_a_break():
    """Every order of up to seven hits, and of six with a pair at every place: no sorted index is both filtered and a break, the first is
    neither, and no filtered index stands right in front of a break or of the end -- a break at j needs j-1 out of line with j, and j-1
    is dropped only where j-2 is in line with j or j is a duplicate, either of which rules the break out.  So a block's first and last
    hit are the first and last walked over, filtered or not."""
    n = 0
    for m, ties in ((4, [()]), (5, [()]), (6, [()] + [(j,) for j in range(1, 6)]), (7, [()])):
        for perm in itertools.permutations(range(m)):
            for tie in ties:
                if tie and perm[tie[0] - 1] > perm[tie[0]]:
                    continue
                sp = P.of([10 * x for x in perm], tie, name="x")
                _, tr = P.paf_of_run(P.alone(P.hits_of(sp)), K)
                assert not tr["both"] and not tr["tail_filtered"] and 0 not in tr["filtered"] and 0 not in tr["breaks"], (perm, tie)
                n += bool(tr["events"])
    assert n > 600


# ---------------------------------------------------------------- the checks (one set for the mock and the GPU)

def check_batch(m, batch, flags, lanes):
    if lanes:
        m.check(batch, flags, lanes=lanes)
    else:
        m.check(batch, flags)


CASES = [(b, "default", 0) for b in BATCHES] + \
        [(b, f, 0) for f in FLAGS if f != "default" for b in SMALL + SEAMS + ["five", "five-1100"]] + \
        [(b, "default", 64) for b in SMALL + SEAMS]
IDS = [f"{b}-{f}" + (f"-lanes{n}" if n else "") for b, f, n in CASES]
# the mock half leaves out nothing: the largest batch costs it under two seconds
SIM_SKIP = set()
SIM_CASES = [c for c, i in zip(CASES, IDS) if i not in SIM_SKIP]


@pytest.fixture(scope="module")
def sim():
    from sim import simlib
    m = Mapper(simlib.device())
    yield m
    m.close()


@pytest.mark.parametrize("batch,flags,lanes", SIM_CASES, ids=[i for i in IDS if i not in SIM_SKIP])
def test_sim_paf(sim, batch, flags, lanes):
    check_batch(sim, batch, flags, lanes)


@pytest.fixture(scope="module")
def gpu():
    m = Mapper(capi.Device(0))
    yield m
    m.close()


@pytest.mark.gpu
@pytest.mark.parametrize("batch,flags,lanes", CASES, ids=IDS)
def test_gpu_paf(gpu, batch, flags, lanes):
    check_batch(gpu, batch, flags, lanes)
