"""Crafted and random runs for the PAF block path of the map stage (tests/test_paf_blocks.py): what map_read of csrc/map_kernels.h makes of a
run -- the hits of a read on one accepted contig -- whose read order is neither the (ctg_pos, read_pos) order nor its exact reverse.

The reference here is plain Python over the hits of one run, paf_of_run(): no device, no library, no oracle.  In words:
  order      the hits sorted by (contig position, read position); m of them, nt = m - 1 transitions between sorted neighbours
  fast       one hit, or the read order is the sorted order ("fast-up") or its exact reverse ("fast-down"): one block of all hits
  twice      the contig positions that two or more hits of the run share
  mode       every transition rising or every one falling: one block ("mode0": not reachable with distinct read positions);
             at least 3/4 of the transitions rising (read positions a <= b): "mode1"; at least 3/4 not rising: "mode2", which reads
             every comparison below the other way round; neither: "mode3", no record at all
  stencil    per false transition t (sorted elements t and t+1 out of line), in this order of precedence:
               dup-skip        t or t+1 lies on a position held twice: nothing happens
               end-break       t + 2 >= nt: a new block begins at t+1
               filter-next     t+2 lies on a position held twice, or t and t+2 are in line: t+1 is dropped
               filter-current  t > 0, and t-1 lies on a position held twice or t-1 and t+1 are in line: t is dropped
               break           a new block begins at t+1
  blocks     the sorted hits without the dropped ones, cut in front of every break that was not dropped itself
  record     per block: the smaller and the larger read / contig position of its first and last hit (+ k on the larger), the number of
             hits, "+" where at least half of its hits have equal strands
paf_of_run() also returns a trace of all that, from which the tests show that a case named for an event has it at that sorted index.

A run is written as its SORTED-ORDER SEQUENCE OF READ RANKS: vals[j] says where in the read the j-th hit by contig position stands (any
distinct numbers: only their order counts), tie holds the sorted indices that share their contig position with the one before.  That is
the stencil's own view.  hits_of() turns it into hits in read order, mirror() into the same run read backwards (mode 2)."""
import collections
import functools
import itertools
import zlib

import numpy as np

K = 24          # as tests/test_map_classes.py
RSTEP = 40      # read positions of neighbouring minimizers, as World.read_arrays
CSTART, CSTEP = 100, 5
SWEEP_SEED, SWEEP_RUNS = 20250, 300
SEAM_M = (63, 64, 65, 66, 67, 127, 128, 129, 130)
SEAM_T = (62, 63, 64, 65)
KINDS = ("filter-next", "filter-current", "break", "dup-at-t", "dup-at-t1", "dup-t2-next", "dup-t1-current")
OUTCOMES = ("dup-skip", "end-break", "filter-next", "filter-current", "break")
DECIDERS = {("dup-skip", "dup@t"), ("dup-skip", "dup@t+1"), ("end-break", "end"), ("filter-next", "dup@t+2"), ("filter-next", "pos"),
            ("filter-current", "dup@t-1"), ("filter-current", "pos"), ("break", "pos")}
PATHS = ("fast-up", "fast-down", "one-hit", "mode1", "mode2", "mode3")


# ---------------------------------------------------------------- the plain reference

def paf_of_run(hits, k):
    """hits: (ctg_pos, read_pos, ctg_strand, read_strand) in read order -> ([(q_start, q_end, t_start, t_end, n_hits, strand)], trace)"""
    hits = [tuple(h) for h in hits]
    m = len(hits)
    order = sorted(hits, key=lambda h: (h[0], h[1]))
    tr = dict(path=None, m=m, nt=m - 1, ups=None, events=[], filtered=[], breaks=[], blocks=[], both=[], tail_filtered=[])
    if m == 1:
        tr["path"], blocks = "one-hit", [order]
    elif order == hits:
        tr["path"], blocks = "fast-up", [order]
    elif order[::-1] == hits:
        tr["path"], blocks = "fast-down", [order]
    else:
        blocks = _general(order, tr)
    tr["blocks"] = [len(b) for b in blocks]
    recs = []
    for b in blocks:
        assert b, "an empty block"
        (c0, r0, _, _), (c1, r1, _, _) = b[0], b[-1]
        same = sum(1 for h in b if h[2] == h[3])
        recs.append((min(r0, r1), max(r0, r1) + k, min(c0, c1), max(c0, c1) + k, len(b), "+" if 2 * same >= len(b) else "-"))
    return recs, tr


def _general(order, tr):
    m, nt = len(order), len(order) - 1
    cp, rp = [h[0] for h in order], [h[1] for h in order]
    seen = collections.Counter(cp)
    dup = [seen[p] > 1 for p in cp]
    ups = sum(1 for t in range(nt) if rp[t] <= rp[t + 1])
    downs = sum(1 for t in range(nt) if rp[t] >= rp[t + 1])
    tr["ups"] = ups
    if ups == nt or downs == nt:
        tr["path"] = "mode0"
        return [order]
    if 4 * ups >= 3 * nt:
        tr["path"], in_line = "mode1", lambda i, j: rp[i] <= rp[j]
    elif 4 * (nt - ups) >= 3 * nt:
        tr["path"], in_line = "mode2", lambda i, j: rp[i] >= rp[j]
    else:
        tr["path"] = "mode3"
        return []
    drop, cut, ev = set(), set(), tr["events"]
    for t in range(nt):
        if in_line(t, t + 1):
            continue
        if dup[t] or dup[t + 1]:
            ev.append((t, "dup-skip", "dup@t" if dup[t] else "dup@t+1"))
        elif t + 2 >= nt:
            cut.add(t + 1)
            ev.append((t, "end-break", "end"))
        elif dup[t + 2] or in_line(t, t + 2):
            drop.add(t + 1)
            ev.append((t, "filter-next", "dup@t+2" if dup[t + 2] else "pos"))
        elif t > 0 and (dup[t - 1] or in_line(t - 1, t + 1)):
            drop.add(t)
            ev.append((t, "filter-current", "dup@t-1" if dup[t - 1] else "pos"))
        else:
            cut.add(t + 1)
            ev.append((t, "break", "pos"))
    tr["filtered"], tr["breaks"], tr["both"] = sorted(drop), sorted(cut), sorted(drop & cut)
    # a dropped element right in front of a break or of the end: the block's last hit is then not the last one walked over
    tr["tail_filtered"] = sorted(i for i in drop if i + 1 == m or i + 1 in cut)
    blocks = [[]]
    for i, h in enumerate(order):
        if i in drop:
            continue
        if i in cut:
            blocks.append([])
        blocks[-1].append(h)
    return blocks


def drop_repeats(hits):
    """the repeat filter on the hits of one run: a contig position held twice is a minimizer the read holds twice; all of its hits go"""
    seen = collections.Counter(h[0] for h in hits)
    return [h for h in hits if seen[h[0]] == 1]


# ---------------------------------------------------------------- runs as the stencil sees them

class Spec:
    """vals[j]: where in the read the j-th hit in sorted order stands; tie: the j that share their contig position with j - 1;
    same[j]: whether that hit's strands are equal (None: drawn from the run's name); want: the events planted, as the trace names them"""

    def __init__(self, vals, tie=(), same=None, want=(), path=None, name=""):
        self.vals, self.tie, self.same, self.path, self.name = list(vals), set(tie), same, path, name
        self.want = None if want is None else list(want)   # None: not planted by hand, whatever the trace says
        self.touched = set()

    def groups(self):
        """maximal stretches of sorted indices on one contig position, as (first, last)"""
        out, j, m = [], 0, len(self.vals)
        while j < m:
            e = j
            while e + 1 < m and e + 1 in self.tie:
                e += 1
            out.append((j, e))
            j = e + 1
        return out


def base(m, name="", path="mode1"):
    return Spec([10 * i for i in range(m)], path=path, name=name)


def of(vals, tie=(), same=None, want=(), path="mode1", name=""):
    return Spec(vals, tie, same, want, path, name)


def _claim(sp, lo, hi):
    region = set(range(max(lo, 0), min(hi, len(sp.vals) - 1) + 1))
    if region & sp.touched:
        return False
    sp.touched |= region
    return True


def plant(sp, kind, t):
    """one event of `kind` whose false transition is t; False (and nothing done) where the run has no room for it there"""
    m, v = len(sp.vals), sp.vals
    if t < (2 if kind == "dup-t1-current" else 1) or t + 3 > m - 1 or not _claim(sp, t - 2, t + 3):
        return False
    if kind == "filter-next":            # .. 1 5 2 6 ..
        v[t + 1] = v[t] - 25
        sp.want.append((t, "filter-next", "pos"))
    elif kind == "filter-current":       # .. 1 9 2 3 ..
        v[t] += 43
        sp.want.append((t, "filter-current", "pos"))
    elif kind in ("break", "dup-t2-next", "dup-t1-current"):   # 5 6 7 0 1 2 3 4 ..
        for j in range(t + 1, t + 4):
            v[j] -= 100000
        if kind == "break":
            sp.want.append((t, "break", "pos"))
        elif kind == "dup-t2-next":
            sp.tie.add(t + 3)
            sp.want.append((t, "filter-next", "dup@t+2"))
        else:
            sp.tie.add(t - 1)
            sp.want.append((t, "filter-current", "dup@t-1"))
    elif kind == "dup-at-t":
        sp.tie.add(t)
        v[t + 1] = v[t] - 25
        sp.want.append((t, "dup-skip", "dup@t"))
    elif kind == "dup-at-t1":
        sp.tie.add(t + 2)
        v[t] += 43
        sp.want.append((t, "dup-skip", "dup@t+1"))
    else:
        raise ValueError(kind)
    return True


def plant_front(sp):
    """9 0 1 2 ..: a false transition at t = 0, a first block of one"""
    if not _claim(sp, 0, 2):
        return False
    sp.vals[0] = 93
    sp.want.append((0, "break", "pos"))
    return True


def plant_end(sp, back):
    """an outlier at sorted index m - back, back = 1, 2 (end breaks at t = nt - 1, nt - 2) or 3 (t = nt - 3: it is filtered)"""
    m = len(sp.vals)
    j = m - back
    if j < 2 or not _claim(sp, j - 1, j + 1):
        return False
    sp.vals[j] = 10 * j - 500003
    sp.want.append((j - 1, "filter-next", "pos") if back == 3 else (j - 1, "end-break", "end"))
    return True


def plant_pair(sp, j):
    """sorted j - 1 and j on one contig position, nothing out of line"""
    if j < 1 or j > len(sp.vals) - 1 or not _claim(sp, j - 1, j):
        return False
    sp.tie.add(j)
    return True


def mirror(sp):
    """the same run read backwards: every event at the same sorted index in mode 2; inside a contig position held several times the
    sorted order goes by read position, so there the transitions are false now and skipped"""
    vals = [-x for x in sp.vals]
    want = None if sp.want is None else list(sp.want)
    for a, e in sp.groups():
        vals[a:e + 1] = vals[a:e + 1][::-1]
        if want is not None:
            want += [(j, "dup-skip", "dup@t") for j in range(a, e)]
    path = {"mode1": "mode2", "mode2": "mode1", "fast-up": "fast-down", "fast-down": "fast-up"}.get(sp.path, sp.path)
    if sp.path == "fast-up" and sp.tie:
        path = "mode2"
    return Spec(vals, sp.tie, sp.same, want, path, sp.name + "/down")


def hits_of(sp, start=CSTART):
    """-> [(ctg_pos, ctg_strand, read_strand)] in read order"""
    m = len(sp.vals)
    assert len(set(sp.vals)) == m, sp.name
    for a, e in sp.groups():
        assert sp.vals[a:e + 1] == sorted(sp.vals[a:e + 1]), f"{sp.name}: hits on one contig position stand in read order"
    rng = np.random.default_rng(zlib.crc32(sp.name.encode()))
    same = sp.same if sp.same is not None else (rng.integers(0, 4, m) != 0).tolist()
    out, slot, cs = [], -1, 0
    for j in range(m):
        if j not in sp.tie:
            slot, cs = slot + 1, int(rng.integers(0, 2))
        out.append((sp.vals[j], start + CSTEP * slot, cs, cs if same[j] else 1 - cs))
    return [h[1:] for h in sorted(out)]


def alone(run, first=0):
    """a run by itself, the first of its hits the read's minimizer number `first`: what paf_of_run and the reference's print_paf take"""
    return [(p, RSTEP * (first + i), cs, rs) for i, (p, cs, rs) in enumerate(run)]


# ---------------------------------------------------------------- (a) the stencil, each outcome alone, small

def small_specs():
    def one(name, m, how):
        sp = base(m, name)
        assert how(sp), name
        return sp
    out = [one(f"small {kind}", 14, functools.partial(plant, kind=kind, t=5)) for kind in KINDS]
    # t = 1: the first transition that has a neighbour in front of it
    out += [one(f"small {kind} t=1", 14, functools.partial(plant, kind=kind, t=1)) for kind in KINDS[:3]]
    out.append(one("small front", 14, plant_front))
    out += [one(f"small end -{back}", 14, functools.partial(plant_end, back=back)) for back in (1, 2, 3)]
    # duplicates at sorted 0 / 1 and m-2 / m-1, a false transition next to each
    out.append(of([40, 50, 0, 10, 20, 30, 60, 70, 80, 90, 100, 110, 120, 125, 127, 150, 130, 140], tie={1, 17}, name="small dups at both ends",
                  want=[(1, "dup-skip", "dup@t"), (15, "dup-skip", "dup@t+1")]))
    out.append(of([0, 10, 20, 60, 70, 80, 30, 40, 50, 90, 100, 110, 120, 130], tie={4, 5}, name="small three on one position",
                  want=[(5, "dup-skip", "dup@t")]))
    out.append(of([80, 90, 50, 0, 10, 20, 30, 40, 60, 70, 100, 110, 120, 130], name="small two breaks in a row",
                  want=[(1, "break", "pos"), (2, "break", "pos")]))
    out.append(of([50, 60, 70, 30, 0, 40, 80, 90, 100, 110, 120, 130, 140, 150], name="small filter behind a break",
                  want=[(2, "break", "pos"), (3, "filter-next", "pos")]))
    # a dropped element right in front of a break (or of the end) cannot be: see test_nothing_dropped_in_front_of_a_break.  The nearest
    # there is: the block's last hit stands behind a dropped one
    out.append(of([30, 40, 50, 45, 60, 10, 20, 25, 27, 70, 80, 90, 100, 110], name="small dropped one before a block's last",
                  want=[(2, "filter-next", "pos"), (4, "break", "pos")]))
    return out


# ---------------------------------------------------------------- (b) thresholds and votes

THRESHOLDS = {4: {3: "mode1", 2: "mode3", 1: "mode2"}, 8: {6: "mode1", 5: "mode3", 3: "mode3", 2: "mode2"},
              7: {6: "mode1", 5: "mode3", 2: "mode3", 1: "mode2"}}


def threshold_specs():
    """nt transitions, `ups` of them rising: the rising ones first.  What the mode must be is worked out by hand above: 3 of 4 and 6 of 8
    are the threshold itself, 5 of 8 and 5 of 7 one transition below, 6 of 7 the first above; and the same from the other side"""
    out = []
    for nt, row in THRESHOLDS.items():
        for ups, path in row.items():
            down = nt - ups
            out.append(of([10 * x for x in list(range(down, nt + 1)) + list(range(down - 1, -1, -1))], want=None, path=path, name=f"threshold {ups} of {nt}"))
    return out


def vote_spec():
    """three blocks of 4, 5 and 7 hits: 2 of 4 equal strands (exactly half: +), 2 of 5 (one below half: -), 7 of 7; the run as a whole
    has 11 of 16 (+), the opposite of the middle block's sign"""
    vals = [100, 110, 120, 130, 50, 60, 70, 80, 90, 0, 10, 20, 30, 40, 140, 150]
    same = [True, False, True, False] + [True, False, False, True, False] + [True] * 7
    return of(vals, same=same, name="vote", want=[(3, "break", "pos"), (8, "break", "pos")])


# ---------------------------------------------------------------- (c) the seams

def seam_specs(m):
    """runs of m hits, in sorted read order but for what is planted: every kind at every t of SEAM_T that has room, each with one of the
    three end events; a pair on sorted 63 / 64 with each end event; for the short m the end events are the ones at SEAM_T"""
    out = []
    for n, (kind, t) in enumerate(itertools.product(KINDS, SEAM_T)):
        sp = base(m, f"seam m={m} {kind} t={t}")
        if t + 3 > m - 6 or not plant(sp, kind, t):
            continue
        assert plant_end(sp, 1 + n % 3)
        out.append(sp)
    for back in (1, 2, 3):
        sp = base(m, f"seam m={m} end -{back}")
        assert plant_end(sp, back)
        out.append(sp)
    for back in (1, 2, 3):
        sp = base(m, f"seam m={m} pair 63/64 end -{back}")
        paired = plant_pair(sp, 64)
        if not plant_end(sp, back):
            assert paired and plant_front(sp)
        if m >= 100:
            assert plant(sp, KINDS[back - 1], 30 + back)
        out.append(sp)
    return out


# ---------------------------------------------------------------- (d) long runs, several runs

def long_specs(m):
    """general-path runs of m hits with an event at both ends and at every staging boundary below m: one run per kind, the kinds
    going round over the boundaries and the three places at each"""
    seams = [b for b in (256, 512, 1024) if b < m]
    out = []
    for n, kind in enumerate(KINDS):
        sp = base(m, f"long m={m} #{n}")
        assert plant_front(sp)
        for q, b in enumerate(seams):
            t = b - (n + q) % 2 if b == 1024 else b + (n + q) % 3 - 1
            plant(sp, KINDS[(n + q) % len(KINDS)], t)   # (no room at the last seam of 257 and 513: the end events are there)
        assert any(plant_end(sp, back) for back in (1 + n % 3, 1, 2, 3))
        out.append(sp)
    return out


def zigzag(m, name):
    """0 9 1 8 2 7 ..: as many transitions one way as the other, no record"""
    lo, hi = iter(range(m)), iter(range(10 * m, 0, -1))
    return of([next(lo) if i % 2 == 0 else next(hi) for i in range(m)], path="mode3", name=name)


def five_runs(first, big=False):
    """fast path (`first` hits), three blocks, mode 3, two blocks, fast path down: [(spec, down)]"""
    sizes = (500, 100, 490, 1100 - 1090 - first) if big else (16, 6, 14, 4)
    three = base(sizes[0], f"five three blocks {first} {big}")
    assert plant(three, "break", 125 if big else 3) and plant(three, "break", 300 if big else 9)
    two = base(sizes[2], f"five two blocks {first} {big}")
    assert plant(two, "break", 255 if big else 7)
    if big:
        assert plant(three, "filter-next", 255) and plant(three, "dup-t2-next", 63) and plant_end(three, 3) and plant(two, "filter-current", 64)
    return [base(first, f"five up {first}", "fast-up" if first > 1 else "one-hit"), three, zigzag(sizes[1], f"five zigzag {big}"), mirror(two),
            mirror(base(sizes[3], f"five fast {first} {big}", "fast-up"))]


# ---------------------------------------------------------------- (f) a seeded random sweep

def sweep_specs(n=SWEEP_RUNS, seed=SWEEP_SEED):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        m = int(rng.integers(3, 201))
        vals, tie = [10 * j for j in range(m)], set()
        kind = ("swaps", "moved", "transposed", "dups", "shuffle", "dups near")[i % 6]
        if kind == "swaps":
            for j in rng.integers(0, m - 1, 1 + m // 12).tolist():
                vals[j], vals[j + 1] = vals[j + 1], vals[j]
        elif kind == "moved":
            x = vals.pop(int(rng.integers(0, m)))
            vals.insert(int(rng.integers(0, m)), x)
        elif kind == "transposed":
            a, b, c = sorted(rng.integers(0, m + 1, 3).tolist())
            vals = vals[:a] + vals[b:c] + vals[a:b] + vals[c:]
        elif kind == "shuffle":
            vals = rng.permutation(vals).tolist()
        else:
            tie = set(rng.integers(1, m, int(rng.integers(1, 4))).tolist())
            for _ in range(1 + m // 16):
                if kind == "dups near":    # something out of line right beside a position held twice
                    j = min(max(int(rng.choice(sorted(tie))) + int(rng.integers(-4, 4)), 0), m - 1)
                else:
                    j = int(rng.integers(0, m))
                x = vals.pop(j)
                vals.insert(min(max(j + int(rng.integers(-6, 7)), 0), m - 1), x)
        sp = of(vals, tie, want=None, path=None, name=f"sweep #{i} {kind}")
        for a, e in sp.groups():
            sp.vals[a:e + 1] = sorted(sp.vals[a:e + 1])
        out.append(mirror(sp) if rng.integers(0, 2) else sp)
    return out


# ---------------------------------------------------------------- reads: what the tests craft into a world

class Read:
    """runs: [(name, [(ctg_pos, ctg_strand, read_strand)] in read order, the spec or None)]; nmx minimizers in all (None: the hits)"""

    def __init__(self, name, specs, nmx=None):
        self.name, self.nmx = name, nmx
        self.runs = [(sp.name, hits_of(sp), sp) for sp in specs]

    def hits(self):
        return sum(len(r[1]) for r in self.runs)


def ahead(n, name):
    return base(n, f"ahead {n} {name}", "fast-up" if n > 1 else "one-hit")


@functools.lru_cache(maxsize=None)
def crafted():
    """every crafted read, by batch: {batch: [Read]}"""
    b = collections.OrderedDict()
    both = lambda sps: [x for sp in sps for x in (sp, mirror(sp))]
    small = both(small_specs())
    b["small"] = [Read(sp.name, [sp]) for sp in small] + [Read(sp.name + " s=3", [ahead(3, sp.name), sp]) for sp in small]
    tv = threshold_specs() + both([vote_spec()])
    b["votes"] = [Read(sp.name, [sp]) for sp in tv] + [Read(sp.name + " s=3", [ahead(3, sp.name), sp]) for sp in tv]
    for m in SEAM_M:
        sps = both(seam_specs(m))
        b[f"seam-{m}"] = [Read(f"seam m={m} reads {i}", sps[i:i + 2]) for i in range(0, len(sps), 2)]   # s = 0 and s = m
    part = [sp for sp in both(seam_specs(130)) if " t=63" in sp.name or " t=64" in sp.name or "pair" in sp.name]
    for nmx in (300, 600):
        b[f"class-{nmx}"] = [Read(f"{sp.name} in {nmx} s={s}", [ahead(s, f"{sp.name} {nmx}"), sp], nmx) for sp in part for s in (2, 3)]
    for m in (257, 513, 1030):
        sps = long_specs(m)
        sps = [mirror(sp) if i % 2 else sp for i, sp in enumerate(sps)]
        b[f"long-{m}"] = [Read(sp.name, [sp]) for sp in sps] + \
                         [Read(f"{sp.name} s={s}", [ahead(s, f"{sp.name} {s}"), sp]) for i, sp in enumerate(sps) for s in ((4, 7) if i < 3 else ())]
    b["five"] = [Read(f"five s={s}", five_runs(s)) for s in (3, 4)]
    b["five-1100"] = [Read(f"five 1100 s={s}", five_runs(s, True)) for s in (3, 4)]
    return b


@functools.lru_cache(maxsize=None)
def sweep():
    sps = sweep_specs()
    return [Read(f"sweep reads {i}", sps[i:i + 3]) for i in range(0, len(sps), 3)]


def fixture_cases():
    """what the reference's print_paf is run over for tests/golden/gen/paf_blocks.json: every run of (a) - (c) and the sweep's first 50"""
    b = crafted()
    runs = [r for name in ["small", "votes"] + [f"seam-{m}" for m in SEAM_M] for rd in b[name] for r in rd.runs if not r[0].startswith("ahead")]
    runs += [r for rd in sweep() for r in rd.runs][:50]
    seen, out = set(), []
    for name, run, _ in runs:
        if name not in seen:
            seen.add(name)
            out.append((name, alone(run)))
    return out


# ---------------------------------------------------------------- a world's reads as the map sees them

def runs_in_world(w, rid, repeat_filter=False):
    """the hits of read `rid` of a GWorld, by run: [(contig, [(ctg_pos, read_pos, ctg_strand, read_strand)])]"""
    if getattr(w, "_paf_inv", None) is None or len(w._paf_inv) != len(w.at):
        strand = {(c, pos): cs for c, recs in enumerate(w.ctgs) for _, pos, cs in recs}
        w._paf_inv = {key: (c, pos, strand[c, pos]) for (c, pos), key in w.at.items()}
    hits = [w._paf_inv[key] + (RSTEP * i, rs) for i, (key, rs) in enumerate(w.reads[rid]) if key in w._paf_inv]
    if repeat_filter:
        seen = collections.Counter((h[0], h[1]) for h in hits)
        hits = [h for h in hits if seen[h[0], h[1]] == 1]
    return [(c, [(pos, rp, cs, rs) for _, pos, cs, rp, rs in g]) for c, g in itertools.groupby(hits, key=lambda h: h[0])]
