"""Crafted map results for ntl_mapres_liftover (tests/test_liftover_device.py), and a plain-Python restatement of the reference's
liftover over records: liftover_ctg_mappings and print_adjusted_mappings of bin/ntlink_liftover_mappings.py:61-121 as they are worded
there -- itertools.groupby into runs, a dict of the runs' first indices with subsumed flags by name, groupby again over the lines that
stay, concatenation, the two all() over neighbours.  No device, no library."""
import itertools

import numpy as np

from ntlink_amd import capi

K = 32
LANE_LINES = capi.NTL_LIFT_LANE_LINES

# contig id -> (path id, scaf_start, ctg_start, ctg_end, orientation): what liftover.read_agp returns
AGP = {
    "a1": ("A", 1, 1, 1000, "+"),        # lifted = pos
    "a2": ("A", 1101, 1, 1000, "-"),     # lifted = 1100 + (1000 - pos) - K, strand flipped
    "a3": ("A", 2201, 11, 1010, "+"),    # lifted = 2200 + (pos - 10) for 10 <= pos <= 978
    "b1": ("B", 1, 1, 5000, "+"),
    "c1": ("C", 51, 1, 5000, "-"),
    "keep1": ("keep1", 301, 101, 900, "-"),  # path id == contig id: positions and strands stay, whatever the orientation
    "odd1": ("O", 301, 101, 900, "?"),       # an orientation that is neither + nor -: the same
    "short": ("S", 1, 1, 20, "+"),           # K is longer than the component: nothing is kept
}
CONTIGS = list(AGP) + ["x1", "x2"]  # x1, x2: not in the AGP


def inc(n, start=100, step=3, cs=1, rs=1):
    return [(start + i * step, (cs + i) & 1 if cs == 2 else cs, 7 + 5 * i, rs) for i in range(n)]


def dec(n, start=900, step=3, cs=0, rs=1):
    return [(start - i * step, cs, 7 + 5 * i, rs) for i in range(n)]


def crafted_reads():
    """-> list of (label, [(contig, hits), ...])"""
    R = []
    for n in (1, 63, 64, 65, 129):
        R.append((f"{n}-hits-shift", [("a1", inc(n, cs=2))]))
        R.append((f"{n}-hits-mirror", [("a2", inc(n, cs=2))]))       # increasing in, decreasing out
        R.append((f"{n}-hits-every-other-kept", [("a3", [(5 + 5 * i if i % 2 else 2000 + i, 1, i, 0) for i in range(n)])]))
    R.append(("bounds", [("a3", [(9, 1, 1, 1), (10, 1, 2, 1), (978, 0, 3, 1), (979, 1, 4, 1)])]))  # ctg_start-2, ctg_start-1, ctg_end-k, +1
    R.append(("bounds-mirror", [("c1", [(0, 1, 1, 1), (4968, 1, 2, 0), (4969, 1, 3, 1)])]))
    R.append(("k-longer-than-component", [("short", inc(4, start=0, step=1))]))
    R.append(("mode0", [("x1", inc(3))]))
    R.append(("mode1-minus", [("keep1", [(99, 1, 1, 1), (100, 1, 2, 1), (500, 0, 3, 0), (868, 1, 4, 1), (869, 1, 5, 1)])]))
    R.append(("mode1-other-orientation", [("odd1", dec(5, start=800, step=100))]))
    R.append(("equal-positions", [("a1", [(100, 1, 1, 1), (100, 1, 2, 1)])]))
    R.append(("equal-positions-across-join", [("a1", [(100, 1, 1, 1)]), ("a1", [(100, 1, 2, 1)])]))
    R.append(("single-hit", [("b1", [(77, 0, 9, 1)])]))
    R.append(("all-filtered", [("a3", [(1, 1, 1, 1), (5, 1, 2, 1), (2000, 1, 3, 1)])]))
    R.append(("up-then-down", [("b1", [(10, 1, 1, 1), (20, 1, 2, 1), (15, 1, 3, 1)])]))
    # the run patterns
    one = lambda c, p: (c, [(p, 1, p, 1)])
    R.append(("A-B-A", [("a1", inc(3)), ("b1", inc(2)), ("a3", inc(3))]))                       # B subsumed, A joined over it
    R.append(("A-X-A", [("a1", inc(3)), ("x1", inc(2)), ("a3", inc(3))]))
    R.append(("X-A-X", [("x1", inc(2)), ("a1", inc(3)), ("x1", inc(1))]))                       # A subsumed by the absent contig
    R.append(("X1-A-X2", [("x1", inc(2)), ("a1", inc(3)), ("x2", inc(1))]))                     # A stays
    R.append(("A-B-A-B", [one("a1", 100), one("b1", 100), one("a1", 200), one("b1", 200)]))     # each subsumes the other
    R.append(("A-B-A-C-A", [one("a1", 100), one("b1", 1), one("a1", 200), one("c1", 1), one("a1", 300)]))  # A subsumes itself
    R.append(("A-A-B", [("a1", inc(3)), ("a3", inc(2)), ("b1", inc(2))]))
    R.append(("A-B-B-A-C", [one("a1", 100), one("b1", 1), one("b1", 2), one("a1", 200), one("c1", 1)]))
    # joins
    R.append(("three-lines-increasing", [("a1", inc(2, 100, 100)), ("a1", [(300, 1, 3, 1)]), ("a3", inc(3))]))
    R.append(("three-lines-broken-join", [("a1", inc(2, 500, 100)), ("a3", inc(3)), ("a1", inc(2, 100, 100))]))
    R.append(("empty-middle-line", [("a1", [(100, 1, 1, 1)]), ("a3", [(1, 1, 2, 1)]), ("a3", [(500, 1, 3, 1)])]))
    R.append(("empty-first-line", [("a3", [(1, 1, 2, 1)]), ("a1", [(100, 1, 1, 1)])]))
    R.append(("three-lines-decreasing", [("a3", [(20, 1, 1, 1)]), ("a2", inc(2, 100, 100)), ("a1", dec(2, 300, 100))]))
    R.append(("decreasing-lines-increasing-join", [("a1", dec(2, 300, 100)), ("a3", dec(2, 300, 100))]))
    # 1, 2, threshold - 1, threshold, threshold + 1 lines (the overflow kernel), and beyond one lane stride of it
    for n in (1, 2, LANE_LINES - 1, LANE_LINES, LANE_LINES + 1, 70):
        R.append((f"{n}-lines-one-group", [("a1", [(50 + 10 * i, 1, i, 1)]) for i in range(n)]))
        R.append((f"{n}-lines-B-A..A-B", [("b1", [(100, 1, 1, 1)])] + [("a1", [(50 + 10 * i, 1, i, 1)]) for i in range(n - 2)] +
                  ([("b1", [(200, 1, 2, 1)])] if n > 1 else [])))
    R.append(("70-lines-alternating-inside-C", [one("c1", 10)] + [one("a1" if i % 2 else "b1", 100 + i) for i in range(68)] + [one("c1", 20)]))
    R.append(("70-lines-two-groups", [one("a1", 100 + i) for i in range(35)] + [one("b1", 900 - i) for i in range(35)]))
    R.append(("40-lines-A-kept-between-X1-X2", [one("x1", 1)] + [one("a1", 100 + i) for i in range(38)] + [one("x2", 1)]))
    return R


GAPS = (3, 0, 1, 64, 0, 300, 2)  # unused slots in front of region i (cycling); 5 more behind the last region


def build(reads, contigs=CONTIGS, gaps=GAPS, tail=5):
    """reads: [[(contig name, hits), ...], ...] -> (maps MAPPING_DT, hit_slots HIT_DT): regions ascend, unused slots hold rubbish"""
    number = {c: i for i, c in enumerate(contigs)}
    maps, slots = [], []
    junk = (0xDEADBEEF, 0xFEEDF00D, 1, 0, (0, 0))
    for r, lines in enumerate(reads):
        for ctg, hits in lines:
            slots += [junk] * gaps[len(maps) % len(gaps)]
            maps.append((r, number[ctg], len(hits), 0, len(slots)))
            slots += [(p, rp, cs, rs, (0, 0)) for p, cs, rp, rs in hits]
    slots += [junk] * tail
    return np.array(maps, capi.MAPPING_DT), np.array(slots, capi.HIT_DT)


# ---------------------------------------------------------------- the reference's wording, over records

def lift_line(ctg, hits, agp, k):
    "liftover_ctg_mappings (:61-85) -> (new_ctg_id, adjusted mappings)"
    if ctg not in agp:
        return ctg, []
    path_id, scaf_start, ctg_start, ctg_end, orientation = agp[ctg]
    adjusted = []
    for ctg_pos, ctg_strand, read_pos, read_strand in hits:
        if not ctg_start - 1 <= ctg_pos <= ctg_end - k:
            continue
        adjust_pos = ctg_pos - (ctg_start - 1)
        offset = scaf_start - 1
        if orientation == "+" and path_id != ctg:
            adjusted.append((offset + adjust_pos, ctg_strand, read_pos, read_strand))
        elif orientation == "-" and path_id != ctg:
            adjusted.append((offset + (ctg_end - ctg_start + 1 - adjust_pos) - k, 1 - ctg_strand, read_pos, read_strand))
        else:
            adjusted.append((ctg_pos, ctg_strand, read_pos, read_strand))
    return path_id, adjusted


def lift_read(lines, agp, k, events=None):
    "print_adjusted_mappings (:87-118) -> [(new_ctg_id, concatenated mappings), ...]"
    mappings = [lift_line(ctg, hits, agp, k) for ctg, hits in lines]
    contig_runs = [(ctg, list(tup)) for ctg, tup in itertools.groupby(mappings, lambda x: x[0])]
    contig_hits = {}
    for i, (ctg, _run) in enumerate(contig_runs):
        if ctg not in contig_hits:
            contig_hits[ctg] = {"index": i, "subsumed": False}
        else:
            for j in range(contig_hits[ctg]["index"] + 1, i):
                contig_hits[contig_runs[j][0]]["subsumed"] = True
    filtered = [m for m in mappings if not contig_hits[m[0]]["subsumed"]]
    out = []
    for ctg, tup in itertools.groupby(filtered, lambda x: x[0]):
        concat = [h for m in tup for h in m[1]]
        if not concat:
            continue
        if not all(a[0] < b[0] for a, b in zip(concat, concat[1:])) and not all(a[0] > b[0] for a, b in zip(concat, concat[1:])):
            if events is not None:
                events.add("non-monotonic")
            continue
        out.append((ctg, concat))
    if events is not None:
        if any(v["subsumed"] for v in contig_hits.values()):
            events.add("subsumed")
        if any(ctg in agp and agp[ctg][4] == "-" and agp[ctg][0] != ctg and lift_line(ctg, hits, agp, k)[1] for ctg, hits in lines):
            events.add("mirror")
    return out


def expected(reads, out_names, agp=AGP, k=K):
    "-> the dense records ntl_mapres_download must hand out"
    number = {n: i for i, n in enumerate(out_names)}
    maps, hits = [], []
    for r, lines in enumerate(reads):
        for name, concat in lift_read(lines, agp, k):
            maps.append((r, number[name], len(concat), 0, len(hits)))
            hits += [(p, rp, cs, rs, (0, 0)) for p, cs, rp, rs in concat]
    return np.array(maps, capi.MAPPING_DT), np.array(hits, capi.HIT_DT)


def verbose_text(reads, read_names):
    "the reads as lines of <prefix>.verbose_mapping.tsv"
    out = []
    for name, lines in zip(read_names, reads):
        for ctg, hits in lines:
            toks = " ".join(f"{p}:{'-+'[cs]}_{rp}:{'-+'[rs]}" for p, cs, rp, rs in hits)
            out.append(f"{name}\t{ctg}\t{len(hits)}\t{toks}\n")
    return "".join(out)


def records_text(maps, hits, read_names, out_names):
    "dense records as lines"
    out = []
    for m in maps:
        o, n = int(m["hit_off"]), int(m["n_hits"])
        toks = " ".join(f"{int(h['ctg_pos'])}:{'-+'[h['ctg_strand']]}_{int(h['read_pos'])}:{'-+'[h['read_strand']]}" for h in hits[o:o + n])
        out.append(f"{read_names[m['read']]}\t{out_names[m['ctg']]}\t{n}\t{toks}\n")
    return "".join(out)


def random_reads(seed=20, n_reads=300):
    rng = np.random.default_rng(seed)
    pool = ["a1", "a2", "a3", "b1", "c1", "keep1", "x1", "x2"]
    reads = []
    for _ in range(n_reads):
        lines = []
        for _l in range(int(rng.integers(1, 7))):
            ctg = pool[int(rng.integers(0, len(pool)))] if rng.random() < 0.7 or not lines else lines[int(rng.integers(0, len(lines)))][0]
            n = int(rng.integers(1, 9))
            pos = np.sort(rng.choice(1200, n, replace=False))
            style = rng.random()
            if style < 0.3:
                pos = pos[::-1]
            elif style < 0.4:
                rng.shuffle(pos)
            lines.append((ctg, [(int(p), int(rng.integers(0, 2)), int(rng.integers(0, 30000)), int(rng.integers(0, 2))) for p in pos]))
        reads.append(lines)
    return reads
