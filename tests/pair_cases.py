"""Crafted map results for ntl_mapres_pairs (tests/test_pair_device.py), and a plain-Python restatement of the per-read rules of the pair
tally as bin/ntlink_pair.py words them: calculate_gap_size with its assertion (:157-187), normalize_pair (:213-219), calculate_pair_info
(:222-239), add_pair (:315-334) up to the dictionary, and tally_pairs_from_mappings (:416-435) -- itertools.combinations for a short
read, the neighbours and then the neighbours among the mappings of more than one hit for a long one.  No device, no library.

A read here is (read length, [(contig number, hits), ...]) with hits = [(ctg_pos, ctg_strand, read_pos, read_strand), ...]; a contig is
(name, length)."""
import collections
import itertools

import numpy as np

from ntlink_amd import capi

K = 32
LANE_MAPS = capi.NTL_PAIR_LANE_MAPS

# names whose byte order is not their index order, a name that is a prefix of another, two contigs of one name
CONTIGS = [("ctg10", 5000), ("ctg1", 5000), ("b", 8000), ("a", 3000), ("dup", 4000), ("dup", 4000), ("z", 100000), ("Z", 2500)]
C10, C1, B, A, DUP1, DUP2, Z, ZU = range(8)


class Negative(AssertionError):
    "Gap distance estimation less than 0"


def mp(ctg, read_pos, ctg_pos=100, n=2, cs=1, rs=1, step=40):
    "a mapping of n hits from (ctg_pos, read_pos) on, `step` apart on both; n = 1: a weak one"
    return ctg, [(ctg_pos + i * step, cs, read_pos + i * step, rs) for i in range(n)]


def edge(ctg, read_pos, a=None, b=None, n=1, contigs=CONTIGS, k=K):
    """a mapping of n hits at one place whose overhang as a source is `a`, or as a target is `b`, with both strands '+':
    a = length - ctg_pos - k, b = ctg_pos"""
    clen = contigs[ctg][1]
    pos = clen - k - a if a is not None else b
    return ctg, [(pos, 1, read_pos, 1)] * n


def build(reads, gaps=(0,), tail=0, read_ids=None):
    """-> (maps MAPPING_DT, hit_slots HIT_DT): regions ascend, gaps[i % len] unused slots in front of region i and `tail` behind the
    last, all holding rubbish.  Read r has .read = read_ids[r] (default r); a read without mappings leaves no record."""
    maps, slots = [], []
    junk = (0xDEADBEEF, 0xFEEDF00D, 1, 0, (0, 0))
    for r, (_rl, lines) in enumerate(reads):
        for ctg, hits in lines:
            slots += [junk] * gaps[len(maps) % len(gaps)]
            maps.append((r if read_ids is None else read_ids[r], ctg, len(hits), 0, len(slots)))
            slots += [(p, rp, cs, rs, (0, 0)) for p, cs, rp, rs in hits]
    slots += [junk] * tail
    return np.array(maps, capi.MAPPING_DT), np.array(slots, capi.HIT_DT)


def read_lengths(reads, read_ids=None):
    n = len(reads) if read_ids is None else max(read_ids, default=-1) + 1
    out = np.zeros(n, np.uint32)
    for r, (rl, _lines) in enumerate(reads):
        out[r if read_ids is None else read_ids[r]] = rl
    return out


# ---------------------------------------------------------------- the reference's wording, over records

def read_records(read_no, lines, contigs, k, f, read_len=None, events=None):
    """The records one read adds, in order: (src, tgt, gap, read, src_ori, tgt_ori, anchor).  read_len None: the checkpoint rule
    (:460-488).  Raises Negative where calculate_gap_size asserts."""
    if read_len is None:
        read_len = max(max(hits[0][2], hits[-1][2]) for _c, hits in lines) if lines else 0
    recs = []
    ev = events if events is not None else collections.Counter()

    def add_pair(i, j, check_added=None):
        (ci, hi), (cj, hj) = lines[i], lines[j]
        last, first = hi[-1], hj[0]
        src_ori, tgt_ori = last[3] == last[1], first[3] == first[1]          # read strand == contig strand: '+'
        a = contigs[ci][1] - last[0] - k if src_ori else last[0]             # calculate_gap_size
        b = first[0] if tgt_ori else contigs[cj][1] - first[0] - k
        if a < 0 or b < 0:
            raise Negative("Gap distance estimation less than 0")
        gap = first[2] - last[2] - a - b
        if not contigs[ci][0] < contigs[cj][0]:                               # normalize_pair, on the names
            ci, cj, src_ori, tgt_ori = cj, ci, not tgt_ori, not src_ori
            swapped = True
        else:
            swapped = False
        key = (contigs[ci][0], src_ori, contigs[cj][0], tgt_ori)
        if abs(gap) > read_len:
            ev["dropped"] += 1
            return None
        if check_added is not None and key in check_added:
            ev["skipped"] += 1
            return None
        ev["swapped"] += swapped
        recs.append((ci, cj, gap, read_no, int(src_ori), int(tgt_ori), int(len(hi) > 1 and len(hj) > 1)))
        return key

    m = len(lines)
    if m < 2:
        return recs
    if m <= f:
        ev["short"] += 1
        for i, j in itertools.combinations(range(m), 2):
            add_pair(i, j)
    else:
        ev["chain"] += 1
        added = set()
        for i in range(m - 1):
            key = add_pair(i, i + 1)
            if key is not None:
                added.add(key)
        strong = [i for i in range(m) if len(lines[i][1]) > 1]
        for i, j in zip(strong, strong[1:]):
            add_pair(i, j, added)
    return recs


def records(reads, contigs, k, f, explicit=True, read_ids=None, events=None):
    "-> PAIR_REC_DT array of every read's records"
    out = []
    for r, (rl, lines) in enumerate(reads):
        out += read_records(r if read_ids is None else read_ids[r], lines, contigs, k, f, rl if explicit else None, events)
    arr = np.zeros(len(out), capi.PAIR_REC_DT)
    for i, (s, t, gap, read, so, to, anchor) in enumerate(out):
        arr[i] = (s, t, gap, read, so, to, anchor, 0)
    return arr


def export_of(recs, contigs):
    "the seven arrays PairTally.export() holds after these records: the dictionary of add_pair, keyed by NAME"
    table = {}
    for r in recs:
        key = (contigs[r["src"]][0], int(r["src_ori"]), contigs[r["tgt"]][0], int(r["tgt_ori"]))
        ent = table.setdefault(key, [int(r["src"]), int(r["tgt"]), [], 0])
        ent[2].append(int(r["gap"]))
        ent[3] += int(r["anchor"])
    src = np.array([e[0] for e in table.values()], np.uint32)
    tgt = np.array([e[1] for e in table.values()], np.uint32)
    so = np.array([key[1] for key in table], np.uint8)
    to = np.array([key[3] for key in table], np.uint8)
    anchor = np.array([e[3] for e in table.values()], np.uint32)
    goff = np.zeros(len(table) + 1, np.uint64)
    goff[1:] = np.cumsum([len(e[2]) for e in table.values()], dtype=np.uint64)
    gaps = np.array([g for e in table.values() for g in e[2]], np.int64)
    return src, so, tgt, to, anchor, goff, gaps


# ---------------------------------------------------------------- crafted reads

def chain(n, strong, ctgs=(C10, C1, B, A, Z), rl=20000, spacing=600):
    "n mappings, spaced along the read; strong(i): mapping i has two hits"
    return rl, [mp(ctgs[i % len(ctgs)], 100 + spacing * i, ctg_pos=200 + 10 * i, n=2 if strong(i) else 1) for i in range(n)]


def count_reads(f):
    "reads of 0 .. 3 mappings and of f - 1, f, f + 1 (all strong, then every third weak)"
    out = []
    for m in sorted({0, 1, 2, 3, max(f - 1, 0), f, f + 1}):
        out.append(chain(m, lambda i: True))
        out.append(chain(m, lambda i: i % 3 != 1))
    return out


def chain_reads():
    "for f = 1: every read of two or more mappings takes the second branch"
    far = 50000
    return [
        ("all-strong", chain(6, lambda i: True)),
        ("strong-weak-strong", (20000, [mp(C10, 100), mp(C1, 700, n=1), mp(B, 1300)])),
        ("two-weak-in-a-row", (20000, [mp(C10, 100), mp(C1, 700, n=1), mp(A, 1300, n=1), mp(B, 1900)])),
        ("all-weak", chain(5, lambda i: False)),
        ("one-strong", chain(5, lambda i: i == 2)),
        ("dropped-neighbour-returns", (5000, [mp(C10, 100), mp(C1, far), mp(B, far + 600)])),            # (0, 1) dropped by the gap rule, twice
        ("dropped-strong-pair-over-weak", (5000, [mp(C10, 100), mp(A, 400, n=1), mp(C1, far)])),
        ("A-B-A-B", (20000, [mp(C10, 100), mp(B, 700, n=1), mp(C10, 1300, ctg_pos=900), mp(B, 1900)])),
        ("A-B-A-B-weak-middle", (20000, [mp(C10, 100), mp(B, 700, n=1), mp(C10, 1300, ctg_pos=900, n=1), mp(B, 1900)])),  # (0, 3) under the key of (0, 1)
        ("A-A-B", (20000, [mp(C10, 100), mp(C10, 700, ctg_pos=900), mp(B, 1300)])),
        ("A-weakA-B", (20000, [mp(C10, 100), mp(C10, 700, ctg_pos=900, n=1), mp(B, 1300)])),
        ("dup-weak-dup", (20000, [mp(DUP1, 100), mp(DUP2, 700, n=1), mp(DUP1, 1300, ctg_pos=900)])),      # equal ranks: the swap, and its key
        ("dup1-x-dup2", (20000, [mp(DUP1, 100), mp(B, 700, n=1), mp(DUP2, 1300)])),
    ]


def strand_reads():
    "every strand combination of the source's last and the target's first hit, on both sides of the swap, equal names included"
    out = []
    for ci, cj in ((C1, C10), (C10, C1), (A, B), (B, A), (DUP1, DUP2), (DUP2, DUP1), (DUP1, DUP1), (Z, ZU), (ZU, Z)):
        for cs_i, rs_i, cs_j, rs_j in itertools.product((0, 1), repeat=4):
            out.append((20000, [mp(ci, 300, ctg_pos=500, cs=cs_i, rs=rs_i), mp(cj, 1500, ctg_pos=700, cs=cs_j, rs=rs_j, n=1)]))
    return out


def bound_reads(rl=1000):
    "|gap| == read length kept, read length + 1 dropped, for both signs; a == 0 and b == 0 accepted (gap = the read positions' difference)"
    out = []
    for d in (rl, rl + 1, -rl, -rl - 1, 0):
        out.append((rl, [edge(C10, 2 * rl + 10, a=0), edge(B, 2 * rl + 10 + d, b=0)]))
    out.append((rl, [edge(C10, 100, a=1), edge(B, 700, b=1, n=2)]))
    out.append((rl, [edge(C10, 100, a=-1)]))  # a negative overhang on a mapping that belongs to no pair: not an error
    return out


def negative_reads():
    "label -> reads whose only flaw is one overhang of -1 in an evaluated pair (the read in front of it makes a good pair)"
    good = (20000, [mp(C10, 100), mp(B, 700)])
    minus_b = (B, [(CONTIGS[B][1] - K + 1, 0, 700, 1)])  # target on '-': b = length - ctg_pos - k
    return {
        "a == -1": [good, (20000, [edge(C10, 100, a=-1), mp(B, 700)])],
        "b == -1": [good, (20000, [mp(C10, 100), minus_b])],
        "a == -1 behind a dropped pair": [good, (3000, [mp(C10, 100), edge(A, 50000, a=-1), mp(B, 50600)])],
    }


def launch_reads():
    T = LANE_MAPS
    out = [chain(m, lambda i: i % 4 != 2) for m in (T - 1, T, T + 1)]
    out.append(chain(130, lambda i: True, rl=200000))
    out.append(chain(130, lambda i: i % 2 == 0, rl=200000))
    out.append(chain(70, lambda i: i % 5 == 0, ctgs=(C10, B), rl=200000))  # few strong lines, far apart; repeated contigs
    return out


def many_reads(n):
    return [(5000, [mp(C10, 100 + i), mp(B, 900, n=1 + i % 2)] + ([mp(A, 1500)] if i % 5 == 0 else [])) for i in range(n)]


RANDOM_F = 3


def random_reads(seed=7, n_reads=300):
    rng = np.random.default_rng(seed)
    reads = []
    for _ in range(n_reads):
        m = int(rng.choice([1, 2, 3, 3, 4, 5, 6, 8, 12, 20]))
        lines = []
        at = int(rng.integers(0, 500))
        for _l in range(m):
            ctg = int(rng.integers(0, len(CONTIGS) - 2)) if rng.random() < 0.6 or not lines else lines[int(rng.integers(0, len(lines)))][0]
            n = int(rng.choice([1, 1, 2, 3, 5]))
            clen = CONTIGS[ctg][1]
            pos = np.sort(rng.choice(clen - K + 1, n, replace=False))
            if rng.random() < 0.4:
                pos = pos[::-1]
            cs, rs = int(rng.integers(0, 2)), int(rng.integers(0, 2))
            hits = []
            for p in pos:
                hits.append((int(p), cs, at, rs))
                at += int(rng.integers(1, 400))
            lines.append((ctg, hits))
            at += int(rng.integers(0, 3000))
        reads.append((int(rng.integers(2000, 12000)), lines))
    return reads
