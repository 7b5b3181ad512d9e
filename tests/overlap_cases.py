"""Crafted keys for the overlap stage's per-sequence sub-tables (csrc/overlap_kernels.h: ovl_insert_kernel, ovl_resolve_kernel,
ovl_gather_kernel behind ntl_overlap_filter).  Sequence s owns the slots [2 * mx_off[s], 2 * mx_off[s + 1]) of one array, a key's home
in them comes from its high word alone, and real or random hashes leave every sub-table half empty with probe sequences of one or two
slots.  Here the keys are chosen: clusters of one high word at the last slot of a sub-table (they wrap to its slot 0, and the slot
behind the last one is the NEXT sequence's) and in its middle, keys inserted 2, 3 and 200 times inside such clusters, the same keys in
the sequences on either side, the key 2^64 - 1 (the empty marker: counted beside the table), sub-tables of two and four slots, records
on and beside the ends of their regions, record counts round the 256 lanes of a workgroup and a scan tile.  Every batch is a set of
arrays for sketch_from_arrays -> overlap_filter with what oracle.overlap_filter (np.unique per sequence: no table, no marker) makes of
them; the strands, which the oracle does not return, are the input's at the kept records.

home() restates ovl_home; tests/test_overlap_edges.py::test_source_literals holds it to the source."""
import functools

import numpy as np

import oracle

M32 = (1 << 32) - 1
ALL_ONES = (1 << 64) - 1             # NTL_INF, the empty marker: counted per sequence in OvlArgs::side
HW_LAST = 0xFFFFFFFF                # home = the last slot of any sub-table
HW_MID = 0x80000000                 # home = slot `count` of a sub-table of 2 * count slots
LAST_ZERO = HW_LAST << 32           # the smallest key of HW_LAST
WHOLE = ((0, 10 ** 6),)


def home(key, size):
    """ovl_home: the high word spread over the `size` = 2 * count slots of the sequence's sub-table"""
    return ((key >> 32) * size) >> 32


def probe(keys, size):
    """Linear-probe inserts of `keys` in that order (repeats and the all-ones key take no slot) -> ({key: slot}, whether a probe
    sequence stepped from the last slot to slot 0).  The occupied slots, and whether one wraps, do not depend on the order."""
    slots, occ, wrapped = {}, set(), False
    for key in keys:
        if key in slots or key == ALL_ONES:
            continue
        j = home(key, size)
        while j in occ:
            j += 1
            if j == size:
                j, wrapped = 0, True
        occ.add(j)
        slots[key] = j
    return slots, wrapped


def kept_indices(mx_off, mx_hash, pos, e_off, eh, ep):
    """Where in the input the records lie that oracle.overlap_filter kept (it returns hashes and positions, no strands): a kept hash is
    the only one of its value among its sequence's valid records, and a record of the same hash and position would be valid with it,
    so (hash, position) names one record of the sequence."""
    mx_hash, pos = np.asarray(mx_hash), np.asarray(pos)
    idx = []
    for s in range(len(mx_off) - 1):
        a, b = int(mx_off[s]), int(mx_off[s + 1])
        kh, kp = eh[int(e_off[s]):int(e_off[s + 1])], ep[int(e_off[s]):int(e_off[s + 1])]
        if not len(kh):
            continue
        order = np.argsort(kh, kind="stable")
        assert len(np.unique(kh)) == len(kh)
        cand = a + np.flatnonzero(np.isin(mx_hash[a:b], kh))
        at = order[np.searchsorted(kh[order], mx_hash[cand])]
        mine = cand[kp[at] == pos[cand]]
        assert np.array_equal(mx_hash[mine], kh) and np.array_equal(pos[mine], kp), "one record each, in input order"
        idx.append(mine)
    return np.concatenate(idx).astype(np.int64) if idx else np.zeros(0, np.int64)


class Seq:
    """one sequence: keys, positions (10 apart from 5 unless given), regions (None: the name is in no region table); kind: what the
    oracle must make of it -- "some" (more than none, fewer than all kept), "all", "none" (records, none kept), "empty" (no records),
    "any" (records; the batch as a whole keeps some);
    kept: the number of kept records where the case knows it"""

    def __init__(self, name, keys, pos=None, regions=WHOLE, kind="some", kept=None):
        self.name, self.keys, self.kind, self.kept = name, [int(key) for key in keys], kind, kept
        self.pos = [5 + 10 * i for i in range(len(keys))] if pos is None else [int(p) for p in pos]
        self.regions = None if regions is None else [(int(a), int(b)) for a, b in regions]
        assert len(self.pos) == len(self.keys) and all(0 <= key <= ALL_ONES for key in self.keys) and all(0 <= p <= M32 for p in self.pos)

    def valid_keys(self):
        """the keys of the records inside a region, in input order: what ovl_insert_kernel puts into the sub-table"""
        return [key for key, p in zip(self.keys, self.pos) if any(a <= p <= b for a, b in self.regions or ())]

    def table(self):
        return probe(self.valid_keys(), 2 * len(self.keys))


class Batch:
    """the sequences of one call, in order; the strands are random bits"""

    def __init__(self, name, seqs, seed, kind="some"):
        self.name, self.seqs, self.kind = name, list(seqs), kind
        assert len({s.name for s in self.seqs}) == len(self.seqs)
        rng = np.random.default_rng(seed)
        self.mx_off = np.zeros(len(self.seqs) + 1, np.uint64)
        self.reg_off = np.zeros(len(self.seqs) + 1, np.uint64)
        if self.seqs:
            np.cumsum([len(s.keys) for s in self.seqs], out=self.mx_off[1:])
            np.cumsum([len(s.regions or ()) for s in self.seqs], out=self.reg_off[1:])
        self.hash = np.array([key for s in self.seqs for key in s.keys], np.uint64)
        self.pos = np.array([p for s in self.seqs for p in s.pos], np.uint32)
        self.strand = rng.integers(0, 2, len(self.hash)).astype(np.uint8)
        self.starts = np.array([a for s in self.seqs for a, _b in s.regions or ()], np.uint32)
        self.ends = np.array([b for s in self.seqs for _a, b in s.regions or ()], np.uint32)
        self.regions = [s.regions for s in self.seqs]
        self._exp = None

    def expected(self):
        """(offsets, hashes, positions, strands) of the kept records by the oracle, made once; the conditions of the cases are asserted
        here, on the oracle's output alone"""
        if self._exp is None:
            e_off, eh, ep = oracle.overlap_filter(self.mx_off, self.hash, self.pos, self.regions)
            es = self.strand[kept_indices(self.mx_off, self.hash, self.pos, e_off, eh, ep)]
            assert len(e_off) == len(self.seqs) + 1 and int(e_off[-1]) == len(eh) == len(ep) == len(es)
            for s, seq in enumerate(self.seqs):
                kept, n = int(e_off[s + 1] - e_off[s]), len(seq.keys)
                ok = {"some": 0 < kept < n, "all": kept == n > 0, "none": kept == 0 < n, "empty": kept == n == 0, "any": n > 0}[seq.kind]
                assert ok and (seq.kept is None or seq.kept == kept), f"{self.name}, {seq.name}: the oracle keeps {kept} of {n}, the case says {seq.kind}, {seq.kept}"
            n = len(self.hash)
            assert {"some": 0 < len(eh) < n, "empty": len(eh) == n == 0}[self.kind], (self.name, len(eh), n)
            self._exp = (e_off, eh, ep, es)
        return self._exp


# ---------------------------------------------------------------- keys

def cluster(hw, n, rng, avoid=()):
    """n distinct keys of the high word hw, none all-ones, none in `avoid`"""
    out = []
    while len(out) < n:
        key = (hw << 32) | int(rng.integers(1, M32))
        if key not in out and key not in avoid:
            out.append(key)
    return out


def random_keys(n, rng, avoid=()):
    """n distinct random keys whose high words are neither HW_LAST nor HW_MID"""
    out = []
    while len(out) < n:
        key = (int(rng.integers(0, 1 << 32)) << 32) | int(rng.integers(0, 1 << 32))
        if key >> 32 not in (HW_LAST, HW_MID) and key not in out and key not in avoid:
            out.append(key)
    return out


def shuffled(keys, rng):
    return [keys[i] for i in rng.permutation(len(keys))]


def filler(n, rng):
    """n random records and one more key twice: whatever joins them, the sequence keeps some and drops some"""
    keys = random_keys(n + 1, rng)
    return keys + [keys[-1]]


# ---------------------------------------------------------------- cases 1 .. 5: one batch

CLUSTER_SIZES = (3, 9, 40)
N_TWICE = {3: 1, 9: 2, 40: 5}
N_RANDOM = 30


def _dup_seq(name, hw, n, rng):
    """case 1: a cluster of n keys of one high word -- N_TWICE[n] of them twice, one three times, one 200 times, the rest once --
    among thirty random keys, in random order"""
    keys = cluster(hw, n, rng)
    times = [2] * N_TWICE[n] + [3, 200] + [1] * (n - N_TWICE[n] - 2)
    others = random_keys(N_RANDOM, rng)
    recs = shuffled([key for key, t in zip(keys, times) for _ in range(t)] + others, rng)
    seq = Seq(name, recs, kept=N_RANDOM + times.count(1))
    slots, wrapped = seq.table()
    size = 2 * len(recs)
    span = {(home(keys[0], size) + i) % size for i in range(n)}
    assert span <= set(slots.values()) and wrapped == (hw == HW_LAST), name
    assert home(keys[0], size) == (size - 1 if hw == HW_LAST else size // 2), name
    # n keys of one home: whatever the order of the inserts, all but one lie behind their home -- some duplicated key among them
    assert sum(1 for t in times if t > 1) >= 2, name
    return seq, keys


def _once_seq(name, keys, rng):
    """case 2: the keys of a neighbour's cluster, once each, among twenty random ones: all kept"""
    seq = Seq(name, shuffled(keys + random_keys(20, rng), rng), kind="all")
    assert seq.table()[1] == (keys[0] >> 32 == HW_LAST), name
    return seq


def crafted_batch():
    rng = np.random.default_rng(4100)
    seqs = [Seq("4-first-of-the-batch-empty", [], kind="empty")]
    # 1, 2: every wrapping cluster between a sequence that holds its keys once each in front of it and one behind it
    for n in CLUSTER_SIZES:
        dup, keys = _dup_seq(f"1-last-slot-{n}", HW_LAST, n, rng)
        seqs += [_once_seq(f"2-in-front-of-{n}", keys, rng), dup, _once_seq(f"2-behind-{n}", keys, rng)]
        # ... and behind that one, which wraps as well, up to eight of the keys alone in sub-tables of two slots: were a probe to walk on
        # into the next sequence's slots, the n - 1 keys that should wrap would lie across these, each on the path of its own copy here
        seqs += [Seq(f"2-behind-{n}-alone-{i}", [keys[i]], kind="all") for i in range(min(n, 8))]
    for n in CLUSTER_SIZES:
        dup, keys = _dup_seq(f"1-mid-table-{n}", HW_MID, n, rng)
        seqs += [dup, _once_seq(f"2-behind-mid-{n}", keys, rng)]
    # 3: the all-ones key, the key 0, the smallest key of the all-ones high word
    one = [ALL_ONES]
    seqs += [
        Seq("3-ones-absent", filler(10, rng), kept=10),
        Seq("3-ones-once", shuffled(filler(10, rng) + one, rng), kept=11),
        Seq("3-ones-twice", shuffled(filler(10, rng) + one * 2, rng), kept=10),
        Seq("3-ones-three-times", shuffled(filler(10, rng) + one * 3, rng), kept=10),
        Seq("3-ones-twice-one-outside", filler(4, rng) + one + random_keys(3, rng) + one, regions=[(0, 70)], kept=5),
        Seq("3-ones-alone", one, kind="all"),
        Seq("3-ones-adjacent-a", shuffled(filler(6, rng) + one, rng), kept=7),
        Seq("3-ones-adjacent-b", shuffled(filler(6, rng) + one, rng), kept=7),
        Seq("3-zero-and-last-zero-once", shuffled(filler(6, rng) + one + [0, LAST_ZERO] + cluster(HW_LAST, 3, rng), rng), kept=12),
        Seq("3-zero-and-last-zero-twice", shuffled(filler(6, rng) + one + [0, LAST_ZERO] * 2 + cluster(HW_LAST, 3, rng), rng), kept=10),
        Seq("3-last-zero-alone", [LAST_ZERO], kind="all"),
        Seq("3-zero-alone", [0], kind="all"),
    ]
    assert seqs[-4].table()[1] and seqs[-3].table()[1]  # the all-ones high word: both wrap
    # 4: sizes
    pair_last, pair_mid = cluster(HW_LAST, 2, rng), cluster(HW_MID, 2, rng)
    twin = random_keys(1, rng)
    seqs += [
        Seq("4-one-record", random_keys(1, rng), kind="all"),
        Seq("4-no-record-between", [], kind="empty"),
        Seq("4-two-equal", twin * 2, kind="none"),
        Seq("4-two-of-one-high-word-last", pair_last, kind="all"),
        Seq("4-two-of-one-high-word-mid", pair_mid, kind="all"),
        Seq("4-two-equal-last", pair_last[:1] * 2, kind="none"),
    ]
    assert seqs[-3].table() == ({pair_last[0]: 3, pair_last[1]: 0}, True) and seqs[-2].table() == ({pair_mid[0]: 2, pair_mid[1]: 3}, False)
    # 5: regions
    k = random_keys(40, rng)
    seqs += [
        Seq("5-on-and-beside-the-ends", k[0:5], pos=[99, 100, 150, 200, 201], regions=[(100, 200)], kept=3),
        Seq("5-start-equals-end", k[5:8], pos=[299, 300, 301], regions=[(300, 300)], kept=1),
        Seq("5-overlapping-regions", k[8:12], pos=[399, 475, 520, 551], regions=[(400, 500), (450, 550), (470, 480)], kept=2),
        Seq("5-regions-none", k[12:16], regions=None, kind="none"),
        Seq("5-regions-empty", k[16:20], regions=[], kind="none"),
        Seq("5-region-beyond-the-last-position", k[20:24], regions=[(10 ** 6, 2 * 10 ** 6)], kind="none"),
        Seq("5-position-0", k[24:26], pos=[0, 1], regions=[(0, 0)], kept=1),
        Seq("5-position-max", k[26:29], pos=[M32 - 10, M32 - 9, M32], regions=[(M32 - 9, M32)], kept=2),
        Seq("5-duplicate-outside", [k[30], k[31], k[32], k[30], k[33], k[32]], pos=[110, 120, 130, 250, 140, 150], regions=[(100, 200)], kept=3),
        Seq("5-duplicate-outside-in-a-cluster", pair_last + cluster(HW_LAST, 3, rng, avoid=pair_last) + pair_last, pos=[10, 20, 30, 40, 50, 300, 60],
            regions=[(0, 100)], kept=4),
    ]
    assert seqs[-1].table()[1]
    seqs += [Seq("4-behind-the-last-cluster", filler(5, rng)), Seq("4-last-of-the-batch-empty", [], kind="empty")]
    batch = Batch("crafted", seqs, 4101)
    # every sequence whose cluster wraps is followed by another one's slots
    assert all(i + 1 < len(seqs) and len(seqs[i + 1].keys) for i, s in enumerate(seqs) if s.keys and s.table()[1])
    assert sum(1 for s in seqs if s.keys and s.table()[1]) >= 12
    return batch


# ---------------------------------------------------------------- cases 6, 7: keys of a small pool

def pool_keys(rng):
    """8 high words x 16 low words: the all-ones high word, its neighbour, the middle, 0 and four random ones; the low word 0 among
    the sixteen (so the keys 0 and LAST_ZERO are in the pool)"""
    highs = [HW_LAST, HW_LAST - 1, HW_MID, 0] + [int(x) for x in rng.integers(1, HW_LAST - 1, 4)]
    lows = [0, 1] + [int(x) for x in rng.integers(2, M32, 14)]
    assert len(set(highs)) == 8 and len(set(lows)) == 16
    return highs, lows


def pool_seq(name, n, rng, highs, lows, p_ones=0.03):
    """n records of 1, 2 or all 8 of the pool's high words, the all-ones key at 3 % of the places; positions 1 .. 40 apart; regions
    as parity_cases.check_overlap_random draws them: none / empty / one to three, overlapping and beyond the end at times"""
    mine = [highs[i] for i in rng.permutation(8)[:(1, 2, 8)[int(rng.integers(0, 3))]]]
    keys = [ALL_ONES if rng.random() < p_ones else (mine[int(rng.integers(0, len(mine)))] << 32) | lows[int(rng.integers(0, 16))] for _ in range(n)]
    pos = np.cumsum(rng.integers(1, 41, n)).tolist()
    length = (pos[-1] if n else 0) + 20
    r = rng.random()
    if r < 0.2:
        regions = None
    elif r < 0.3:
        regions = []
    else:
        regions = [tuple(sorted(int(x) for x in rng.integers(0, length + 100, 2))) for _ in range(int(rng.integers(1, 4)))]
    return Seq(name, keys, pos=pos, regions=regions, kind="any" if n else "empty")


class PoolBatch(Batch):
    def __init__(self, name, counts, seed):
        rng = np.random.default_rng(seed)
        highs, lows = pool_keys(rng)
        super().__init__(name, [pool_seq(f"{name}-seq{i}", int(n), rng, highs, lows) for i, n in enumerate(counts)], seed + 1)

    def reach(self):
        """(sequences whose valid records hold a cluster that crosses the end of its sub-table, sequences whose valid records hold
        the all-ones key)"""
        return sum(1 for s in self.seqs if s.keys and s.table()[1]), sum(1 for s in self.seqs if ALL_ONES in s.valid_keys())


def _counts(total, parts, rng):
    """`parts` counts that sum to `total`, a zero among them"""
    cuts = np.sort(rng.integers(0, total + 1, parts - 2))
    counts = np.diff(np.concatenate([[0], cuts, [total]])).tolist()
    counts.insert(int(rng.integers(1, parts - 1)), 0)
    assert sum(counts) == total and len(counts) == parts
    return counts


def total_batch(total):
    """case 6: 255, 256, 257 records in all -- the last lane of the first workgroup idle, busy, and one record in a second workgroup"""
    batch = PoolBatch(f"total-{total}", _counts(total, 9, np.random.default_rng(6000 + total)), 6100 + total)
    assert len(batch.hash) == total
    return batch


def boundary_batch():
    """a sequence ends with record 255 and the next one starts with record 256: the first lane of the second workgroup"""
    batch = PoolBatch("boundary-at-256", [50, 60, 0, 146, 57, 31, 0, 40], 6256)
    assert 256 in batch.mx_off.tolist() and len(batch.hash) > 256 + 57
    return batch


def geometry_batch(which):
    """about 5000 records over 300 sequences (three scan tiles; n > nseq + 1: the gather's grid is sized by the records), and 300 records
    over 2500 sequences, most of them empty (nseq + 1 > n: its grid is sized by the offsets, more than one scan tile of them)"""
    rng = np.random.default_rng(6500)
    if which == "records":
        batch = PoolBatch("geometry-records", rng.integers(0, 35, 300).tolist(), 6501)
        assert 4500 < len(batch.hash) < 5600 and len(batch.hash) > 2 * 2048 and len(batch.seqs) == 300
    else:
        counts = np.zeros(2500, np.int64)
        counts[rng.choice(2500, 60, replace=False)] = 5
        counts[[0, 2499]] = 0
        batch = PoolBatch("geometry-offsets", counts.tolist(), 6502)
        assert 280 <= len(batch.hash) <= 300 and len(batch.seqs) + 1 > 2048 > len(batch.hash)
    return batch


MIN_WRAPPING, MIN_ALL_ONES = 20, 20


def random_batch():
    """case 7: 300 sequences of 0 .. 60 records"""
    rng = np.random.default_rng(7000)
    batch = PoolBatch("random-300", rng.integers(0, 61, 300).tolist(), 7001)
    wrapping, ones = batch.reach()
    assert wrapping >= MIN_WRAPPING and ones >= MIN_ALL_ONES, (wrapping, ones)
    assert sum(1 for s in batch.seqs if not s.keys) >= 1
    return batch


def empty_batch(nseq):
    """no sequences at all; sequences without any record (region lists for some of them all the same)"""
    seqs = [Seq(f"no-record-{i}", [], regions=(None, [], [(0, 100)])[i % 3], kind="empty") for i in range(nseq)]
    return Batch(f"empty-{nseq}-sequences", seqs, 8000 + nseq, kind="empty")


BATCHES = {"crafted": crafted_batch}
BATCHES.update({f"total-{n}": functools.partial(total_batch, n) for n in (255, 256, 257)})
BATCHES["boundary-at-256"] = boundary_batch
BATCHES["geometry-records"] = functools.partial(geometry_batch, "records")
BATCHES["geometry-offsets"] = functools.partial(geometry_batch, "offsets")
BATCHES["random-300"] = random_batch
BATCHES["empty-0-sequences"] = functools.partial(empty_batch, 0)
BATCHES["empty-7-sequences"] = functools.partial(empty_batch, 7)


@functools.lru_cache(maxsize=None)
def batch(name):
    """the batch of that name, built once (the mock half and the GPU half share it and its expected records)"""
    return BATCHES[name]()
